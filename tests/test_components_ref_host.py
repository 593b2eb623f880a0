"""CPU: the numpy restatement of the label clean-up (tests/_components_ref.py) against scipy's answers (tests/golden/components.npz,
written by make_golden_components.py), and the host half of nas_3d_unet_amd.postprocess -- stats_of and every argument check, which
run before the library is loaded.  Everything is an integer and compared with ==."""
import os
import re

import numpy as np
import pytest

import _components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("n3d_cc_workspace_bytes", "n3d_cc_label", "n3d_cc_clean", "n3d_cc_phases")
CASES = ("box", "wide", "tall", "spiral", "diag", "wrap", "full", "checker", "empty", "single", "tie", "et_rule")


def test_fixture_matches_its_generator(golden):
    """the inputs and rule sets the fixture stores are the ones make_golden_components builds (numpy only: no scipy needed)"""
    import make_golden_components as mg
    g = golden("components")
    cases = mg.component_cases()
    assert tuple(c[0] for c in cases) == tuple(g["names"]) == CASES
    for name, labels in cases:
        assert g[name + "/labels"].dtype == np.uint8 and np.array_equal(g[name + "/labels"], labels), name
    assert [tuple(int(v) for v in r) for r in g["rules"]] == [(c, mv, int(kl), em) for c, mv, kl, em in mg.RULES]
    assert mg.STAT_KEYS == R.STAT_KEYS


@pytest.mark.parametrize("name", CASES)
def test_helper_equals_scipy(golden, name):
    g = golden("components")
    labels = g[name + "/labels"]
    for c in R.CONNECTIVITIES:
        ids = R.label(labels, c)
        assert ids.dtype == np.int32 and np.array_equal(ids, g["%s/ids_%d" % (name, c)]), (name, c)
    for k, (c, mv, kl, em) in enumerate(g["rules"]):
        out, stats = R.clean(labels, int(c), int(mv), bool(kl), int(em))
        assert np.array_equal(out, g["%s/clean_%d" % (name, k)]), (name, k)
        assert np.array_equal(R.stats_row(stats), g["%s/stats_%d" % (name, k)]), (name, k)


def test_fixture_holds_what_the_cases_are_for(golden):
    g = golden("components")
    count = lambda name, c: len(np.unique(g["%s/ids_%d" % (name, c)][g["%s/ids_%d" % (name, c)] >= 0]))
    assert [count("diag", c) for c in (6, 18, 26)] == [5, 4, 3]
    assert [count("wrap", c) for c in (6, 18, 26)] == [4, 4, 4]
    assert [count("checker", c) for c in (6, 18, 26)] == [int((g["checker/labels"] != 0).sum()), 1, 1]
    assert (g["full/labels"] != 0).all() and (g["full/ids_6"] == 0).all()
    assert (g["empty/ids_26"] == -1).all() and g["empty/stats_0"].tolist() == [0, 0, 0, 0, 0, -1, 0, 0, 0]
    # the serpentine is one component that starts at its smallest index
    wide = g["wide/ids_6"]
    start = int(np.ravel_multi_index((0, 2, 0), wide.shape))
    assert (wide[:, 2, :][g["wide/labels"][:, 2, :] != 0] == start).all() and (wide == start).sum() > 2300
    # equal sizes: the smaller id is the largest
    tie = g["tie/stats_3"]
    assert tie[4] == 8 and tie[5] == int(np.ravel_multi_index((1, 1, 1), (13, 9, 21))) and tie[1] == 1
    # et_min_voxels = e - 1, e, e + 1 with e counted in kept components only
    e = int(g["et_rule/stats_9"][7])
    assert [int(g["rules"][k][3]) for k in (8, 9, 10)] == [e - 1, e, e + 1] and int(g["et_rule/stats_9"][6]) > e
    assert [int(g["et_rule/stats_%d" % k][8]) for k in (8, 9, 10)] == [0, 0, 1]
    for name in CASES:      # every rule off: the input comes back
        assert np.array_equal(g[name + "/clean_0"], g[name + "/labels"])


def test_stats_of():
    import torch
    from nas_3d_unet_amd import postprocess as P
    from nas_3d_unet_amd._lib import N3DError
    assert P.STAT_KEYS == R.STAT_KEYS and P.REC_WORDS == 10
    rec = np.array([5, 2, 100, 90, 80, 1234, 9, 4, 1, (80 << 32) | (0xFFFFFFFF - 1234)], np.int64)
    want = {"n_components": 5, "n_kept": 2, "voxels_in": 100, "voxels_kept": 90, "largest_size": 80, "largest_id": 1234, "et_in": 9,
            "et_kept": 4, "et_relabelled": True}
    for r in (rec, rec.tolist(), torch.from_numpy(rec)):
        s = P.stats_of(r)
        assert s == want and s["et_relabelled"] is True and all(type(s[k]) is int for k in P.STAT_KEYS[:-1])
    none = P.stats_of(np.array([0, 0, 0, 0, 0, -1, 0, 0, 0, 0], np.int64))
    assert none["largest_id"] == -1 and none["n_components"] == 0 and none["et_relabelled"] is False
    with pytest.raises(N3DError, match="10 int64 words"):
        P.stats_of(rec[:9])
    with pytest.raises(N3DError, match="10 int64 words"):
        P.stats_of(rec.astype(np.float64))


def test_symbols_declared_bound_and_exported():
    from nas_3d_unet_amd import _lib, postprocess as P
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    assert "Label clean-up" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/n3d.h" % name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    for k, v in (("WORDS", P.REC_WORDS), ("COMPONENTS", P.REC_COMPONENTS), ("KEPT", P.REC_KEPT), ("VOXELS_IN", P.REC_VOXELS_IN),
                 ("VOXELS_KEPT", P.REC_VOXELS_KEPT), ("LARGEST_SIZE", P.REC_LARGEST_SIZE), ("LARGEST_ID", P.REC_LARGEST_ID),
                 ("ET_IN", P.REC_ET_IN), ("ET_KEPT", P.REC_ET_KEPT), ("ET_RELABELLED", P.REC_ET_RELABELLED), ("PACKED", P.REC_PACKED)):
        assert int(re.search(r"#define N3D_CC_REC_%s (\d+)" % k, hdr).group(1)) == v, k
    assert [P.STAT_KEYS.index(k) for k in P.STAT_KEYS] == list(range(P.REC_PACKED))
    for k, v in (("PHASES", len(P.PHASES)), ("TILED", P.TILED), ("GLOBAL_ONLY", P.GLOBAL_ONLY)):
        assert int(re.search(r"#define N3D_CC_%s (\d+)" % k, hdr).group(1)) == v, k
    sys_path_tools = os.path.join(ROOT, "tools", "kernel_table.py")
    assert '"n3d_cc_workspace_bytes"' in open(sys_path_tools).read().split("HOST_ONLY = {")[1].split("}")[0]
    # the host-side query runs without a device: 17 bytes per voxel and the record
    off = (_lib.C.c_int64 * 6)()
    n = 240 * 240 * 155
    total = lib.n3d_cc_workspace_bytes(240, 240, 155, off)
    assert off[0] == 0 and off[1] >= 4 * n and off[2] >= off[1] + 4 * n and off[3] >= off[2] + 4 * n and off[4] >= off[3] + 4 * n
    assert off[5] >= off[4] + n and off[5] % 8 == 0 and off[5] + 8 * P.REC_WORDS <= total < 17 * n + 4096
    assert lib.n3d_cc_workspace_bytes(0, 4, 4, None) == 0 and lib.n3d_cc_workspace_bytes(2048, 1024, 1024, None) == 0
    # the entry points refuse a bad connectivity and null pointers with a message, before anything is launched
    full = (_lib.C.c_int32 * 3)(4, 4, 4)
    assert lib.n3d_cc_label(None, full, 26, None, None, None) != 0 and b"cc_label" in lib.n3d_last_error()
    assert lib.n3d_cc_clean(None, full, 26, 0, 0, 0, None, None, None) != 0 and b"cc_clean" in lib.n3d_last_error()
    assert lib.n3d_cc_label(None, full, 7, None, None, None) != 0 and b"connectivity 7" in lib.n3d_last_error()
    assert lib.n3d_cc_clean(None, full, 0, 0, 0, 0, None, None, None) != 0 and b"connectivity 0" in lib.n3d_last_error()


def test_arguments_are_validated_without_a_device():
    import torch
    from nas_3d_unet_amd import postprocess as P
    from nas_3d_unet_amd._lib import N3DError
    host = torch.zeros((4, 4, 4), dtype=torch.uint8)
    # a host tensor (or no tensor): there is no CPU fallback
    for call in (lambda: P.label_components(host), lambda: P.label_components(host.bool()), lambda: P.clean_labels(host),
                 lambda: P.clean_labels(np.zeros((4, 4, 4), np.uint8)), lambda: P.clean_labels(host, return_stats=True)):
        with pytest.raises(N3DError, match="HIP device.*no CPU fallback"):
            call()
    # dtype and rank (the message names what came)
    with pytest.raises(N3DError, match="uint8 or bool"):
        P.label_components(host.to(torch.int32))
    with pytest.raises(N3DError, match=r"\(X, Y, Z\) uint8 volume"):
        P.clean_labels(host.bool())
    with pytest.raises(N3DError, match=r"\(X, Y, Z\)"):
        P.clean_labels(host[0])
    with pytest.raises(N3DError, match=r"\(X, Y, Z\)"):
        P.label_components(host[None])
    # more voxels than int32 ids (a view of one byte: nothing that large is allocated)
    huge = torch.zeros(1, dtype=torch.uint8).expand(2048, 1024, 1024)
    with pytest.raises(N3DError, match=r"X \* Y \* Z < 2\^31"):
        P.clean_labels(huge)
    with pytest.raises(N3DError, match=r"X \* Y \* Z < 2\^31"):
        P.label_components(huge)
    # connectivity and thresholds, checked before the volume
    for c in (0, 4, 8, 27, 26.0, "26", None, True):
        with pytest.raises(N3DError, match="connectivity must be 6, 18 or 26"):
            P.label_components(host, connectivity=c)
        with pytest.raises(N3DError, match="connectivity must be 6, 18 or 26"):
            P.clean_labels(host, connectivity=c)
        with pytest.raises(N3DError, match="connectivity must be 6, 18 or 26"):
            P.CleanedPredictor(_Stub(), connectivity=c)
    for kw in ({"min_voxels": -1}, {"et_min_voxels": -5}, {"min_voxels": 2.5}, {"et_min_voxels": None}):
        with pytest.raises(N3DError, match="%s must be an integer >= 0" % list(kw)[0]):
            P.clean_labels(host, **kw)
        with pytest.raises(N3DError, match="%s must be an integer >= 0" % list(kw)[0]):
            P.CleanedPredictor(_Stub(), **kw)


class _Stub:
    def predict(self, volumes, index, **kw):
        raise AssertionError("not called")


def test_cleaned_predictor_arguments():
    import torch
    from nas_3d_unet_amd import postprocess as P
    from nas_3d_unet_amd._lib import N3DError
    with pytest.raises(N3DError, match="predict"):
        P.CleanedPredictor(object())
    with pytest.raises(N3DError, match="unknown rule min_voxel "):
        P.CleanedPredictor(_Stub(), min_voxel=3)
    with pytest.raises(N3DError, match="unknown rules"):
        P.CleanedPredictor(_Stub(), return_stats=True, threshold=0.5)
    cp = P.CleanedPredictor(_Stub(), min_voxels=np.int64(7), keep_largest=1)
    assert cp.rules == {"connectivity": 26, "min_voxels": 7, "keep_largest": True, "et_min_voxels": 0} and cp.last_stats is None
    with pytest.raises(N3DError, match="no subject"):
        cp.stats()

    class Host:
        def predict(self, volumes, index, **kw):
            return torch.zeros((4, 4, 4), dtype=torch.uint8), "rest"

    with pytest.raises(N3DError, match="HIP device.*no CPU fallback"):
        P.CleanedPredictor(Host()).predict(None, 0)

    class Bare:
        def predict(self, volumes, index, **kw):
            return None

    with pytest.raises(N3DError, match="sequence that starts with the labels"):
        P.CleanedPredictor(Bare()).predict(None, 0)
