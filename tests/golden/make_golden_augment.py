#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by running the REFERENCE's own scale / flip augmentation (augment.py:8-73) and its Generator
class with augment=True (generator.py:68-248).

Runs only in the build container (needs /root/reference and scipy).  do_augment, augment_data, distort_image, flip_image,
scale_image, get_image, random_scale_factor, random_flip_dimensions, random_boolean and the permutation functions (augment.py),
the Generator class (generator.py) and the patching functions (patches.py) are taken out of the parsed reference sources (ast) and
executed as they are, as make_golden_generator.py does.  nibabel and nilearn are not installed; the three names augment.py takes
from them are stand-ins:

  * nib.Nifti1Image(dataobj, affine) -> an object that holds dataobj, affine, shape and get_data();
  * new_img_like(ref, data, affine)  -> such an object with the given affine, or a copy of ref's;
  * resample_to_img(source, target, interpolation="nearest")
                                     -> nilearn's resample_img for this call, restated: if np.allclose(target affine, source
                                        affine) the source is returned as it is; else T = inv(source affine) . target affine, whose
                                        3x3 part must be diagonal, and the data is
                                        scipy.ndimage.affine_transform(data, diag(T[:3,:3]), offset=T[:3,3],
                                                                       output_shape=target.shape, order=0, mode="constant", cval=0).

nilearn itself is never run: what the fixture pins is scipy's resampling rule as nilearn calls it.  The draws are the reference's
own (np.random.normal, np.random.choice through random_scale_factor / random_boolean); for the operator cases that need a particular
scale, the `np` the reference functions see has a `random` that plays back the listed draws instead.

The fixture holds
  (a) operator cases: per case the drawn scale and flipped axes, A, b (what affine_transform was given; A = 1, b = 0 and
      identity = 1 on the early-return path) and do_augment's outputs for the inputs operator_inputs() regenerates;
  (b) adversarial coordinates: one-axis cases (P, A, b) for which scipy's coordinate (j + b / A) * A and the textbook A * j + b
      give a different voxel or a different inside / outside answer, with scipy's source index per output index (-1: outside);
  (c) generator cases: per run the (epoch, batch, volume, corner, key, flips) rows, the drawn scales, and the arrays of the first
      batch.
Nothing of the reference's source is stored.  Usage:  python tests/golden/make_golden_augment.py
"""
import itertools
import json
import os
import sys

import numpy as np

import make_golden_generator as mg

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

IDENTITY_AFFINE = np.eye(4)
BRATS_AFFINE = np.array([[-1.0, 0, 0, 0], [0, -1.0, 0, 239.0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
AFFINES = {"identity": IDENTITY_AFFINE, "brats": BRATS_AFFINE}


def operator_inputs(P):
    """(data (2, P, P, P) float32, truth (1, P, P, P) uint8): channel 0 numbers the voxels 1..P^3 (an output names its source),
    channel 1 is a small signed integer pattern; labels {0, 1, 2, 4} in shells around an off-centre point"""
    g = np.meshgrid(*[np.arange(P)] * 3, indexing="ij")
    ident = (g[0] * P + g[1]) * P + g[2] + 1
    data = np.stack([ident, (g[0] + 2 * g[1] + 3 * g[2]) % 5 - 2]).astype(np.float32)
    d = np.sqrt((g[0] - 0.35 * P) ** 2 + (g[1] - 0.55 * P) ** 2 + (g[2] - 0.6 * P) ** 2)
    truth = np.select([d <= 0.15 * P, d <= 0.3 * P, d <= 0.45 * P], [4, 1, 2], 0).astype(np.uint8)[None]
    return data, truth


def operator_cases():
    """(name, P, affine, scale_deviation, flip, draws): draws = None: np.random seeded with `seed`; else (scale or None, [bool] * 3)
    played back"""
    T, F = True, False
    return [
        ("seeded_both_p8", 8, "brats", 0.25, True, 501),
        ("seeded_both_p10", 10, "identity", 0.25, True, 502),
        ("seeded_scale_only_p10", 10, "brats", 0.25, False, 503),
        ("seeded_flip_only_p8", 8, "identity", None, True, 504),
        ("zoom_in_p8", 8, "identity", 0.25, False, ([0.7, 0.55, 0.8], None)),
        ("zoom_out_p10", 10, "brats", 0.25, True, ([1.3, 1.6, 1.15], [T, F, T])),
        ("negative_p8", 8, "brats", 0.25, True, ([-0.9, 1.1, -0.6], [F, F, T])),
        ("allclose_p8", 8, "brats", 0.25, True, ([1 + 2e-9, 1 - 1e-9, 1 + 1e-9], [T, T, F])),
        ("near_one_p10", 10, "identity", 0.25, False, ([1 + 1e-6, 1 - 1e-6, 1 + 5e-7], None)),   # within 1e-6 of 1, NOT allclose
        ("half_voxel_p8", 8, "identity", 0.25, True, ([0.5, 2.0, 0.25], [T, F, F])),             # exact half-integer coordinates
    ]


class _Playback:
    """np.random stand-in for the forced operator cases: normal() returns the listed scale, choice() the listed booleans"""

    def __init__(self, scale, flips):
        self.scale, self.flips = scale, list(flips or [])

    def normal(self, mean, std, n):
        assert (mean, n) == (1, 3)
        return np.array(self.scale, np.float64)

    def choice(self, options):
        assert list(options) == [True, False]
        return np.bool_(self.flips.pop(0))


class _NumpyWith:
    """numpy with some attributes replaced (random: a playback; load: the affine file)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        return getattr(np, name)


class _Image:
    """nibabel.Nifti1Image stand-in"""

    def __init__(self, dataobj, affine):
        self.dataobj, self.affine, self.shape = dataobj, affine, dataobj.shape

    def get_data(self):
        return self.dataobj


def _new_img_like(ref, data, affine=None):
    return _Image(data, np.copy(ref.affine) if affine is None else affine)


def augment_namespace(np_like, log):
    """augment.py's functions over the stand-ins; log collects one record per resample_to_img call"""
    from scipy.ndimage import affine_transform

    def resample_to_img(source, target, interpolation="nearest"):
        assert interpolation == "nearest"
        M, N = target.affine, source.affine
        if np.allclose(M, N):
            log.append((np.ones(3), np.zeros(3), True))
            return source
        T = np.linalg.inv(N).dot(M)
        assert np.all(np.diag(np.diag(T[:3, :3])) == T[:3, :3]), T
        A, b = np.diag(T[:3, :3]), T[:3, 3]
        log.append((A.copy(), b.copy(), False))
        data = affine_transform(source.get_data(), A, offset=b, output_shape=target.shape, order=0, mode="constant", cval=0)
        return _Image(data, M)

    import random
    ns = {"np": np_like, "nib": type("nib", (), {"Nifti1Image": _Image}), "new_img_like": _new_img_like,
          "resample_to_img": resample_to_img, "random": random, "itertools": itertools}
    mg._reference_defs(os.path.join(REF, "augment.py"),
                       ["scale_image", "flip_image", "random_flip_dimensions", "random_scale_factor", "random_boolean", "distort_image",
                        "do_augment", "augment_data", "get_image", "generate_permutation_keys", "random_permutation_key", "permute_data",
                        "random_permutation_x_y"], ns)
    drawn = []
    scale_fn, flip_fn = ns["random_scale_factor"], ns["random_flip_dimensions"]

    def recording_scale(*a, **k):
        s = scale_fn(*a, **k)
        drawn.append(("scale", s))
        return s

    def recording_flips(*a, **k):
        f = flip_fn(*a, **k)
        drawn.append(("flips", f))
        return f
    ns["random_scale_factor"], ns["random_flip_dimensions"] = recording_scale, recording_flips
    return ns, drawn


def _draw_record(drawn):
    scale = [s for k, s in drawn if k == "scale"]
    flips = [f for k, f in drawn if k == "flips"]
    s = np.asarray(scale[-1], np.float64) if scale else np.full(3, np.nan)
    f = np.array([int(a in flips[-1]) for a in range(3)] if flips else [0, 0, 0], np.int8)
    return s, f


def run_operator_case(case):
    name, P, aff, dev, flip, draws = case
    log = []
    if isinstance(draws, int):
        np.random.seed(draws)
        ns, drawn = augment_namespace(np, log)
    else:
        ns, drawn = augment_namespace(_NumpyWith(random=_Playback(*draws)), log)
    data, truth = operator_inputs(P)
    x, y = ns["do_augment"](data.copy(), truth.copy(), AFFINES[aff].copy(), scale_deviation=dev, flip=flip)
    assert len(log) == data.shape[0] + 1 and all(np.array_equal(l[0], log[0][0]) and np.array_equal(l[1], log[0][1]) for l in log)
    scale, flips = _draw_record(drawn)
    assert x.dtype == np.float32 and y.dtype == np.uint8 and np.array_equal(x, np.round(x))
    return {"scale": scale, "flips": flips, "A": log[0][0], "b": log[0][1], "identity": np.int8(log[0][2]),
            "x": x.astype(np.int16), "y": y}


def find_adversarial(n_want=8, seed=77):
    """one-axis (P, A, b) for which floor((j + b / A) * A + 0.5) / its bounds test and floor(A * j + b + 0.5) / its bounds test
    disagree at some j; scipy's own answer (affine_transform on the line 1..P) is what is kept"""
    from scipy.ndimage import affine_transform
    rng = np.random.default_rng(seed)
    found, kinds = [], {"voxel": 0, "bound": 0}
    tries = 0
    while len(found) < n_want:
        tries += 1
        P = int(rng.choice([8, 10]))
        A = float(rng.choice([-1, 1]) * rng.uniform(0.4, 1.9))
        j0 = int(rng.integers(0, P))
        want_bound = kinds["bound"] < n_want // 2 and tries % 2 == 0
        target = float(rng.choice([0.0, P - 1.0])) if want_bound else float(rng.integers(0, P - 1)) + 0.5
        b = target - A * j0                       # A * j0 + b lands on (or an ulp off) a rounding or bounds threshold
        j = np.arange(P, dtype=np.float64)
        naive_c = A * j + b
        naive = np.where((naive_c >= 0) & (naive_c <= P - 1), np.floor(naive_c + 0.5), -1).astype(np.int64)
        line = np.arange(1, P + 1, dtype=np.float64)
        got = affine_transform(line, np.array([A]), offset=np.array([b]), output_shape=(P,), order=0, mode="constant", cval=0)
        src = got.astype(np.int64) - 1
        if np.array_equal(src, naive):
            continue
        kind = "bound" if ((src < 0) != (naive < 0)).any() else "voxel"
        if kinds[kind] >= n_want - 2:
            continue
        kinds[kind] += 1
        found.append((P, int(rng.integers(0, 3)), A, b, src))
    assert kinds["voxel"] >= 2 and kinds["bound"] >= 2, kinds
    return found, tries


def generator_cases():
    """(name, python seed, numpy seed, affine, Generator kwargs, epochs)"""
    return [
        ("permute_hanging_b2", 35, 131, "brats", dict(indices_list=[3, 0], patch_shape=8, patch_overlap=3, batch_size=2, permute=True,
                                                      augment=True), 2),
        ("noflip_incl_b2", 32, 132, "identity", dict(indices_list=[1, 0], patch_shape=8, patch_overlap=None, batch_size=2,
                                                     augment=True, augment_flip=False, inclusive_label=True), 1),
        ("noscale_b2", 33, 133, "brats", dict(indices_list=[1, 3], patch_shape=8, patch_overlap=2, batch_size=2, augment=True,
                                              augment_distortion_factor=None, both_ps=True), 1),
    ]


def run_generator_case(case, volumes, spe_path):
    """make_golden_generator.run_reference with augment=True: the same replacements of file access, plus np.load(affine_file) ->
    the affine and do_augment -> the reference's own over the stand-ins above"""
    import pickle
    import random
    from random import shuffle
    name, seed, np_seed, aff, kw, epochs = case
    pat = mg._reference_defs(os.path.join(REF, "patches.py"), ["_patching_autofit", "get_set_of_patch_indices", "patching",
                                                               "get_patch_from_3d_data", "fix_out_of_bound_patch_attempt"],
                             {"np": mg._NumpyWithOldAliases()})
    log = []
    aug, drawn = augment_namespace(np, log)
    keys = []
    draw_key = aug["random_permutation_key"]

    def recording_key():
        k = draw_key()
        keys.append(k)
        return k
    aug["random_permutation_key"] = recording_key
    overlaps, reads = [], []

    def create_id_index_patch_list(id_index_list, data_file, patch_shape, patch_overlap=None, both_ps=False, trivial=True):
        overlaps.append(patch_overlap)
        out = []
        for index in id_index_list:
            box = np.asarray(data_file[index][0].shape[1:])
            out.extend(itertools.product([index], pat["patching"](box, patch_shape, overlap=patch_overlap, both_ps=both_ps)))
        return out

    def get_data_from_file(data_file, id_index_patch, patch_shape):
        id_index, corner = id_index_patch
        reads.append((id_index, tuple(int(c) for c in corner)))
        vol, truth = data_file[id_index]
        return pat["get_patch_from_3d_data"](vol, patch_shape, corner), pat["get_patch_from_3d_data"](truth, patch_shape, corner)

    ns = {"DEBUG_FLAG": False, "random": random, "shuffle": shuffle, "os": os, "pickle": pickle,
          "np": _NumpyWith(load=lambda path: AFFINES[path].copy()),
          "create_id_index_patch_list": create_id_index_patch_list, "get_data_from_file": get_data_from_file,
          "get_patch_from_3d_data": pat["get_patch_from_3d_data"], "tqdm": lambda it, **k: it,
          "random_permutation_x_y": aug["random_permutation_x_y"], "do_augment": aug["do_augment"]}
    mg._reference_defs(os.path.join(REF, "generator.py"), ["Generator"], ns)

    class Observed(ns["Generator"]):
        def add_data(self, x_list, y_list, id_index_patch, _augment=True, _permute=True):
            n, nk, nd = len(x_list), len(keys), len(drawn)
            super().add_data(x_list, y_list, id_index_patch, _augment, _permute)
            if len(x_list) > n and _permute:
                scale, flips = _draw_record(drawn[nd:])
                self.pending.append(reads[-1] + (keys[-1] if len(keys) > nk else None, scale, flips))

        def convert_data(self, x_list, y_list):
            self.batches.append(self.pending)
            self.pending = []
            return super().convert_data(x_list, y_list)

    random.seed(seed)
    np.random.seed(np_seed)
    Observed.pending, Observed.batches = [], []
    g = Observed(data_file=list(volumes), spe_file=spe_path, labels=[1, 2, 4], affine_file=aff, **kw)
    rec = {"overlap": [], "spe": [], "rows": [], "scales": [], "first": None}
    for e in range(epochs):
        rec["overlap"].append(overlaps[-1])
        rec["spe"].append(g.steps_per_epoch)
        g.batches = []
        for x, y in g.epoch():
            if rec["first"] is None:
                rec["first"] = (x, y)
        rows, scales = [], []
        for b, batch in enumerate(g.batches):
            for v, corner, key, scale, flips in batch:
                k = [-1] * 6 if key is None else [key[0][0], key[0][1], key[1], key[2], key[3], key[4]]
                rows.append([b, v, *corner, *k, *[int(f) for f in flips]])
                scales.append(scale)
        rec["rows"].append(np.asarray(rows, np.int32).reshape(-1, 14))
        rec["scales"].append(np.asarray(scales, np.float64).reshape(-1, 3))
    rec["overlap"].append(overlaps[-1])
    return rec


def main():
    import tempfile
    out, config = {}, {"ops": [], "gens": []}
    seen = {"scale_only": 0, "flip_only": 0, "both": 0, "zoom_in": 0, "zoom_out": 0, "negative": 0, "allclose": 0}
    table, xs, ys = [], [], []
    for case in operator_cases():
        r = run_operator_case(case)
        config["ops"].append({"name": case[0], "P": case[1], "affine": case[2]})
        table.append(np.concatenate((r["scale"], r["flips"], r["A"], r["b"], [r["identity"]])))
        xs.append(r["x"].reshape(-1))
        ys.append(r["y"].reshape(-1))
        s, f = r["scale"], r["flips"]
        has_s, has_f = not np.isnan(s).any(), bool(f.any())
        seen["scale_only"] += has_s and not has_f
        seen["flip_only"] += has_f and not has_s
        seen["both"] += has_s and has_f
        if has_s:
            seen["zoom_in"] += bool(((s > 0) & (s < 1 - 1e-3)).any())
            seen["zoom_out"] += bool((s > 1 + 1e-3).any())
            seen["negative"] += bool((s < 0).any())
            seen["allclose"] += bool(r["identity"]) and bool((np.abs(s - 1) < 1e-6).all())
        print("%-22s scale %s flips %s A %s b %s identity %d  zero voxels %d" % (case[0], s, f, r["A"], r["b"], r["identity"],
                                                                                int((r["x"][0] == 0).sum())))
    assert all(v >= 1 for v in seen.values()), seen
    # one row per operator case: scale (NaN: none drawn), flips, A, b, identity; the outputs of all cases end to end
    out["op/table"] = np.asarray(table, np.float64)
    out["op/x"] = np.concatenate(xs).astype(np.int16)
    out["op/y"] = np.concatenate(ys).astype(np.uint8)
    adv, tries = find_adversarial()
    out["adv/table"] = np.array([[P, axis, A, b] for P, axis, A, b, _ in adv], np.float64)
    out["adv/src"] = np.array([np.concatenate((src, np.full(10 - len(src), -2))) for *_, src in adv], np.int8)
    for i, (P, axis, A, b, src) in enumerate(adv):
        print("adversarial %d: P %d axis %d A %r b %r -> %s" % (i, P, axis, A, b, src.tolist()))
    print("(%d candidates tried)" % tries)
    volumes = mg.generator_volumes()
    for ci, case in enumerate(generator_cases()):
        name, seed, np_seed, aff, kw, epochs = case
        with tempfile.TemporaryDirectory() as tmp:
            rec = run_generator_case(case, volumes, os.path.join(tmp, "spe.pkl"))
        k = "gen%d" % ci
        config["gens"].append({"name": name, "seed": seed, "np_seed": np_seed, "affine": aff, "epochs": epochs, "kwargs": kw,
                               "overlap": rec["overlap"], "spe": rec["spe"]})
        # rows: (epoch, batch, volume, corner x y z, six key entries or -1, flips x y z); scales: the drawn scale of each row (NaN: none)
        out[k + "/rows"] = np.concatenate([np.concatenate((np.full((len(r), 1), e, np.int32), r), axis=1) for e, r in enumerate(rec["rows"])])
        out[k + "/scales"] = np.concatenate(rec["scales"])
        x, y = rec["first"]
        x8 = x.astype(np.float64) * 8
        assert np.array_equal(x8, np.round(x8)) and np.abs(x8).max() < 2 ** 15
        out[k + "/x8"] = x8.astype(np.int16)          # the first batch; the volumes hold multiples of 1/8
        out[k + "/y"] = y.astype(np.int8)
        rows = rec["rows"][0]
        P = kw["patch_shape"]
        hang = sum(int((r[2:5] < 0).any() or any(r[2 + a] + P > volumes[r[1]][0].shape[1 + a] for a in range(3))) for r in rows)
        print("%-20s overlaps %s spe %s kept/epoch %s hanging %d" % (name, rec["overlap"], rec["spe"], [len(r) for r in rec["rows"]], hang))
        if kw.get("permute"):
            assert hang >= 1
    out["config"] = np.array(json.dumps(config))
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d arrays, %.1f KB)" % (path, len(out), os.path.getsize(path) / 1024))
    import zipfile
    print("  ".join("%s %d" % (i.filename[:-4], i.compress_size) for i in zipfile.ZipFile(path).infolist()))


if __name__ == "__main__":
    sys.exit(main())
