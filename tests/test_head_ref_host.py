"""CPU: the references, operands and buffer builders of tests/_head_ref.py, which tests/test_gpu_head_operands.py relies on."""
import numpy as np
import pytest
import torch

import _head_ref as hr
import _loss_ref as lr
from oracle import ref_path as orc


def test_dice_closed_form_equals_the_oracle_under_autograd():
    """Spec(0.5, 0.5, 1, 0) with half the smooth is the reference's Dice loss: value and d loss / d logits in fp64"""
    c = hr.DLOSS_CASE
    z, _ = hr.logits(c, True)
    t = hr.draw(c)["t"].double()
    zz = z.clone().requires_grad_(True)
    loss = orc.dice_loss(torch.sigmoid(zz), t, hr.DICE_SMOOTH)
    loss.backward()
    r = hr.reference(c, hr.DICE)
    assert abs(float(loss.detach()) - float(r.c.loss)) <= 1e-14
    assert float((zz.grad - r.c.dz).abs().max()) <= 1e-14 * max(1.0, float(zz.grad.abs().max()))
    # and the closed form with a cross-entropy term against the literal formula, on these operands
    zz = z.clone().requires_grad_(True)
    l2 = lr.torch_loss(zz, t, hr.BCE)
    l2.backward()
    r2 = hr.reference(c, hr.BCE)
    assert abs(float(l2.detach()) - float(r2.c.loss)) <= 1e-13
    assert float((zz.grad - r2.c.dz).abs().max()) <= 1e-13 * max(1.0, float(zz.grad.abs().max()))


@pytest.mark.parametrize("c", sorted(set(hr.all_cases())), ids=lambda c: "ci%d-co%d-B%d-%s" % (c.ci, c.co, c.B, "x".join(map(str, c.shape))))
def test_every_logit_is_an_fp32_number(c):
    d = hr.draw(c)
    assert set(np.unique(d["gate"].numpy())) <= {0.0, 2.0} and set(np.unique(d["t"].numpy())) <= {0.0, 1.0}
    assert torch.equal(d["x"], d["x"].round()) and float(d["x"].abs().max()) <= 4
    assert torch.equal(d["x"].bfloat16().float(), d["x"])
    assert torch.equal(d["w"] * 32, (d["w"] * 32).round()) and torch.equal(d["bias"] * 8, (d["bias"] * 8).round())
    for gated in (True, False):
        z, _ = hr.logits(c, gated)
        assert torch.equal(z.float().double(), z)
        assert torch.equal(z * 32, (z * 32).round()) and float(z.abs().max()) < 128     # 0, or 1/32 and more away from it
        # any partial sum is a multiple of 1/32 below the worst-case absolute sum, itself far below 2^24 / 32
        worst = float((d["w"].double().abs().reshape(c.co, c.ci).sum(1) * 4 * 2 + d["bias"].double().abs()).max())
        assert worst * 32 < 2 ** 24


def test_hard_sums_are_integers_and_one_pair_is_empty():
    c = hr.DLOSS_CASE
    z, _ = hr.logits(c, False)
    t = hr.draw(c)["t"]
    I, P = hr.hard_sums(z, t)
    assert torch.equal(I, I.round()) and torch.equal(P, P.round()) and bool((I <= P).all())
    assert float(t[0, c.co - 1].sum()) == 0.0
    p = torch.sigmoid(z)
    assert torch.equal((p >= 0.5), (z >= 0))


@pytest.mark.parametrize("wk", hr.WALKS, ids=lambda wk: "%s-B%d-co%d" % ("x".join(map(str, wk.shape)), wk.B, wk.co))
def test_walk_rows_reach_what_they_claim(wk):
    N = int(np.prod(wk.shape))
    assert hr.walk_reach(N, wk.B, wk.co) == (wk.rows, wk.per, wk.BC, wk.M)
    flat = wk.rows % 256 == 0 and wk.BC <= 64
    assert flat == (wk.per is not None) == wk.what.startswith("flat")


def test_walk_table_covers_the_named_conditions():
    flat = [wk for wk in hr.WALKS if wk.per is not None]
    assert {wk.per for wk in flat} >= {1, 2, 3}
    assert any(wk.M > 8 and wk.per == 1 for wk in flat) and any(wk.M > 8 and wk.per == 2 for wk in flat)
    assert any(wk.per == 3 and 8 % wk.per != 0 and wk.M > 8 for wk in flat)          # a pair's records straddle two rounds of 8
    assert any(wk.BC == 64 for wk in flat)
    wave = [wk for wk in hr.WALKS if wk.per is None]
    assert any(wk.BC == 68 and wk.rows == 256 for wk in wave)
    assert any(64 < wk.rows < 256 and wk.rows > 65 for wk in wave) and any(wk.rows == 65 for wk in wave)
    assert all(wk.BC <= 256 for wk in hr.WALKS)                                        # the evaluation forms' limit


def test_placement_tables():
    assert {c.ci for c in hr.PLACE_CASES} == {4, 8, 12, 16, 24, 32} and {c.co for c in hr.PLACE_CASES} == {1, 2, 3, 4}
    ns = {int(np.prod(c.shape)) for c in hr.PLACE_CASES}
    assert ns == {1200, 1024}
    assert hr.X_SLICE["extra"] != hr.DX_SLICE["extra"] and hr.X_LAST["off"] == hr.X_LAST["extra"]
    for pl in (hr.X_SLICE, hr.X_LAST, hr.DX_SLICE):
        assert pl["off"] % 4 == 0 and pl["extra"] % 4 == 0 and pl["off"] <= pl["extra"]
    assert set(hr.STORAGE) == {(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")}


def test_slice_builders_alias_their_buffer_and_sentinels_sit_where_claimed():
    a = torch.arange(2 * 4 * 2 * 3 * 5, dtype=torch.float32).reshape(2, 4, 2, 3, 5) % 7
    for pl in (hr.X_SLICE, hr.X_LAST, hr.DX_SLICE):
        buf, v = hr.place_ndhwc(a, pl["off"], pl["extra"])
        assert buf.shape == (2, 2, 3, 5, 4 + pl["extra"]) and buf.is_contiguous()
        assert v.shape == a.shape and torch.equal(v, a)
        assert v.data_ptr() == buf.data_ptr() + 4 * pl["off"] and v.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        assert v.stride() == (2 * 3 * 5 * buf.shape[-1], 1, 3 * 5 * buf.shape[-1], 5 * buf.shape[-1], buf.shape[-1])
        assert hr.outside_unchanged(buf, pl["off"], 4, hr.SENT_IN)
        assert int((buf == hr.SENT_IN).sum()) == 2 * 30 * pl["extra"]
        v[1, 2, 1, 1, 1] = 99.0          # a write through the view lands in the buffer, inside the slice
        assert float(buf[1, 1, 1, 1, pl["off"] + 2]) == 99.0 and hr.outside_unchanged(buf, pl["off"], 4, hr.SENT_IN)
        buf[0, 0, 0, 0, (pl["off"] + 4) % buf.shape[-1]] = 1.0      # a write next to the slice is seen
        assert not hr.outside_unchanged(buf, pl["off"], 4, hr.SENT_IN)
    # the last slice ends where its allocation ends
    buf, v = hr.place_ndhwc(a, hr.X_LAST["off"], hr.X_LAST["extra"])
    assert v.storage_offset() + (2 * 30 - 1) * buf.shape[-1] + 4 == buf.numel()
    # an output buffer: the slice holds the prefill until it is written
    out = hr.ndhwc_buffer(2, (2, 3, 5), 4 + hr.DX_SLICE["extra"], hr.SENT_OUT)
    ov = hr.channel_slice(out, hr.DX_SLICE["off"], 4)
    assert not hr.no_prefill_left(ov)
    ov.copy_(a)
    assert hr.no_prefill_left(ov) and hr.outside_unchanged(out, hr.DX_SLICE["off"], 4, hr.SENT_OUT)
    # NCDHW channel slices and the byte offset
    buf, v = hr.place_ncdhw(a, 1, 2)
    assert v.data_ptr() == buf.data_ptr() + 4 * 30 and torch.equal(v, a) and float(buf[:, 0].min()) == hr.SENT_IN == float(buf[:, 5].max())
    b8 = (a % 2).to(torch.uint8)
    buf, v = hr.place_bytes_offset(b8)
    assert v.data_ptr() == buf.data_ptr() + 1 and torch.equal(v, b8) and v.is_contiguous() and int(buf[0]) == 255
    for dt in (torch.float32, torch.bfloat16):
        assert float(torch.tensor(hr.SENT_IN, dtype=dt)) == hr.SENT_IN and float(torch.tensor(hr.SENT_OUT, dtype=dt)) == hr.SENT_OUT


def test_eval_accumulator_and_dloss_scaling():
    I = np.array([[2.0, 0.0], [1.0, 0.0]])
    P = np.array([[4.0, 0.0], [1.0, 3.0]])
    T = np.array([[2.0, 0.0], [3.0, 0.0]])
    acc = hr.eval_accumulator([(0.25, I, P, T), (0.5, I, P, T)], 2)
    assert acc[:4].tolist() == [0.75, 2.0, 4.0, 0.0]
    assert acc[4:8].tolist() == [6.0, 10.0, 10.0, 2 * (4.0 / 6.0 + 2.0 / 4.0)]
    assert acc[8:12].tolist() == [0.0, 6.0, 0.0, 2 * (1.0 + 0.0)]
    g = (torch.ones(2), torch.full((2,), 3.0))
    assert [v.tolist() for v in hr.scaled(g, -4.0)] == [[-4.0, -4.0], [-12.0, -12.0]] and hr.scaled(g, None)[1].tolist() == [3.0, 3.0]
