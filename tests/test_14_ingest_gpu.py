"""Clip ingest on the device: vptr_clip_ingest through the C ABI and through ops.ingest_clips against the integer reference builder of
ingest_ref.py (pinned to PIL by test_ingest_cpu.py), the PIL-written fixture, ClipIngest / DeviceClipLoader end to end, one graph
capture, and the guards.

Every comparison is torch.equal: PIL's 8-bit resize is integer arithmetic and ToTensor + Normalize of a uint8 value is a table, so there
is no tolerance.  Outputs are NaN before each C-ABI call and sit inside a guard buffer whose other floats must stay bit-identical."""
import functools

import numpy as np
import pytest
import torch

from helpers import jload, load
from vptr_amd.data import ClipIngest, DeviceClipLoader, IngestPlan      # the module under test
from ingest_ref import GOLDEN_GEOMETRIES, KINDS, make_raw, normalise_u8, ref_ingest

pytestmark = pytest.mark.gpu

NAN = float("nan")
KTH = (0.6013795, 2.7570653)
BAIR = ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673))

# (Hin, Win, C, crop box or None, (Hout, Wout))
GEOMS = [
    (120, 160, 1, (0, 20, 120, 120), (64, 64)),      # KTH 64
    (120, 160, 1, (0, 20, 120, 120), (128, 128)),    # upscale, ksize 3
    (64, 64, 3, None, (64, 64)),                     # both passes skipped, HWC -> CHW
    (37, 53, 3, (3, 5, 31, 41), (16, 24)),           # odd offsets, ksize 5 / 5 from 31 x 41
    (9, 7, 1, None, (20, 13)),                       # odd Wout: scalar stores
    (5, 300, 1, None, (3, 64)),                      # ksize 11
    (240, 240, 1, None, (64, 64)),                   # ksize 9
    (20, 300, 1, None, (17, 256)),                   # maximum width, a band of one row
    (120, 64, 1, None, (64, 64)),                    # vertical pass only
    (64, 120, 1, None, (64, 64)),                    # horizontal pass only
    (130, 50, 3, (1, 2, 128, 47), (16, 250)),        # 8x down (ksize 17) beside a 5.3x up, RGB at nearly full width: the largest LDS need
]
IDS = ["%dx%dx%d-%dx%d" % (g[0], g[1], g[2], g[4][0], g[4][1]) for g in GEOMS]


def consts(C):
    return KTH if C == 1 else BAIR


@functools.lru_cache(maxsize=None)
def plan_for(gi):
    Hin, Win, C, crop, out_hw = GEOMS[gi]
    mean, std = consts(C)
    return IngestPlan((Hin, Win), C, out_hw, crop=crop, mean=mean, std=std, device="cuda:0")


@functools.lru_cache(maxsize=None)
def case(gi, kind, N=2, T=3, flips=None):
    """(raw uint8 numpy, reference fp32 [N, T, C, Hout, Wout]); built once per case and shared, never written to"""
    Hin, Win, C, crop, out_hw = GEOMS[gi]
    raw = make_raw((N, T, Hin, Win, C), kind, 6000 + 100 * gi + KINDS.index(kind))
    mean, std = consts(C)
    return raw, ref_ingest(raw, crop, out_hw, mean, std, flips=None if flips is None else list(flips))


def abi_ingest(raw_d, plan, flips_d=None, Tp=None, two=True, pad=64):
    """one direct C-ABI call; the outputs are NaN-filled views into a guard buffer [pad | out0 | pad | out1 | pad] whose other floats must
    not change.  Returns (out0, out1) (out1 None for a single output)."""
    from vptr_amd._lib import check, lib, ptr, stream
    N, T, Hin, Win, C = raw_d.shape
    Tp = T if Tp is None else Tp
    top, left, Hc, Wc = plan.crop
    Hout, Wout = plan.out_hw
    per = C * Hout * Wout
    n0, n1 = N * Tp * per, (N * (T - Tp) * per if two else 0)
    guard = torch.arange(n0 + n1 + 3 * pad, device=raw_d.device, dtype=torch.float32) * 0.37 + 1.0
    before = guard.clone()
    o0 = guard[pad:pad + n0].view(N, Tp, C, Hout, Wout)
    o1 = guard[2 * pad + n0:2 * pad + n0 + n1].view(N, T - Tp, C, Hout, Wout) if two else None
    o0.fill_(NAN)
    if two:
        o1.fill_(NAN)
    hp, vp = Wout != Wc, Hout != Hc
    check(lib.vptr_clip_ingest(ptr(raw_d), ptr(plan.kx) if hp else None, ptr(plan.bx) if hp else None, ptr(plan.ky) if vp else None,
                               ptr(plan.by) if vp else None, ptr(plan.lut), ptr(flips_d), ptr(o0) if Tp > 0 else None,
                               ptr(o1) if two and Tp < T else None, N, T, Tp, Hin, Win, C, top, left, Hc, Wc, Hout, Wout,
                               plan.ksx if hp else 0, plan.ksy if vp else 0, stream()), "vptr_clip_ingest")
    gi32, bi32 = guard.view(torch.int32), before.view(torch.int32)
    for lo, hi in ((0, pad), (pad + n0, 2 * pad + n0), (2 * pad + n0 + n1, 3 * pad + n0 + n1)):
        assert torch.equal(gi32[lo:hi], bi32[lo:hi]), "guard floats %d .. %d changed" % (lo, hi)
    return o0, o1


# ------------------------------------------------------------------------------------------------------ 1. geometries
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_geometry(dev, gi, kind):
    import vptr_amd.ops as ops
    raw, ref = case(gi, kind)
    plan, raw_d = plan_for(gi), torch.from_numpy(raw).to(dev)
    got, _ = abi_ingest(raw_d, plan, two=False)
    assert torch.equal(got.cpu(), ref), "abi %s %s: %d values differ" % (IDS[gi], kind, int((got.cpu() != ref).sum()))
    op = ops.ingest_clips(raw_d, plan)
    assert op.dtype == torch.float32 and tuple(op.shape) == tuple(ref.shape) and op.is_contiguous()
    assert torch.equal(op.cpu(), ref), "op %s %s: %d values differ" % (IDS[gi], kind, int((op.cpu() != ref).sum()))


def test_unaligned_outputs_take_scalar_stores(dev):
    """Wout % 4 == 0 but the output pointers are not 16-byte aligned (pad of 61 floats)"""
    raw, ref = case(0, "random")
    got, _ = abi_ingest(torch.from_numpy(raw).to(dev), plan_for(0), two=False, pad=61)
    assert got.data_ptr() % 16 != 0
    assert torch.equal(got.cpu(), ref)


# ------------------------------------------------------------------------------------------------------ 2. flips, splits
@pytest.mark.parametrize("gi", [0, 3, 4, 2], ids=[IDS[i] for i in (0, 3, 4, 2)])
def test_all_four_flips_in_one_batch(dev, gi):
    import vptr_amd.ops as ops
    flips = (0, 1, 2, 3)
    raw, ref = case(gi, "random", N=4, T=2, flips=flips)
    _, plain = case(gi, "random", N=4, T=2)
    assert not torch.equal(ref[1:], plain[1:]) and torch.equal(ref[3], plain[3].flip(-1).flip(-2))
    raw_d, fl = torch.from_numpy(raw).to(dev), torch.tensor(flips, dtype=torch.int32, device=dev)
    got, _ = abi_ingest(raw_d, plan_for(gi), fl, two=False)
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(ops.ingest_clips(raw_d, plan_for(gi), flips=fl).cpu(), ref)


@pytest.mark.parametrize("Tp", [2, 0, 5])
def test_splits(dev, Tp):
    import vptr_amd.ops as ops
    gi, T = 3, 5
    raw, ref = case(gi, "random", N=2, T=T, flips=(2, 1))
    raw_d, fl = torch.from_numpy(raw).to(dev), torch.tensor([2, 1], dtype=torch.int32, device=dev)
    o0, o1 = abi_ingest(raw_d, plan_for(gi), fl, Tp=Tp)
    assert torch.equal(o0.cpu(), ref[:, :Tp]) and torch.equal(o1.cpu(), ref[:, Tp:])
    for split in ((Tp, T - Tp), Tp):
        past, future = ops.ingest_clips(raw_d, plan_for(gi), flips=fl, split=split)
        assert tuple(past.shape) == (2, Tp) + tuple(ref.shape[2:]) and tuple(future.shape) == (2, T - Tp) + tuple(ref.shape[2:])
        assert past.is_contiguous() and future.is_contiguous()
        assert torch.equal(past.cpu(), ref[:, :Tp]) and torch.equal(future.cpu(), ref[:, Tp:])
    mine = (torch.full_like(past, NAN), torch.full_like(future, NAN))       # caller-owned outputs: the pair implies the split
    back = ops.ingest_clips(raw_d, plan_for(gi), flips=fl, out=mine)
    assert back[0] is mine[0] and back[1] is mine[1]
    assert torch.equal(mine[0].cpu(), ref[:, :Tp]) and torch.equal(mine[1].cpu(), ref[:, Tp:])


def test_single_output_into_callers_tensor(dev):
    import vptr_amd.ops as ops
    raw, ref = case(1, "ramp")
    out = torch.full(tuple(ref.shape), NAN, device=dev)
    assert ops.ingest_clips(torch.from_numpy(raw).to(dev), plan_for(1), out=out) is out
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------------ 3. PIL's own images
@pytest.mark.parametrize("tag", sorted(GOLDEN_GEOMETRIES))
def test_pil_fixture_through_lut(dev, tag):
    """tests/golden/ingest_pil.npz: what PIL made of the raw frames, pushed through ToTensor + Normalize, against the kernel on the raw"""
    import vptr_amd.ops as ops
    z = load("ingest_pil")
    meta = jload(z, "meta")[tag]
    Hin, Win, C, crop, out_hw = GOLDEN_GEOMETRIES[tag]
    mean, std = consts(C)
    want = normalise_u8(z["pil:" + tag], mean, std)
    plan = IngestPlan((Hin, Win), C, out_hw, crop=crop, mean=mean, std=std, device=dev)
    raw_d = torch.from_numpy(z["raw:" + meta["raw"]]).to(dev)
    got, _ = abi_ingest(raw_d, plan, two=False)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.ingest_clips(raw_d, plan).cpu(), want)
    assert float(plan.lut[0, int(z["pil:" + tag][0, 0, 0, 0, 0])]) == float(want[0, 0, 0, 0, 0])


def test_presets_on_device(dev):
    """IngestPlan.kth(64) / kth(128) / bair() / mnist() on batches of their own shape"""
    import vptr_amd.ops as ops
    for plan, gi, shape, crop, ms in ((IngestPlan.kth(64, device=dev), 0, (2, 3, 120, 160, 1), (0, 20, 120, 120), KTH),
                                      (IngestPlan.kth(128, device=dev), 1, (2, 3, 120, 160, 1), (0, 20, 120, 120), KTH),
                                      (IngestPlan.bair(device=dev), 2, (2, 3, 64, 64, 3), None, BAIR),
                                      (IngestPlan.mnist(device=dev), None, (2, 3, 64, 64, 1), None, (0.0, 1.0))):
        if gi is not None:
            raw, ref = case(gi, "random")
        else:
            raw = make_raw(shape, "random", 6900)
            ref = ref_ingest(raw, crop, (64, 64), *ms)
        assert torch.equal(ops.ingest_clips(torch.from_numpy(raw).to(dev), plan).cpu(), ref)


# ------------------------------------------------------------------------------------------------------ 4. determinism
def test_two_calls_bit_identical(dev):
    raw, ref = case(6, "random")
    raw_d = torch.from_numpy(raw).to(dev)
    a, _ = abi_ingest(raw_d, plan_for(6), two=False)
    b, _ = abi_ingest(raw_d, plan_for(6), two=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.cpu(), ref)


# ------------------------------------------------------------------------------------------------------ 5. end to end
def test_clip_ingest_from_pinned_host_batch(dev):
    plan = IngestPlan.kth(64, device=dev)
    ing = ClipIngest(plan, 2, 3, hflip_p=0.5, vflip_p=0.5, seed=3)
    raw = make_raw((6, 5, 120, 160, 1), "random", 6950)
    seen = set()
    for batch in (torch.from_numpy(raw).pin_memory(), raw, torch.from_numpy(raw).to(dev)):      # pinned tensor, numpy, device tensor
        past, future = ing(batch)
        seen.update(ing.last_flips.tolist())
        ref = ref_ingest(raw, (0, 20, 120, 120), (64, 64), *KTH, flips=ing.last_flips)
        assert past.is_cuda and tuple(past.shape) == (6, 2, 1, 64, 64) and tuple(future.shape) == (6, 3, 1, 64, 64)
        assert torch.equal(past.cpu(), ref[:, :2]) and torch.equal(future.cpu(), ref[:, 2:])
    assert len(seen) > 1                                                                          # 18 draws at p = 0.5
    past, future = ing(raw, flips=[3, 0, 1, 2, 3, 0])
    ref = ref_ingest(raw, (0, 20, 120, 120), (64, 64), *KTH, flips=[3, 0, 1, 2, 3, 0])
    assert torch.equal(past.cpu(), ref[:, :2]) and torch.equal(future.cpu(), ref[:, 2:])
    test = ClipIngest(plan, 2, 3)                                                                 # the test transform: no flips
    past, future = test(raw)
    assert torch.equal(torch.cat([past, future], dim=1).cpu(), ref_ingest(raw, (0, 20, 120, 120), (64, 64), *KTH))


def test_device_clip_loader_feeds_evaluate_rollout(dev):
    """a loader of uint8 clips whose future frames repeat the past ones, scored with the identity predictor: every frame is predicted
    exactly, so PSNR sits at frame_metrics' cap (-10 log10(1e-8) = 80 dB), SSIM at 1 and the squared error at 0"""
    from vptr_amd.evaluate import evaluate_rollout
    plan = IngestPlan.kth(64, device=dev)
    batches = []
    for i, n in enumerate((2, 1)):
        half = make_raw((n, 3, 120, 160, 1), "random", 6960 + i)
        batches.append(np.concatenate([half, half], axis=1))
    loader = DeviceClipLoader(batches, ClipIngest(plan, 3, 3))
    assert len(loader) == 2
    for (past, future), raw in zip(loader, batches):
        ref = ref_ingest(raw, (0, 20, 120, 120), (64, 64), *KTH)
        assert torch.equal(past.cpu(), ref[:, :3]) and torch.equal(future.cpu(), ref[:, 3:]) and torch.equal(past, future)
    res = evaluate_rollout(lambda past: past, loader, 3, mean=KTH[0], std=KTH[1], device=dev)
    assert res["samples"] == 3
    assert np.all(np.isinf(res["psnr"]) | (np.abs(res["psnr"] - 80.0) <= 1e-4)), res["psnr"]
    assert np.all(np.abs(res["ssim"] - 1.0) < 1e-5) and np.all(res["mse"] == 0.0)


def test_graph_capture(dev):
    """the call inside torch.cuda.graph, replayed twice onto refilled inputs, equal to eager"""
    import vptr_amd.ops as ops
    gi = 3
    plan = plan_for(gi)
    raws = [case(gi, kind, N=2, T=5, flips=f) for kind, f in (("random", (1, 2)), ("ramp", (3, 0)), ("binary", (0, 1)))]
    flips = [(1, 2), (3, 0), (0, 1)]
    raw_s = torch.from_numpy(raws[0][0]).to(dev)
    fl_s = torch.tensor(flips[0], dtype=torch.int32, device=dev)
    outs = (torch.full((2, 2) + tuple(raws[0][1].shape[2:]), NAN, device=dev), torch.full((2, 3) + tuple(raws[0][1].shape[2:]), NAN, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ingest_clips(raw_s, plan, flips=fl_s, out=outs)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.ingest_clips(raw_s, plan, flips=fl_s, out=outs)
    for (raw, ref), f in list(zip(raws, flips))[1:]:
        raw_s.copy_(torch.from_numpy(raw))
        fl_s.copy_(torch.tensor(f, dtype=torch.int32))
        for o in outs:
            o.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.ingest_clips(raw_s, plan, flips=fl_s, split=2)
        assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])
        assert torch.equal(outs[0].cpu(), ref[:, :2]) and torch.equal(outs[1].cpu(), ref[:, 2:])
    g.reset()


# ------------------------------------------------------------------------------------------------------ 6. guards
@pytest.mark.parametrize("change,word", [(dict(C=2), "C 2"), (dict(Wout=257), "256"), (dict(Hout=0), "256"), (dict(left=30), "crop box"),
                                         (dict(top=-1), "crop box"), (dict(Hc=0), "crop box"), (dict(ksx=19), "8x"), (dict(ksy=19), "8x"),
                                         (dict(Tp=4), "Tp"), (dict(Tp=-1), "Tp"), (dict(out1=None), "out1"), (dict(kx=None), "horizontal"),
                                         (dict(raw=None), "null")])
def test_c_abi_rejects_before_any_launch(dev, change, word):
    from vptr_amd._lib import lib, ptr, stream
    a = dict(N=1, T=3, Tp=2, Hin=20, Win=40, C=1, top=2, left=4, Hc=16, Wc=32, Hout=8, Wout=16, ksx=5, ksy=5)
    raw = torch.zeros(3 * 20 * 40 * 3, dtype=torch.uint8, device=dev)
    tab = torch.zeros(257 * 19, dtype=torch.int32, device=dev)
    lut = torch.zeros(3 * 256, device=dev)
    out = torch.full((3 * 3 * 8 * 257,), 7.25, device=dev)
    p = dict(raw=ptr(raw), kx=ptr(tab), bx=ptr(tab), ky=ptr(tab), by=ptr(tab), lut=ptr(lut), flips=None, out0=ptr(out), out1=ptr(out))
    a.update({k: v for k, v in change.items() if k in a})
    p.update({k: v for k, v in change.items() if k in p})
    rc = lib.vptr_clip_ingest(p["raw"], p["kx"], p["bx"], p["ky"], p["by"], p["lut"], p["flips"], p["out0"], p["out1"], a["N"], a["T"],
                              a["Tp"], a["Hin"], a["Win"], a["C"], a["top"], a["left"], a["Hc"], a["Wc"], a["Hout"], a["Wout"], a["ksx"],
                              a["ksy"], stream())
    assert rc != 0
    msg = lib.vptr_last_error().decode()
    assert "clip_ingest" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())                                                              # nothing was launched


def test_op_guards(dev):
    import vptr_amd.ops as ops
    plan = plan_for(3)                                                                            # 37 x 53 x 3 -> 16 x 24
    raw = torch.zeros((2, 3, 37, 53, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.ingest_clips(raw.float(), plan)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.ingest_clips(torch.zeros((2, 3, 37, 3, 53), dtype=torch.uint8, device=dev).transpose(3, 4), plan)
    with pytest.raises(RuntimeError, match="for this plan"):
        ops.ingest_clips(raw[:, :, :, :, :1].contiguous(), plan)                                  # wrong channel count
    with pytest.raises(RuntimeError, match="for this plan"):
        ops.ingest_clips(raw[0], plan)                                                            # 4-d
    with pytest.raises(RuntimeError, match="Tp 4"):
        ops.ingest_clips(raw, plan, split=4)
    with pytest.raises(RuntimeError, match=r"\(Tp, Tf\)"):
        ops.ingest_clips(raw, plan, split=(2, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.ingest_clips(raw, plan, out=torch.zeros((2, 3, 3, 16, 25), device=dev))               # wrong shape
    with pytest.raises(RuntimeError, match="out must be"):
        ops.ingest_clips(raw, plan, out=torch.zeros((2, 3, 3, 16, 24), device=dev, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.ingest_clips(raw, plan, split=1, out=(torch.zeros((2, 1, 3, 16, 24), device=dev), torch.zeros((2, 1, 3, 16, 24), device=dev)))
    with pytest.raises(RuntimeError, match="pair"):
        ops.ingest_clips(raw, plan, split=1, out=torch.zeros((2, 3, 3, 16, 24), device=dev))
    with pytest.raises(RuntimeError, match="flips must be"):
        ops.ingest_clips(raw, plan, flips=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="flips must be"):
        ops.ingest_clips(raw, plan, flips=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ingest_clips(raw, plan, flips=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="8x"):                                                 # a 9x downscale: ksize 19
        ops.ingest_clips(torch.zeros((1, 1, 90, 90, 1), dtype=torch.uint8, device=dev), IngestPlan((90, 90), 1, (10, 10), device=dev))
    with pytest.raises(RuntimeError, match="256"):
        ops.ingest_clips(torch.zeros((1, 1, 4, 300, 1), dtype=torch.uint8, device=dev), IngestPlan((4, 300), 1, (4, 257), device=dev))
    out = ops.ingest_clips(raw, plan)
    assert not out.requires_grad and bool(torch.isfinite(out).all())
