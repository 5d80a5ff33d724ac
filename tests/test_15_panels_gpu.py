"""Sample panels on the device: vptr_clip_panels through the C ABI and through ops.clip_panels against the literal builder of panels_ref.py
(checked against a second formulation by test_panels_cpu.py), the strided and unaligned paths, ingest -> panels round trips, one graph
capture, the GIF writer, the three *_show_samples, export_rollout and the guards of both layers.

Every comparison is torch.equal: the kernel runs the reference's fp32 operations one by one, so there is no tolerance.  Every C-ABI output
lies inside a larger uint8 buffer that is filled with a sentinel first, 0x00 and 0xA5 in turn: the guard bytes must keep it, and an
unwritten output byte cannot equal the expected byte under both."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import build_transformer
from oracle import fill
from panels_ref import BAIR, KTH, MNIST, consts, grid_clip, ref_panels, special_values, spread_clip

pytestmark = pytest.mark.gpu

SENTINELS = (0x00, 0xA5)
GUARD = 64          # bytes on either side of an output: a multiple of 4, so an aligned buffer keeps the dword stores

# (C, H, W), N, clip lengths
GEOMS = [((1, 1, 1), 2, (3, 3, 3)),          # smallest
         ((1, 3, 5), 2, (3, 3, 3)),          # scalar tail
         ((3, 2, 6), 2, (3, 3, 3)),          # 18-byte rows
         ((3, 5, 7), 2, (3, 3, 3)),          # scalar tail with 3 channels
         ((1, 8, 4), 2, (3, 3, 3)),          # one vector quad
         ((1, 64, 64), 2, (2, 3, 3)),        # the models' own sizes
         ((3, 64, 64), 2, (2, 3, 3)),
         ((1, 128, 128), 1, (2, 2, 2)),      # KTH 128
         ((3, 256, 256), 1, (1,))]           # one sample, one frame
IDS = ["%dx%dx%d" % g[0] for g in GEOMS]
KINDS = ("grid", "spread")
CLIP_SETS = [(10, 10, 10), (2, 5, 5), (3, 7, 6), (4,), (3, 3, 3, 3)]


def make_clips(chw, N, lengths, kind, seed):
    C, H, W = chw
    if kind == "grid":
        return [grid_clip((N, T, C, H, W), seed + k)[0] for k, T in enumerate(lengths)]
    return [spread_clip((N, T, C, H, W), seed + k) for k, T in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def case(gi, kind):
    """(fp32 CPU clips, builder panels with the dataset's renormalisation, clamp, floor, frames, reference padding); built once, never
    written to"""
    chw, N, lengths = GEOMS[gi]
    clips = make_clips(chw, N, lengths, kind, 9000 + 100 * gi + 10 * KINDS.index(kind))
    return clips, ref_panels(clips, *consts(chw[0]))


def renorm_d(C, dev, ms=None):
    from vptr_amd.visualize import ReNorm
    mean, std = ms or consts(C)
    return ReNorm(mean, std).tensors(C, dev)


def abi_panels(clips_d, a=None, b=None, clamp=0, nearest=0, rgb=0, layout=0, pads=None, sentinel=0, guard=GUARD):
    """one direct C-ABI call into [guard | out | guard], everything filled with `sentinel` first; the guard bytes must keep it"""
    from vptr_amd._lib import check, lib, ptr, stream
    from vptr_amd.ops.panels import pad_indices, panel_shape
    K = len(clips_d)
    N, _, C, H, W = clips_d[0].shape
    lengths = [int(x.shape[1]) for x in clips_d]
    pads = pad_indices(lengths) if pads is None else pads
    shape = panel_shape(N, lengths, C, H, W, ("frames", "sheet")[layout], bool(rgb))
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), sentinel, dtype=torch.uint8, device=clips_d[0].device)
    out = buf[guard:guard + n].view(shape)
    check(lib.vptr_clip_panels((ctypes.c_void_p * K)(*[x.data_ptr() for x in clips_d]), (ctypes.c_int32 * K)(*lengths),
                               (ctypes.c_int64 * K)(*[x.stride(0) if x.shape[0] > 1 else 0 for x in clips_d]),
                               (ctypes.c_int64 * K)(*[x.stride(1) if x.shape[1] > 1 else 0 for x in clips_d]), (ctypes.c_int32 * K)(*pads),
                               ptr(a), ptr(b), ptr(out), K, N, C, H, W, clamp, nearest, rgb, layout, stream()), "vptr_clip_panels")
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all()), "guard bytes changed"
    return out


def differ(got, ref):
    return "%d of %d bytes differ" % (int((got.cpu() != ref).sum()), ref.numel())


# ------------------------------------------------------------------------------------------------------ 1. geometries
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_geometry(dev, gi, kind):
    import vptr_amd.ops as ops
    clips, ref = case(gi, kind)
    if kind == "spread":                                     # both ends of the range are populated
        lo, hi = float((ref == 0).float().mean()), float((ref == 255).float().mean())
        assert ref.numel() < 1000 or (0.02 < lo < 0.20 and 0.02 < hi < 0.20), (lo, hi)
    clips_d = [c.to(dev) for c in clips]
    a, b = renorm_d(GEOMS[gi][0][0], dev)
    for s in SENTINELS:
        got = abi_panels(clips_d, a, b, clamp=1, sentinel=s)
        assert torch.equal(got.cpu(), ref), "abi %s %s sentinel %#x: %s" % (IDS[gi], kind, s, differ(got, ref))
    op = ops.clip_panels(clips_d, a, b)
    assert op.dtype == torch.uint8 and tuple(op.shape) == tuple(ref.shape) and op.is_contiguous()
    assert torch.equal(op.cpu(), ref), "op %s %s: %s" % (IDS[gi], kind, differ(op, ref))


# ------------------------------------------------------------------------------------------------------ 2. clip sets, layouts, pads
@pytest.mark.parametrize("chw", [(1, 8, 4), (3, 5, 7)], ids=["1x8x4", "3x5x7"])
@pytest.mark.parametrize("lengths", CLIP_SETS, ids=lambda v: "-".join(str(e) for e in v))
def test_clip_sets_layouts_pads(dev, lengths, chw):
    import vptr_amd.ops as ops
    from vptr_amd.ops.panels import pad_indices
    a, b = renorm_d(chw[0], dev)
    for N in (1, 3):
        clips = make_clips(chw, N, lengths, "grid", 9900 + 7 * len(lengths) + N)
        clips_d = [c.to(dev) for c in clips]
        for li, layout in enumerate(("frames", "sheet")):
            for pad in ("reference", "last", "blank"):
                ref = ref_panels(clips, *consts(chw[0]), layout=layout, pad=pad)
                for s in SENTINELS:
                    got = abi_panels(clips_d, a, b, clamp=1, layout=li, pads=pad_indices(lengths, pad), sentinel=s)
                    assert torch.equal(got.cpu(), ref), (N, layout, pad, s, differ(got, ref))
                op = ops.clip_panels(clips_d, a, b, layout=layout, pad=pad)
                assert torch.equal(op.cpu(), ref), (N, layout, pad, differ(op, ref))


# ------------------------------------------------------------------------------------------------------ 3. options
@pytest.mark.parametrize("chw", [(1, 8, 4), (1, 3, 5), (3, 2, 6)], ids=["1x8x4", "1x3x5", "3x2x6"])
def test_quantize_renorm_gray_to_rgb(dev, chw):
    import vptr_amd.ops as ops
    C = chw[0]
    grid = make_clips(chw, 2, (2, 3), "grid", 9950)
    unit = [grid_clip((2, T) + chw, 9960 + T, *MNIST)[0] for T in (2, 3)]            # v / 255: in range without a renormalisation
    for clips, ms in ((grid, consts(C)), (unit, None)):
        clips_d = [c.to(dev) for c in clips]
        a, b = renorm_d(C, dev, ms) if ms else (None, None)
        mean, std = ms if ms else (None, None)
        for quantize in ("floor", "nearest"):
            for rgb in (False, True):
                for clamp in (None, True, False):
                    ref = ref_panels(clips, mean, std, clamp=clamp, quantize=quantize, gray_to_rgb=rgb)
                    assert ref.shape[-1] == (3 if rgb or C == 3 else 1)
                    c_abi = int(ms is not None if clamp is None else clamp)
                    for s in SENTINELS:
                        got = abi_panels(clips_d, a, b, clamp=c_abi, nearest=int(quantize == "nearest"), rgb=int(rgb), sentinel=s)
                        assert torch.equal(got.cpu(), ref), (quantize, rgb, clamp, s, differ(got, ref))
                    op = ops.clip_panels(clips_d, a, b, clamp=clamp, quantize=quantize, gray_to_rgb=rgb)
                    assert torch.equal(op.cpu(), ref), (quantize, rgb, clamp, differ(op, ref))


@pytest.mark.parametrize("renorm", [None, MNIST, KTH], ids=["plain", "mnist", "kth"])
@pytest.mark.parametrize("clamp", [0, 1])
def test_specials(dev, clamp, renorm):
    """NaN, +-inf, +-0, 1 and its neighbours, values outside [0, 1]: equal to the builder with the stated saturation (q < 0 -> 0, q > 255 ->
    255, NaN -> 0), which is the literal cast wherever that is defined (test_panels_cpu.py)"""
    sv = special_values()
    x = sv.repeat(4)[:64].view(1, 2, 1, 4, 8).contiguous()                          # vector path
    y = sv.repeat(4)[:70].view(1, 2, 1, 5, 7).contiguous()                          # scalar path
    for clip in (x, y):
        a, b = renorm_d(1, dev, renorm) if renorm else (None, None)
        mean, std = renorm if renorm else (None, None)
        for nearest in (0, 1):
            ref = ref_panels([clip], mean, std, clamp=bool(clamp), quantize=("floor", "nearest")[nearest], saturate=True)
            for s in SENTINELS:
                got = abi_panels([clip.to(dev)], a, b, clamp=clamp, nearest=nearest, sentinel=s)
                assert torch.equal(got.cpu(), ref), (nearest, s, got.cpu().view(-1)[:18].tolist(), ref.view(-1)[:18].tolist())


# ------------------------------------------------------------------------------------------------------ 4. views, alignment, out=
@pytest.mark.parametrize("chw", [(1, 8, 8), (3, 5, 7)], ids=["1x8x8", "3x5x7"])
def test_strided_views_are_read_in_place(dev, chw):
    import vptr_amd.ops as ops
    base = grid_clip((4, 6) + chw, 9970)[0]
    base_d = base.to(dev)
    views = lambda t: [t[0:2, 1:], t[0:2, :-1], t[::2]]                             # noqa: E731  (N 2: T 5, 5, 6)
    vd = views(base_d)
    assert not vd[0].is_contiguous() and not vd[2].is_contiguous() and vd[0].data_ptr() != base_d.data_ptr()
    a, b = renorm_d(chw[0], dev)
    for layout in ("frames", "sheet"):
        ref = ref_panels(views(base), *consts(chw[0]), layout=layout)
        got = ops.clip_panels(vd, a, b, layout=layout)
        assert torch.equal(got.cpu(), ref), (layout, differ(got, ref))
    for s in SENTINELS:
        got = abi_panels(vd, a, b, clamp=1, sentinel=s)
        assert torch.equal(got.cpu(), ref_panels(views(base), *consts(chw[0])))
    wide = base_d[:2, :1].expand(2, 3, *chw)                                        # frame stride 0
    assert torch.equal(ops.clip_panels([wide], a, b).cpu(), ref_panels([base[:2, :1].expand(2, 3, *chw)], *consts(chw[0])))


def test_unaligned_and_aligned_bases(dev):
    """W % 4 == 0 with a clip one float past a 16-byte boundary (scalar loads), with the output one byte past a dword boundary (byte stores),
    and both aligned (16-byte loads, dword stores): the same bytes"""
    import vptr_amd.ops as ops
    for C in (1, 3):
        clips, (a, b) = make_clips((C, 8, 8), 2, (2, 3), "grid", 9980 + C), renorm_d(C, dev)
        ref = ref_panels(clips, *consts(C))
        aligned = [c.to(dev) for c in clips]
        off = []
        for c in clips:
            flat = torch.empty(c.numel() + 1, device=dev)
            v = flat[1:].view(c.shape)
            v.copy_(c)
            off.append(v)
        assert all(x.data_ptr() % 16 == 0 for x in aligned) and all(x.data_ptr() % 16 == 4 for x in off)
        for s in SENTINELS:
            assert torch.equal(abi_panels(aligned, a, b, clamp=1, sentinel=s).cpu(), ref)
            assert torch.equal(abi_panels(off, a, b, clamp=1, sentinel=s).cpu(), ref)
            assert torch.equal(abi_panels([aligned[0], off[1]], a, b, clamp=1, sentinel=s).cpu(), ref)
            got = abi_panels(aligned, a, b, clamp=1, sentinel=s, guard=61)
            assert got.data_ptr() % 4 != 0 and torch.equal(got.cpu(), ref)
        assert torch.equal(ops.clip_panels(off, a, b).cpu(), ref)


def test_out_given_and_two_calls_bit_identical(dev):
    import vptr_amd.ops as ops
    clips, ref = case(5, "grid")
    clips_d = [c.to(dev) for c in clips]
    a, b = renorm_d(1, dev)
    out = torch.full(tuple(ref.shape), 0xA5, dtype=torch.uint8, device=dev)
    assert ops.clip_panels(clips_d, a, b, out=out) is out
    again = ops.clip_panels(clips_d, a, b)
    assert torch.equal(out, again) and torch.equal(out.cpu(), ref)


def test_offsets_past_2_31(dev):
    """every element offset is 64-bit: a panel of 2.2e9 bytes written from broadcast views (frame stride 0, so the inputs stay small), and a
    frame that lies 2^31 floats behind its clip's base"""
    import vptr_amd.ops as ops
    small = [grid_clip((1, 1, 1, 256, 256), 9985 + k)[0] for k in range(4)]
    ref = ref_panels(small, *KTH, gray_to_rgb=True).to(dev)                          # (1, 1, 256, 1024, 3)
    L = 2800
    a, b = renorm_d(1, dev)
    out = torch.full((1, L, 256, 1024, 3), 0xA5, dtype=torch.uint8, device=dev)
    assert out.numel() > 2 ** 31
    ops.clip_panels([c.to(dev).expand(1, L, 1, 256, 256) for c in small], a, b, gray_to_rgb=True, out=out)
    assert bool((out == ref).all()) and torch.equal(out[0, L - 1], ref[0, 0])
    del out
    far = torch.empty(2 ** 31 + 64, device=dev)
    clip = far.as_strided((1, 2, 1, 8, 8), (0, 2 ** 31, 64, 8, 1))
    frames = grid_clip((1, 2, 1, 8, 8), 9989)[0]
    clip.copy_(frames)
    assert clip[0, 1].data_ptr() - clip.data_ptr() == 4 * 2 ** 31
    assert torch.equal(ops.clip_panels([clip], a, b).cpu(), ref_panels([frames], *KTH))
    del far, clip
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ 5. whole paths
@pytest.mark.parametrize("preset", ["bair", "mnist"])
def test_ingest_then_nearest_returns_the_bytes(dev, preset):
    """uint8 frames -> ClipIngest's fp32 tensors -> panels with quantize="nearest": the ingested bytes, all of them"""
    import vptr_amd.ops as ops
    from vptr_amd.data import IngestPlan
    from vptr_amd.visualize import ReNorm, clips_to_uint8
    plan = IngestPlan.bair(device=dev) if preset == "bair" else IngestPlan.mnist(device=dev)
    C = plan.channels
    raw = torch.from_numpy(np.random.RandomState(9990).randint(0, 256, size=(2, 3, 64, 64, C)).astype(np.uint8)).to(dev)
    raw[0, 0, 0, :, :] = torch.arange(64, dtype=torch.uint8, device=dev).view(64, 1) * 4        # every fourth level for certain
    x = ops.ingest_clips(raw, plan)
    back = clips_to_uint8([x], renorm=ReNorm(plan.mean, plan.std), quantize="nearest")
    assert torch.equal(back, raw)
    if preset == "bair":
        floor = clips_to_uint8([x], renorm=ReNorm(plan.mean, plan.std))
        share = float((floor == raw).float().mean())
        assert 0.6 < share < 0.9 and int((floor.int() - raw.int()).abs().max()) == 1, share      # ToPILImage's truncation loses a quarter


def test_graph_capture(dev):
    """the call inside torch.cuda.graph, replayed onto overwritten inputs: the outputs follow and equal the builder's"""
    import vptr_amd.ops as ops
    chw, N, lengths = (1, 8, 8), 2, (2, 4, 4)
    sets = [make_clips(chw, N, lengths, kind, seed) for kind, seed in (("grid", 9991), ("spread", 9992), ("grid", 9993))]
    a, b = renorm_d(1, dev)
    static = [c.to(dev) for c in sets[0]]
    out = torch.zeros((N, 4, 8, 24, 1), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.clip_panels(static, a, b, out=out)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.clip_panels(static, a, b, out=out)
    for clips in sets[1:]:
        for s, c in zip(static, clips):
            s.copy_(c)
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), ref_panels(clips, *KTH))
    g.reset()


# ------------------------------------------------------------------------------------------------------ 6. files
@pytest.mark.parametrize("C", [1, 3])
def test_visualize_batch_clips_writes_the_builders_gifs(dev, tmp_path, C):
    """unequal clip lengths: the files are byte-identical to the GIFs PIL writes from the builder's arrays"""
    Image = pytest.importorskip("PIL.Image")
    from vptr_amd.visualize import ReNorm, visualize_batch_clips
    past, fut, pred = make_clips((C, 16, 16), 2, (2, 4, 4), "grid", 9994 + C)
    mean, std = consts(C)
    got = visualize_batch_clips(past.to(dev), fut.to(dev), pred.to(dev), tmp_path / "got", ReNorm(mean, std), desc="pred")
    ref = ref_panels([past, fut, pred], mean, std).numpy()
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, ref)
    (tmp_path / "want").mkdir()
    for n in range(2):
        imgs = [Image.fromarray(ref[n, t, :, :, 0], "L") if C == 1 else Image.fromarray(ref[n, t], "RGB") for t in range(4)]
        imgs[0].save(str(tmp_path / "want" / ("pred_clip_%d.gif" % n)), save_all=True, append_images=imgs[1:])
        assert (tmp_path / "got" / ("pred_clip_%d.gif" % n)).read_bytes() == (tmp_path / "want" / ("pred_clip_%d.gif" % n)).read_bytes()
    assert sorted(p.name for p in (tmp_path / "got").iterdir()) == ["pred_clip_0.gif", "pred_clip_1.gif"]


# ------------------------------------------------------------------------------------------------------ 7. the scripts' sample functions
class Rec:
    """a module that keeps what it returned, so that the builder is applied to the very tensors the sample functions saw"""

    def __init__(self, m):
        self.m, self.outs = m, []

    def eval(self):
        self.m.eval()
        return self

    def __call__(self, *args, **kw):
        r = self.m(*args, **kw)
        self.outs.append(r)
        return r

    def __getattr__(self, name):
        return getattr(self.m, name)


FEAT, HW = 48, 64


def tiny_ae(dev):
    import vptr_amd.model as pkg
    enc, dec = pkg.VPTREnc(1, FEAT, 3, "reflect").eval(), pkg.VPTRDec(1, FEAT, 3, "Sigmoid", "reflect").eval()
    fill.apply_fill(enc, 71)
    fill.apply_fill(dec, 72)
    return enc.to(dev), dec.to(dev)


def zero_pad(c, T):
    return torch.cat([c, torch.zeros((c.shape[0], T - c.shape[1]) + tuple(c.shape[2:]), device=c.device)], dim=1) if c.shape[1] < T else c


def names(d):
    return sorted(p.name for p in d.iterdir())


def test_ae_show_samples(dev, tmp_path):
    from vptr_amd.visualize import ReNorm, ae_show_samples
    enc, dec = tiny_ae(dev)
    dec = Rec(dec)
    past, future = fill.rand_input((5, 2, 1, HW, HW), 1200), fill.rand_input((5, 2, 1, HW, HW), 1201)
    got = ae_show_samples(enc, dec, (past, future), tmp_path, ReNorm(*KTH), device=dev)
    rec_past, rec_future = dec.outs
    assert torch.equal(torch.from_numpy(got["ae"]), ref_panels([past[:4], rec_future[:4], rec_past[:4]], *KTH))
    assert tuple(got["ae"].shape) == (4, 2, HW, 3 * HW, 1) and names(tmp_path) == ["ae_clip_%d.gif" % n for n in range(4)]   # min(N, 4)


def test_nar_show_samples(dev, tmp_path):
    """2 past, 3 future frames: the past and its reconstruction are zero-padded in the model's range, as train_NAR.py does"""
    import vptr_amd.model as pkg
    from vptr_amd.visualize import nar_show_samples
    enc, dec = tiny_ae(dev)
    dec = Rec(dec)
    T = build_transformer(pkg, dict(Tp=2, Tf=3, H=8, W=8, C=FEAT, nhead=8, window_size=4, num_encoder_layers=1, num_decoder_layers=1,
                                    rpe=True), False)
    fill.apply_fill(T, 73)
    T = T.to(dev)
    past, future = fill.rand_input((2, 2, 1, HW, HW), 1210), fill.rand_input((2, 3, 1, HW, HW), 1211)
    got = nar_show_samples(enc, dec, T, (past, future), tmp_path, None, device=dev)
    rec_past, rec_future, pred = dec.outs
    assert tuple(pred.shape) == (2, 3, 1, HW, HW) and not T.training
    assert torch.equal(torch.from_numpy(got["pred"]), ref_panels([zero_pad(past, 3), future, pred]))
    assert torch.equal(torch.from_numpy(got["ae"]), ref_panels([zero_pad(past, 3), rec_future, zero_pad(rec_past, 3)]))
    assert names(tmp_path) == ["ae_clip_0.gif", "ae_clip_1.gif", "pred_clip_0.gif", "pred_clip_1.gif"]


@pytest.mark.parametrize("test_phase", [True, False])
def test_far_show_samples(dev, tmp_path, test_phase):
    import vptr_amd.model as pkg
    from vptr_amd.visualize import ReNorm, far_show_samples
    enc, dec = tiny_ae(dev)
    dec = Rec(dec)
    T = build_transformer(pkg, dict(Tp=3, Tf=3, H=8, W=8, C=FEAT, nhead=8, window_size=4, num_encoder_layers=2, rpe=True), True)
    fill.apply_fill(T, 75)
    T = T.to(dev)
    num_pred = 3
    past, future = fill.rand_input((2, 3, 1, HW, HW), 1220), fill.rand_input((2, 3, 1, HW, HW), 1221)
    got = far_show_samples(enc, dec, T, num_pred, (past, future), tmp_path, ReNorm(*KTH), device=dev, test_phase=test_phase)
    frames = dec.outs[-1]                                                       # the one decoder pass over every predicted feature
    assert tuple(frames.shape) == (2, 5, 1, HW, HW)
    pred_past, pred_future = frames[:, :-num_pred], frames[:, -num_pred:]
    assert torch.equal(torch.from_numpy(got["pred_future"]), ref_panels([past, future, pred_future], *KTH))
    assert torch.equal(torch.from_numpy(got["pred_past"]), ref_panels([past[:, 1:], pred_past, pred_future[:, :-1]], *KTH))
    assert tuple(got["pred_past"].shape) == (2, 2, HW, 3 * HW, 1)
    assert names(tmp_path) == ["pred_future_clip_0.gif", "pred_future_clip_1.gif", "pred_past_clip_0.gif", "pred_past_clip_1.gif"]


def test_export_rollout_far_cached(dev):
    """uint8 [N, T, H, W, C] videos of a KV-cached tiny FAR rollout and of its ground truth, grey as three channels"""
    import vptr_amd.model as pkg
    from vptr_amd.inference import far_rollout
    from vptr_amd.visualize import ReNorm, export_rollout
    enc, dec = tiny_ae(dev)
    far = build_transformer(pkg, dict(Tp=3, Tf=3, H=8, W=8, C=FEAT, nhead=8, window_size=4, num_encoder_layers=2, rpe=True), True)
    fill.apply_fill(far, 75)
    far = far.to(dev)
    seen = []

    def predict(past):
        seen.append(far_rollout(enc, dec, far, past, 3, mode="train", kv_cache=True)[1])
        return seen[-1]

    loader = [(fill.rand_input((n, 3, 1, HW, HW), 1230 + i), grid_clip((n, 3, 1, HW, HW), 1240 + i)) for i, n in enumerate((2, 1))]
    batches = list(export_rollout(predict, [(p, f[0]) for p, f in loader], 2, ReNorm(*KTH), gray_to_rgb=True, device=dev))
    assert len(batches) == 2 and len(seen) == 2
    for (pred_u8, gt_u8), pred, (_, (fut, fut_bytes)) in zip(batches, seen, loader):
        n = pred.shape[0]
        assert pred_u8.dtype == gt_u8.dtype == np.uint8 and pred_u8.shape == gt_u8.shape == (n, 2, HW, HW, 3)
        assert np.array_equal(pred_u8, ref_panels([pred[:, :2]], *KTH, quantize="nearest", gray_to_rgb=True).numpy())
        assert np.array_equal(gt_u8, np.repeat(fut_bytes[:, :2], 3, axis=-1))               # nearest: the original bytes
    with pytest.raises(RuntimeError, match="at least 4 frames"):
        list(export_rollout(predict, [loader[0][:1] + (loader[0][1][0],)], 4, device=dev))


# ------------------------------------------------------------------------------------------------------ 8. guards
@pytest.mark.parametrize("change,word", [(dict(K=0), "K 0"), (dict(K=5), "K 5"), (dict(C=2), "C 2"), (dict(N=0), ">= 1"), (dict(H=0), ">= 1"),
                                         (dict(W=0), ">= 1"), (dict(T=(3, 0)), "T 0"), (dict(pad=(3, -1)), "pad 3"), (dict(pad=(1, -2)), "pad -2"),
                                         (dict(sn=(256, -256)), "negative stride"), (dict(st=(-64, 64)), "negative stride"),
                                         (dict(out=None), "null"), (dict(clips=None), "null"), (dict(clip1=None), "clip 1 is a null"),
                                         (dict(b=None), "together"), (dict(layout=2), "layout 2"), (dict(N=2 ** 31 - 1, H=64), "workgroups")])
def test_c_abi_rejects_before_any_launch(dev, change, word):
    from vptr_amd._lib import lib, ptr, stream
    x = torch.zeros((2, 5, 3, 4, 16), device=dev)
    ab = torch.ones(3, device=dev)
    out = torch.full((2 * 5 * 4 * 32 * 3,), 0xA5, dtype=torch.uint8, device=dev)
    v = dict(K=2, N=1, C=1, H=4, W=16, T=(3, 4), pad=(1, -1), sn=(256, 256), st=(64, 64), layout=0)
    v.update({k: c for k, c in change.items() if k in v})
    clips = None if "clips" in change else (ctypes.c_void_p * 2)(x.data_ptr(), None if "clip1" in change else x.data_ptr())
    rc = lib.vptr_clip_panels(clips, (ctypes.c_int32 * 2)(*v["T"]), (ctypes.c_int64 * 2)(*v["sn"]), (ctypes.c_int64 * 2)(*v["st"]),
                              (ctypes.c_int32 * 2)(*v["pad"]), ptr(ab), None if "b" in change else ptr(ab), None if "out" in change else ptr(out),
                              v["K"], v["N"], v["C"], v["H"], v["W"], 1, 0, 0, v["layout"], stream())
    assert rc != 0
    msg = lib.vptr_last_error().decode()
    assert "clip_panels" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                                              # nothing was launched


def test_op_guards(dev):
    import vptr_amd.ops as ops
    from vptr_amd.visualize import ReNorm, clips_to_uint8
    x = torch.zeros((2, 3, 1, 4, 8), device=dev)
    a, b = renorm_d(1, dev)
    with pytest.raises(RuntimeError, match="float32"):
        ops.clip_panels([x.double()])
    with pytest.raises(RuntimeError, match="float32"):
        ops.clip_panels([x[0]])                                                                   # 4-d
    with pytest.raises(RuntimeError, match="does not match clip 0"):
        ops.clip_panels([x, x[:1]])
    with pytest.raises(RuntimeError, match="does not match clip 0"):
        ops.clip_panels([x, torch.zeros((2, 3, 1, 4, 4), device=dev)])
    with pytest.raises(RuntimeError, match="empty dimension"):
        ops.clip_panels([x[:, :0]])
    with pytest.raises(RuntimeError, match="C 2"):
        ops.clip_panels([torch.zeros((2, 3, 2, 4, 8), device=dev)])
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.clip_panels([torch.zeros((2, 3, 1, 8, 4), device=dev).transpose(3, 4)])
    with pytest.raises(RuntimeError, match="must be contiguous"):
        ops.clip_panels([torch.zeros((2, 3, 1, 4, 16), device=dev)[..., ::2]])
    with pytest.raises(RuntimeError, match="together"):
        ops.clip_panels([x], a=a)
    with pytest.raises(RuntimeError, match=r"a must be a contiguous float32 \[1\]"):
        ops.clip_panels([x], a=torch.ones(3, device=dev), b=b)
    with pytest.raises(RuntimeError, match="b must be"):
        ops.clip_panels([x], a=a, b=b.double())
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.clip_panels([x], a=a.cpu(), b=b)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.clip_panels([x, x.cpu()])
    with pytest.raises(RuntimeError, match="T = 1 < 2"):
        ops.clip_panels([x[:, :1], x])
    with pytest.raises(RuntimeError, match="out must be"):
        ops.clip_panels([x], out=torch.zeros((2, 3, 4, 8, 3), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.clip_panels([x], out=torch.zeros((2, 3, 4, 8, 1), device=dev))
    with pytest.raises(RuntimeError, match="between 1 and 4"):
        ops.clip_panels([x] * 5)
    with pytest.raises(ValueError, match="entries for 1 channels"):
        clips_to_uint8([x], renorm=ReNorm(*BAIR))
    ok = ops.clip_panels([x[:, :1], x], pad="last")
    assert tuple(ok.shape) == (2, 3, 4, 16, 1) and not ok.requires_grad and bool((ok == 0).all())
