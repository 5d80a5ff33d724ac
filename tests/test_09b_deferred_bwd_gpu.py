"""Op-level fp64 parity of the backward kernels the trainers run for slab-backed parameters: the deferred LayerNorm(C) backward
(`vptr_layernorm_bwd_deferred`), the end-of-backward partial-sum reduction (`vptr_partial_reduce`), the LayerNorm((F,H,W)) backward of the
conv-FFN in its atomic and deferred forms (`vptr_norm_act_bwd`, `vptr_norm_act_bwd_deferred`), the depthwise weight gradient from the fp16 side
copy (`vptr_dwconv3x3_bwd_xh`) with the launch classes of `vptr_dwconv3x3_bwd` the step takes -- all through the C ABI -- and one integration
test of the autograd / slab / flush wiring through `ops`.

Every reference is plain torch fp64 on the CPU from the same seeded inputs (helpers.ln_bwd_ref, helpers.norm_act_ln_bwd_ref -- both checked
against closed forms in tests/test_cpu.py --, F.conv2d + autograd).  Every output and every partial-sum buffer is NaN-filled before the call:
an element a kernel never writes fails its comparison.  Destinations that are accumulated into (dw / db, dw9 / db, the reduce destinations)
start from non-zero values that the reference includes.  Bars (rel-L2): fp32 vector kernels 2e-5, their gradients
5e-5, a P16 output 2^-16.  ReLU: the kink rule of tests/test_09_stage1_ops_gpu.py (upstream gradient zeroed where |pre| < 1e-3 rms(pre),
share <= 0.5 %).
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import KINK_CAP, NORM_ACT_LN_CASES, ln_bwd_ref, norm_act_ln_bwd_ref, norm_act_ln_inputs, rel
from oracle import fill

pytestmark = pytest.mark.gpu

TOLV = 2e-5                      # fp32 vector kernels
TOLG = 5e-5                      # their gradients
TOLP16 = 2.0 ** -16              # a P16 image of a kernel's output
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def abi():
    from vptr_amd import _lib
    return _lib


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def cdiv(a, b):
    return (a + b - 1) // b


@contextlib.contextmanager
def deterministic(ops, on):
    """the launchers' mode for the enclosed calls, restored afterwards (as test_09's det_mode fixture does)"""
    prev = ops.config.deterministic
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(prev)


# ------------------------------------------------------------------------------------------------------ 1. vptr_layernorm_bwd_deferred
# default mode (rows >= 4096, 256 < C <= 768): ln_bwd_fused_kernel<3, 4>, 16 rows per workgroup
#   4096 x 260: C / 4 = 65 -- ONE live lane in the second of the three 64-lane column chunks, none in the third
#   4111 x 528: the model's width; the last workgroup has 15 rows, its four waves take 4 / 4 / 4 / 3
#   4097 x 768: every column chunk full; the last workgroup has one row and three idle waves
# deterministic mode (any C % 4 == 0, C <= 1024; 32 rows per workgroup): <1, 4> (70 x 48), <3, 8> (100 x 528), <4, 4> (33 x 772: 193 quads, one
# live lane in the fourth chunk; 45 x 1024: full)
LN_CASES = [(4096, 260, False), (4111, 528, False), (4097, 768, False), (70, 48, True), (100, 528, True), (33, 772, True), (45, 1024, True)]
LN_VARIANTS = {"dy2+dx_add": (True, True), "neither": (False, False), "dx_add": (False, True)}


@functools.lru_cache(maxsize=2)
def _ln_inputs(rows, C):
    seed = 2000 + rows % 89 + C
    return (rn((rows, C), seed, 2.0) + 0.3, rn((C,), seed + 1).abs() + 0.5, rn((rows, C), seed + 2), rn((rows, C), seed + 3), rn((rows, C), seed + 4))


@pytest.mark.parametrize("variant", sorted(LN_VARIANTS))
@pytest.mark.parametrize("rows,C,det", LN_CASES)
def test_layernorm_bwd_deferred(ops, dev, abi, rows, C, det, variant):
    """dx, the partial rows summed (dgamma, dbeta) and -- separately -- the dx rows of the LAST workgroup vs fp64 autograd of F.layer_norm with
    the upstream gradient dy + dy2 and dx_add; mean / rstd are the fp64 statistics of the fp32 x, handed over as fp32"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    with_dy2, with_add = LN_VARIANTS[variant]
    x, gamma, dy, dy2, add = _ln_inputs(rows, C)
    dy2, add = (dy2 if with_dy2 else None), (add if with_add else None)
    ref = ln_bwd_ref(x, gamma, dy, dy2, add)
    rpb = 32 if det else 16
    xd, gd, dyd = x.to(dev), gamma.to(dev), dy.to(dev)
    dy2d, addd = (dy2.to(dev) if with_dy2 else None), (add.to(dev) if with_add else None)
    mean, rstd = ref["mean"].float().to(dev), ref["rstd"].float().to(dev)
    with deterministic(ops, det):
        nparts = lib.vptr_layernorm_bwd_partials(rows, C)
        assert nparts == cdiv(rows, rpb)
        part = torch.full((nparts, 2, C), NAN, device=dev)
        dx = torch.full((rows, C), NAN, device=dev)
        check(lib.vptr_layernorm_bwd_deferred(ptr(dyd), ptr(dy2d), ptr(xd), ptr(gd), ptr(mean), ptr(rstd), ptr(dx), rows, C, ptr(addd), ptr(part),
                                              stream()), "vptr_layernorm_bwd_deferred")
    assert part.shape[0] == nparts
    assert rel(dx, ref["dx"]) < TOLG
    tail = (nparts - 1) * rpb
    assert 0 < rows - tail <= rpb
    assert rel(dx[tail:], ref["dx"][tail:]) < TOLG
    sums = part.double().sum(0)
    assert rel(sums, torch.stack([ref["dgamma"], ref["dbeta"]])) < TOLG
    assert rel(sums[0], ref["dgamma"]) < TOLG and rel(sums[1], ref["dbeta"]) < TOLG


@pytest.mark.parametrize("rows,C", [(4000, 528), (4096, 256)])
def test_layernorm_bwd_deferred_rejects(ops, dev, abi, rows, C):
    """default mode has no deferred variant below 4096 rows or at C <= 256: the partial count is 0 and the call returns an error before any launch
    (dx keeps its NaN fill)"""
    lib, ptr, stream = abi.lib, abi.ptr, abi.stream
    x, gamma, dy = rn((rows, C), 1).to(dev), rn((C,), 2).to(dev), rn((rows, C), 3).to(dev)
    mean, rstd = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
    dx, part = torch.full((rows, C), NAN, device=dev), torch.full((cdiv(rows, 16), 2, C), NAN, device=dev)
    with deterministic(ops, False):
        assert lib.vptr_layernorm_bwd_partials(rows, C) == 0
        rc = lib.vptr_layernorm_bwd_deferred(ptr(dy), None, ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), rows, C, None, ptr(part), stream())
    assert rc < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(part).all())


# -------------------------------------------------------------------------------------------------------------- 2. vptr_partial_reduce
def _reduce_table(abi, dev, entries):
    """entries (part, dst0, dst1 or None, nparts, C) -> the vptr_reduce_entry table on the device (built on the host, uploaded as bytes)"""
    tab = (abi.ReduceEntry * len(entries))()
    for i, (part, d0, d1, nparts, C) in enumerate(entries):
        tab[i].part, tab[i].dst0, tab[i].dst1, tab[i].nparts, tab[i].C = abi.ptr(part), abi.ptr(d0), abi.ptr(d1), nparts, C
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)


class _Guarded:
    """destinations cut out of ONE guard buffer of known, NaN-free values: after the launch every float outside the destinations must be
    bit-unchanged, every destination holds its start value + the fp64 sum of its partial rows"""

    def __init__(self, dev, floats, seed):
        self.host = rn((floats,), seed, 0.5)
        self.buf = self.host.to(dev)
        self.want = self.host.double().clone()
        self.touched = torch.zeros(floats, dtype=torch.bool)
        self.spans = []

    def dst(self, off, C, add):      # (two entries may name the same span on purpose: their sums add up)
        self.want[off:off + C] += add
        self.touched[off:off + C] = True
        self.spans.append((off, C))
        return self.buf[off:off + C]

    def check(self):
        got = self.buf.cpu()
        assert torch.equal(got[~self.touched], self.host[~self.touched]), "a float outside every destination changed"
        for off, C in self.spans:
            assert rel(got[off:off + C], self.want[off:off + C]) < TOLV, (off, C)


def _parts(dev, nparts, rpp, C, seed):
    """partial rows [nparts][rpp][C] + their fp64 sums per row of the pair"""
    p = rn((nparts, rpp, C), seed)
    return p.to(dev), p.double().sum(0)


@pytest.mark.parametrize("nparts", [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 257])
def test_partial_reduce_row_counts(dev, abi, nparts):
    """the row loop (16 row lanes; four rows per lane and trip while p + 48 < nparts, then one by one): every boundary of 49 ... 64 and both
    sides of 16 / 64, in the [nparts][2][C] layout with two destinations and in the [nparts][C] layout with dst1 == NULL, one launch"""
    g = _Guarded(dev, 2048, 600 + nparts)
    p2, s2 = _parts(dev, nparts, 2, 260, 610 + nparts)
    p1, s1 = _parts(dev, nparts, 1, 252, 620 + nparts)
    p0, s0 = _parts(dev, nparts, 2, 4, 630 + nparts)
    entries = [(p2, g.dst(16, 260, s2[0]), g.dst(300, 260, s2[1]), nparts, 260),
               (p1, g.dst(600, 252, s1[0]), None, nparts, 252),
               (p0, g.dst(900, 4, s0[0]), g.dst(908, 4, s0[1]), nparts, 4)]
    tab = _reduce_table(abi, dev, entries)
    abi.check(abi.lib.vptr_partial_reduce(abi.ptr(tab), len(entries), 260, 1, abi.stream()), "vptr_partial_reduce")
    g.check()


@pytest.mark.parametrize("unique,shift", [(1, 0), (1, 1), (0, 0), (0, 1)], ids=["unique_aligned", "unique_scalar_branch", "atomic_aligned", "atomic_shifted"])
def test_partial_reduce_widths_in_one_launch(dev, abi, unique, shift):
    """entries of C = 4, 252, 260, 528, 1028 in one launch sized for the widest (five column blocks): a narrower entry must leave everything past
    its own C alone -- its destinations sit in a guard buffer whose other floats are compared bit for bit.  shift 1: every destination starts one
    float past a 16-byte boundary (with unique_dst the scalar read-add-write branch)"""
    g = _Guarded(dev, 8192, 640 + 2 * unique + shift)
    entries, off = [], 64 + shift
    for i, (C, nparts) in enumerate([(4, 3), (252, 17), (260, 64), (528, 70), (1028, 5)]):
        p, s = _parts(dev, nparts, 2, C, 650 + i)
        entries.append((p, g.dst(off, C, s[0]), g.dst(off + C + 12, C, s[1]), nparts, C))
        off += 2 * C + 40                       # (a multiple of 4: every destination keeps the launch's alignment class)
    for _, d0, d1, _, _ in entries:
        assert d0.data_ptr() % 16 == 4 * shift and d1.data_ptr() % 16 == 4 * shift
    tab = _reduce_table(abi, dev, entries)
    abi.check(abi.lib.vptr_partial_reduce(abi.ptr(tab), len(entries), 1028, unique, abi.stream()), "vptr_partial_reduce")
    g.check()


def test_partial_reduce_shared_destination(dev, abi):
    """unique_dst = 0: two entries (a module applied twice in one forward) name the same dst0 / dst1; both sums arrive"""
    g = _Guarded(dev, 2048, 660)
    pa, sa = _parts(dev, 17, 2, 528, 661)
    pb, sb = _parts(dev, 64, 2, 528, 662)
    d0, d1 = g.dst(32, 528, sa[0]), g.dst(600, 528, sa[1])
    g.dst(32, 528, sb[0]), g.dst(600, 528, sb[1])
    tab = _reduce_table(abi, dev, [(pa, d0, d1, 17, 528), (pb, d0, d1, 64, 528)])
    abi.check(abi.lib.vptr_partial_reduce(abi.ptr(tab), 2, 528, 0, abi.stream()), "vptr_partial_reduce")
    g.check()


def test_partial_reduce_rejects(dev, abi):
    g = _Guarded(dev, 256, 670)
    p, s = _parts(dev, 3, 2, 8, 671)
    tab = _reduce_table(abi, dev, [(p, g.dst(16, 8, 0.0), g.dst(32, 8, 0.0), 3, 8)])
    assert abi.lib.vptr_partial_reduce(abi.ptr(tab), 1, 6, 1, abi.stream()) < 0      # max_C % 4 != 0
    assert abi.lib.vptr_partial_reduce(abi.ptr(tab), 0, 8, 1, abi.stream()) < 0      # count == 0
    torch.cuda.synchronize()
    g.check()                                                                        # nothing was launched


# -------------------------------------------------------------- 3. vptr_norm_act_bwd (LayerNorm((F,H,W)) mode) and vptr_norm_act_bwd_deferred
# plain call (atomics into dw / db):
#   13 x 12 x 20:  one frame chunk, 60 float4 positions < 64: dead lanes in the only block; waves take 4 / 3 / 3 / 3 frames (F % 16 != 0: no P16 dx)
#   70 x 16 x 32:  frames >= 64 -> four chunks of 18 / 18 / 18 / 16 frames meeting in atomics
#   67 x 64 x 256: rows * F / 4 >= 2^18 -> norm_act_bwd_dx4_pos_kernel, 16 frame rows over 67 frames (not a multiple of 4)
# deferred call (partials [chunks][2][HW * F]):
#   64 x 16 x 32:  small class (HW * F < 65536): 16 chunks of 4 frames
#   70 x 16 x 32:  14 chunks of 5: wave 0 takes two frames, waves 1 .. 3 one
#   100 x 4 x 16:  16 float4 positions: one partial block of 64 lanes; 15 chunks of 7 frames, the last one of 2
#   66 x 64 x 1024: big class: 4 chunks of 17 / 17 / 17 / 15 frames, 17 MB per tensor
SITE = 13


@functools.lru_cache(maxsize=1)
def _na_inputs(case):
    return norm_act_ln_inputs(case)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "gelu", "relu"])
@pytest.mark.parametrize("case", sorted(NORM_ACT_LN_CASES))
def test_norm_act_ln_bwd(ops, dev, abi, case, act, p):
    """dx (fp32 and P16) and the affine gradients (dw / db accumulated onto non-zero start values, or the deferred call's partial rows summed) vs
    fp64 autograd of F.layer_norm over the frame, the activation, the regenerated dropout mask / keep and a DropPath-like row scale per frame"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    deferred, frames, HW, Fc = NORM_ACT_LN_CASES[case]
    rows, E = frames * HW, HW * Fc
    x, dy, w, b, rs = _na_inputs(case)
    assert 0 < int((rs == 0).sum()) < frames
    mask, seed = None, None
    if p > 0:
        ops.manual_seed(dev, 97531)
        seed = ops.new_seed_scope(dev)
        ones, md = torch.ones(rows * Fc, device=dev), torch.empty(rows * Fc, device=dev)
        check(lib.vptr_dropout(ptr(ones), ptr(md), rows * Fc, p, ptr(seed), SITE, stream()), "vptr_dropout")   # element index = row * F + col
        mask = (md.reshape(rows, Fc) != 0).float().cpu()
        assert 0.05 < float((mask == 0).double().mean()) < 0.15
        assert rel(md.reshape(rows, Fc), mask.double() / (1.0 - p)) < 1e-6                                      # kept elements carry 1 / keep
    ref = norm_act_ln_bwd_ref(x, w, b, dy, frames, HW, act, mask, 1.0 - p, rs, HW, frames)
    assert ref["kink_share"] <= KINK_CAP
    xd, dyd, wd, bd, rsd = x.to(dev), ref["dy"].float().to(dev), w.to(dev), b.to(dev), rs.to(dev)
    mean, rstd = ref["mean"].float().to(dev), ref["rstd"].float().to(dev)
    dw0, db0 = rn((HW, Fc), 680, 0.5), rn((HW, Fc), 681, 0.5)
    nscratch = max(2 * Fc, 2 * frames * (1 + 4 * cdiv(E // 4, 256)))
    nparts = lib.vptr_norm_act_bwd_partials(rows, Fc, HW, 0)
    if deferred:
        want = 4 if E >= 65536 else 16
        assert nparts == cdiv(frames, cdiv(frames, want))
    for p16 in (0, 1):
        dx = torch.full((rows, Fc), NAN, device=dev)
        scratch = torch.full((nscratch,), NAN, device=dev)
        part = torch.full((max(nparts, 1), 2, E), NAN, device=dev)
        dwd, dbd = dw0.clone().to(dev), db0.clone().to(dev)
        if deferred:
            rc = lib.vptr_norm_act_bwd_deferred(ptr(dyd), ptr(xd), ptr(mean), ptr(rstd), ptr(wd), ptr(bd), ptr(dx), ptr(scratch), rows, Fc, HW, act, 0, p,
                                                ptr(seed), SITE, ptr(rsd), HW, frames, p16, ptr(part), stream())
        else:
            rc = lib.vptr_norm_act_bwd(ptr(dyd), ptr(xd), ptr(mean), ptr(rstd), ptr(wd), ptr(bd), ptr(dx), ptr(dwd), ptr(dbd), ptr(scratch), rows, Fc, HW,
                                       0, act, 0, p, ptr(seed), SITE, ptr(rsd), HW, frames, p16, stream())
        if p16 and Fc % 16 != 0:
            assert rc < 0                      # a P16 row is made of 16-channel groups: documented rejection, nothing launched
            torch.cuda.synchronize()
            assert bool(torch.isnan(dx).all())
            continue
        check(rc, "vptr_norm_act_bwd_deferred" if deferred else "vptr_norm_act_bwd")
        if p16:
            assert rel(ops.p16_decode(dx), ref["dx"]) < TOLP16
        else:
            assert rel(dx, ref["dx"]) < TOLG
        if deferred:
            assert part.shape[0] == nparts
            sums = part.double().sum(0).cpu()
            assert rel(sums[0], ref["dw"]) < TOLG and rel(sums[1], ref["db"]) < TOLG
        else:
            assert rel(dwd, dw0.double() + ref["dw"]) < TOLG and rel(dbd, db0.double() + ref["db"]) < TOLG


def test_norm_act_bwd_deferred_rejects_short_clips(dev, abi):
    """63 frames: no deferred variant (the partial count is 0), the call returns an error and launches nothing"""
    lib, ptr, stream = abi.lib, abi.ptr, abi.stream
    frames, HW, Fc = 63, 16, 32
    rows, E = frames * HW, HW * Fc
    x, dy, w, b = rn((rows, Fc), 1).to(dev), rn((rows, Fc), 2).to(dev), rn((HW, Fc), 3).to(dev), rn((HW, Fc), 4).to(dev)
    mean, rstd = torch.zeros(frames, device=dev), torch.ones(frames, device=dev)
    dx, part = torch.full((rows, Fc), NAN, device=dev), torch.full((16, 2, E), NAN, device=dev)
    scratch = torch.empty(2 * frames * (1 + 4 * cdiv(E // 4, 256)), device=dev)
    assert lib.vptr_norm_act_bwd_partials(rows, Fc, HW, 0) == 0
    rc = lib.vptr_norm_act_bwd_deferred(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(dx), ptr(scratch), rows, Fc, HW, 1, 0, 0.0, None, 0, None, 1,
                                        1, 0, ptr(part), stream())
    assert rc < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(part).all())


# ------------------------------------------------------- 4. depthwise weight gradient: vptr_dwconv3x3_bwd_xh and vptr_dwconv3x3_bwd launch classes
# id -> (fp16 operand?, frames, H, W, F, deterministic)
DW_CASES = {
    "xh_6x8x8x192": (True, 6, 8, 8, 192, False),           # frames < 64: one frame per block, dwconv_bwd_w_kernel<true, true, 32>
    "xh_70x4x4x64": (True, 70, 4, 4, 64, False),           # the step's class: <true, true, 16>, 8 frames per block, a tail block of 6
    "xh_69x8x6x48": (True, 69, 8, 6, 48, False),           # 12 channel quads < 16: a partial channel block; tail of 5 frames over 4 frame lanes; W / 2 = 3
    "xh_64x16x16x32": (True, 64, 16, 16, 32, False),       # W = 16: two passes of the x loop (8 columns per pass)
    "xh_512x2x2x2048": (True, 512, 2, 2, 2048, False),     # 16 x 64 = 1024 blocks: not narrow -> <true, true, 32> with 8 frames per block; W = 2: one live x lane of four
    "f32_512x2x2x2048": (False, 512, 2, 2, 2048, False),   # the same through the fp32 operand: <true, false, 32>
    "f32_66x3x5x16": (False, 66, 3, 5, 16, False),         # odd W with frames >= 64: the single-column form <false>, 8 frames per block, tail of 2
    "xh_70x4x4x64_det": (True, 70, 4, 4, 64, True),        # deterministic: ONE block walks all 70 frames
    "f32_66x3x5x16_det": (False, 66, 3, 5, 16, True),
}


@pytest.mark.parametrize("case", sorted(DW_CASES))
def test_dwconv3x3_bwd_weight_classes(ops, dev, abi, case):
    """dx, dw9 (tap-major [9, F]) and db vs fp64 F.conv2d(groups = F, padding = 1) + autograd; dw9 / db are added onto non-zero start values.
    For the fp16 operand the test rounds x itself and the reference reads the ROUNDED values, so the fp16 rounding is no part of the error"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    xh, frames, H, W, Fc, det = DW_CASES[case]
    rows = frames * H * W
    seed = 700 + 10 * sorted(DW_CASES).index(case)
    x, dy, w = rn((rows, Fc), seed), rn((rows, Fc), seed + 1), rn((Fc, 1, 3, 3), seed + 2, 0.3)
    dw0, db0 = rn((9, Fc), seed + 3, 0.5), rn((Fc,), seed + 4, 0.5)
    x_op = x.half() if xh else x

    def nchw(t):
        return t.double().reshape(frames, H, W, Fc).permute(0, 3, 1, 2)
    xr, wr = nchw(x_op).clone().requires_grad_(True), w.double().requires_grad_(True)
    br = torch.zeros(Fc, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, wr, br, padding=1, groups=Fc).backward(nchw(dy))
    dx_ref = xr.grad.permute(0, 2, 3, 1).reshape(rows, Fc)
    dw_ref, db_ref = dw0.double() + wr.grad.reshape(Fc, 9).t(), db0.double() + br.grad

    xd, dyd, w9 = x_op.to(dev), dy.to(dev), w.reshape(Fc, 9).t().contiguous().to(dev)
    dx, dw9, db = torch.full((rows, Fc), NAN, device=dev), dw0.clone().to(dev), db0.clone().to(dev)
    with deterministic(ops, det):
        fn = lib.vptr_dwconv3x3_bwd_xh if xh else lib.vptr_dwconv3x3_bwd
        check(fn(ptr(dyd), ptr(xd), ptr(w9), ptr(dx), ptr(dw9), ptr(db), frames, H, W, Fc, stream()), "vptr_dwconv3x3_bwd_xh" if xh else "vptr_dwconv3x3_bwd")
    assert rel(dx, dx_ref) < TOLG
    assert rel(dw9, dw_ref) < TOLG
    assert rel(db, db_ref) < TOLG


def test_dwconv3x3_bwd_xh_rejects_odd_width(dev, abi):
    lib, ptr, stream = abi.lib, abi.ptr, abi.stream
    frames, H, W, Fc = 4, 3, 5, 16
    rows = frames * H * W
    x, dy, w9 = rn((rows, Fc), 1).half().to(dev), rn((rows, Fc), 2).to(dev), rn((9, Fc), 3).to(dev)
    dx, dw9, db = torch.full((rows, Fc), NAN, device=dev), torch.zeros((9, Fc), device=dev), torch.zeros(Fc, device=dev)
    assert lib.vptr_dwconv3x3_bwd_xh(ptr(dy), ptr(x), ptr(w9), ptr(dx), ptr(dw9), ptr(db), frames, H, W, Fc, stream()) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and float(dw9.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- 5. autograd + slab + end-of-backward flush
def test_slab_backed_deferred_gradients_through_ops(ops, dev, monkeypatch):
    """parameters sliced out of a registered flat slab: ops.layernorm (4112 x 528, applied TWICE in one graph -> two reduce entries share their
    destinations, unique_dst = 0) and ops.norm_act("ln") on 64 frames take the deferred kernels, the end-of-backward callback empties the
    reduce queue, autograd gets no parameter gradient, and after two forward + backward passes the gradient slab holds the fp64 gradients of
    both passes and both applications"""
    C, HW, Fc, frames, rows = 528, 16, 32, 64, 4112
    E = HW * Fc
    offs = {"gamma": (0, C), "beta": (C, C), "w": (2 * C, E), "b": (2 * C + E, E)}
    total = 2 * C + 2 * E + 32
    host = {"gamma": rn((C,), 801).abs() + 0.5, "beta": rn((C,), 802, 0.3), "w": rn((E,), 803).abs() + 0.5, "b": rn((E,), 804, 0.3)}
    x, xn = rn((rows, C), 805, 2.0) + 0.3, rn((frames * HW, Fc), 806, 2.0) + 0.3
    cots = [(rn((rows, C), 807 + 2 * i), rn((frames * HW, Fc), 808 + 2 * i)) for i in range(2)]

    # fp64 reference: both passes summed
    pr = {k: v.double().requires_grad_(True) for k, v in host.items()}
    xr = x.double().requires_grad_(True)
    for g1, g2 in cots:
        h = F.layer_norm(F.layer_norm(xr, (C,), pr["gamma"], pr["beta"], 1e-5), (C,), pr["gamma"], pr["beta"], 1e-5)
        z = F.gelu(F.layer_norm(xn.double().view(frames, HW, Fc), (HW, Fc), pr["w"].view(HW, Fc), pr["b"].view(HW, Fc), 1e-5))
        ((h * g1.double()).sum() + (z.reshape(-1, Fc) * g2.double()).sum()).backward()

    calls = {"norm": 0, "convffn": 0}

    def counted(mod, key):
        orig = mod.defer_partial_reduce

        def wrapper(*a, **k):
            calls[key] += 1
            return orig(*a, **k)
        monkeypatch.setattr(mod, "defer_partial_reduce", wrapper)
    counted(ops.norm, "norm")
    counted(ops.convffn, "convffn")

    flat, grad = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    for k, (o, n) in offs.items():
        flat[o:o + n].copy_(host[k])
    par = {k: flat[o:o + n].requires_grad_(True) for k, (o, n) in offs.items()}
    xd, xnd = x.to(dev).requires_grad_(True), xn.to(dev)
    assert ops.config.defer_ln_param_grads and not ops.config.deterministic
    ops.register_flat_slab(flat, grad)
    try:
        assert ops.flat_grad_for(par["gamma"]).data_ptr() == grad.data_ptr()
        for i, (g1, g2) in enumerate(cots):
            h = ops.layernorm(ops.layernorm(xd, par["gamma"], par["beta"]), par["gamma"], par["beta"])
            z = ops.norm_act(xnd, par["w"].view(HW, Fc), par["b"].view(HW, Fc), "ln", HW, True)
            ((h * g1.to(dev)).sum() + (z * g2.to(dev)).sum()).backward()
            assert calls == {"norm": 2 * (i + 1), "convffn": i + 1}
            assert len(ops.wgrad._reduce_q) == 0
            assert all(t.grad is None for t in par.values())
        torch.cuda.synchronize()
        got = grad.cpu()
        for k, (o, n) in offs.items():
            assert rel(got[o:o + n], pr[k].grad) < TOLG, k
        assert float(got[2 * C + 2 * E:].abs().max()) == 0.0
        assert rel(xd.grad, xr.grad) < TOLG
    finally:
        ops.unregister_flat_slab(flat)
        ops.discard_wgrads()
    assert ops.flat_grad_for(par["gamma"]) is None and ops.flat_grad_for(par["w"]) is None
