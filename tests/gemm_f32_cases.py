"""Case runner of tests/test_01c_gemm_f32_abi_gpu.py: the fp32-staged MFMA GEMM (vptr_gemm with a_mode 0 / 1 / 2 and b_mode 0 / 1; csrc/gemm.hip,
csrc/gemm_shared.h) called through the C ABI in each of its launch classes -- the pipelined loop vptr_gemm_kernel_p ("P") and the single-image
loop vptr_gemm_kernel ("S", grids of at least 384 workgroups) x the four epilogue functions x NFN 4 / 8 / 11 x the operand stagers -- and
compared PER ELEMENT with the fp64 product of the split operands.

The runner talks to a BACKEND exactly as tests/gemm_p16_cases.py does (gemm(d), last_error(), mm64(a, b), sync(), dev, dry); the guarded
buffers (Buf), act64 and the row / column rule are that module's.  `EmuBackend` below emulates the call on the CPU (tests/test_cpu.py
runs every case against it and against named MUTATIONS of it, each of which has to make a case fail).

Operands.  A ~ N(0, 1), B ~ N(0, 1 / (K nseg)), so the accumulator is of order 1.  split(x): hi = bf16_rne(x), lo = bf16_rne(x - hi).  The 2^-18
of the accumulator bar rests on |lo| <= 2^-9 |x|, while round-to-nearest only gives |x - hi| <= 2^-8 2^floor(log2 |x|) (up to 2^-8 |x| just above a
power of two; at K = 4 nothing averages that out).  The operands are therefore drawn as x = hi(g) + (g - hi(g)) / 2 from Gaussian g: hi(x) = hi(g),
|x - hi| <= 2^-9 |x| holds for every element, and lo keeps all eight bits of its significand (operand()).
Bars.  ref = fp64 product of hi + lo of both operands (precision 3) or of hi alone (precision 1), S_ij = sum_k |a_ik| |b_jk| of the same
operands, u = 2^-23, nk = number of 32-wide K-steps of all splits, nseg = K segments.
  accumulator   precision 3: (2^-18 + (32 + 3 nk nseg) u) S, the bar of gemm_p16_cases.py; precision 1: (32 + nk nseg) u S (no dropped lo . lo
                term, one MFMA per step).
  epilogue      as in gemm_p16_cases.py: the accumulator bar times the first-order gains, plus u times the magnitudes of the intermediates.
  atomics       a launch that accumulates (atomic = 1 or split-K) performs `adds` = number of splits read-modify-write additions per element, in
                any order; each rounds a running sum that is at most |D0| + |alpha| S + |bias| + |residual|: + adds u times that.
  rows, columns against the fp64 product of the RAW fp32 operands pushed through the same epilogue: rel-L2 of every row and every column below
                TOL3 = 3e-5 (precision 3) / TOL1 = 1.5e-2 (precision 1), small norms by the rule of gemm_p16_cases.rowcol.  The two
                fp64 references of a case (split and raw operands) must themselves be less than a third of that apart in every row and
                column: a property of the seeded data (a one-element column with a cancelled sum shows 2^-17 S / |ref|), asserted before
                the kernel's output is looked at; a case that misses it gets another `seed`.
  a_rowsum      the kernel sums the raw fp32 operand: against the fp64 row sums of the split operand the bar is
                |alpha| (2^-17 + (2 nk + 8 + splits) u) sum_k |a| + splits u |initial value| (2^-17: x - (hi + lo); 2 nk additions per thread,
                3 shuffles, the wave pair, the scaling and one atomic addition per split).
Kinks (ReLU / LeakyReLU / act_after within their own bar of zero) are left out of the value check only, at most KINK_SHARE of a case.  Dropped
elements are their residual bit for bit, +0 without one."""
import torch
import torch.nn.functional as F

from gemm_p16_cases import (DROP_P, GELU, IN_NAN, KINK_SHARE, LRELU, NONE, OUT_CANARY, RELU, SEED, SITE, TOL3, U, Buf, DryBackend, act64, f32,
                            fields_of, rn, rowcol)
from helpers import drop_scale_emu, gemm_f32_class, gemm_f32_plan, margin, split_bf16

TOL1 = 1.5e-2
ACC_CANARY = 0x3F800000          # 1.0f around every buffer the call ACCUMULATES into: an atomic addition to a NaN canary would leave it a NaN
BIG = 128 * 383 + 5              # rows of 384 row tiles: the smallest one-column-tile problem that takes the single-image loop
ZERO, REFLECT, REPLICATE = 0, 1, 2
RS_DIV, RS_MOD = 7, 5
FULL = dict(cs=1, act=GELU, dpre=1, rs=1, drop=1, res=1, after=1)      # every epilogue option of include/vptr_hip.h at once

LOOPS_EPIS = [("P", "rows", n) for n in (4, 8, 11)] + [("P", "frag", n) for n in (4, 8, 11)] + [("S", "rows_halves", 11)] + \
             [("S", "serial", n) for n in (4, 8, 11)]
MODE_PAIRS = [("kc", "kc"), ("kc", "ks"), ("ks2", "ks"), ("ks2", "kc"), ("conv", "kc")]


def conv(Fr, IH, IW, Cin, KH, KW, stride, pad, mode=ZERO, tr=0, outpad=0):
    if tr:
        OH, OW = (IH - 1) * stride - 2 * pad + KH + outpad, (IW - 1) * stride - 2 * pad + KW + outpad
    else:
        OH, OW = (IH + 2 * pad - KH) // stride + 1, (IW + 2 * pad - KW) // stride + 1
    return dict(Fr=Fr, IH=IH, IW=IW, Cin=Cin, KH=KH, KW=KW, stride=stride, pad=pad, mode=mode, tr=tr, outpad=outpad, OH=OH, OW=OW)


def _c(cls, M=129, N=64, K=68, am=0, bm=0, **kw):
    return dict(cls=cls, M=M, N=N, K=K, am=am, bm=bm, **kw)


def _cv(cls, N, cg, **kw):
    return dict(cls=cls, M=cg["Fr"] * cg["OH"] * cg["OW"], N=N, K=cg["KH"] * cg["KW"] * cg["Cin"], am=2, bm=0, conv=cg, **kw)


# name -> case.  cls "loop/epilogue/NFN" is the class the case must reach (asserted against helpers.gemm_f32_class when it is built); `grid`,
# where given, the number of workgroups it must launch.  Defaults: bias, alpha = 0.75, precision 3, every pitch wider than its row.
SPEC = {}
# -- k-contiguous x k-contiguous, pipelined loop: K against the prefetch depth of 2 (1, 2, 3 steps, with and without a tail), M, N, the grid
for _K in (4, 32, 36, 64, 68, 96, 100):
    SPEC["kc_K%d" % _K] = _c("P/rows/4", K=_K, grid=2)
for _M, _g in ((1, 1), (127, 1), (128, 1), (257, 3)):
    SPEC["kc_M%d" % _M] = _c("P/frag/4", M=_M, N=50, K=36, grid=_g)
SPEC["kc_M1"].update(pos=1, bias=0)      # a column is ONE element: operands of one sign, so that no sum cancels (S = |ref|, see the rows / columns rule)
SPEC.update({
    "kc_N3": _c("P/frag/4", N=3, K=36, seed=70), "kc_N4": _c("P/rows/4", M=13 * 128 - 100, N=4, K=36, grid=13), "kc_N128": _c("P/rows/8", N=128),
    "kc_N176": _c("P/rows/11", N=176), "kc_N180": _c("P/rows/4", M=257, N=180, grid=9), "kc_N200": _c("P/rows/8", N=200, grid=4),
    "kc_N340": _c("P/rows/11", N=340, grid=4), "kc_grid7": _c("P/rows/4", M=7 * 128 - 3, K=36, grid=7), "kc_tight": _c("P/rows/4", M=257, N=180, tight=1),
    "kc_plain": _c("P/rows/8", N=200, alpha=1.0, res=1), "kc_nobias": _c("P/rows/4", bias=0, alpha=0.0),
    # the full option set in the two epilogue functions of the pipelined loop, at each NFN
    "full_rows4": _c("P/rows/4", M=257, N=180, **FULL), "full_rows8": _c("P/rows/8", N=200, **FULL), "full_rows11": _c("P/rows/11", N=340, **FULL),
    "full_frag4": _c("P/frag/4", N=50, **FULL), "full_frag8": _c("P/frag/8", N=127, **FULL), "full_frag11": _c("P/frag/11", N=342, **FULL),
    "full_frag8_dshift": _c("P/frag/8", N=128, dshift=1, **FULL), "full_frag11_dshift": _c("P/frag/11", N=176, dshift=1, **FULL),
    "rows_relu_alias": _c("P/rows/4", act=RELU, res=1, alias=1, rs=1), "rows_lrelu_alpha0": _c("P/rows/8", N=128, act=LRELU, alpha=0.0, dpre=1),
    "frag_relu_alias": _c("P/frag/4", N=50, act=RELU, res=1, alias=1, rs=1), "frag_lrelu_alpha0": _c("P/frag/8", N=127, act=LRELU, alpha=0.0, dpre=1),
    "rows_drop_nores": _c("P/rows/4", act=LRELU, drop=1), "frag_drop_nores": _c("P/frag/4", N=50, act=LRELU, drop=1),
    "rows_after": _c("P/rows/11", N=176, res=1, after=1), "frag_after": _c("P/frag/11", N=342, res=1, after=1),
    # -- k-contiguous x k-strided
    "kcks_N64": _c("P/rows/4", bm=1, K=36), "kcks_N128": _c("P/rows/8", bm=1, N=128, K=100), "kcks_N176": _c("P/rows/11", bm=1, N=176),
    "kcks_N180": _c("P/rows/4", bm=1, M=257, N=180, **FULL), "kcks_N200": _c("P/rows/8", bm=1, N=200, K=32), "kcks_N340": _c("P/rows/11", bm=1, N=340, K=4),
    "kcks_dshift": _c("P/frag/8", bm=1, N=200, dshift=1, act=GELU, res=1),
    # -- k-strided x k-strided (weight gradients): any K, M % 4 == 0
    "ksks_K1": _c("P/rows/4", am=1, bm=1, M=4, K=1), "ksks_K2": _c("P/rows/4", am=1, bm=1, M=124, K=2), "ksks_K3": _c("P/rows/8", am=1, bm=1, M=132, N=128, K=3),
    "ksks_K31": _c("P/rows/11", am=1, bm=1, M=132, N=176, K=31), "ksks_K33": _c("P/rows/4", am=1, bm=1, M=260, N=180, K=33, grid=9),
    "ksks_K65": _c("P/rows/8", am=1, bm=1, M=132, N=200, K=65, **FULL), "ksks_K97_11": _c("P/rows/11", am=1, bm=1, M=124, N=340, K=97),
    # -- k-strided x k-contiguous
    "kskc_K36": _c("P/rows/4", am=1, M=132, K=36), "kskc_K100": _c("P/rows/8", am=1, M=260, N=200, K=100, **FULL), "kskc_N50": _c("P/frag/4", am=1, M=124, N=50, K=4),
    "kskc_N176": _c("P/rows/11", am=1, M=4, N=176, K=64),
    # -- split-K and atomics: D pre-initialised, bias and residual by the first split only
    "split2": _c("P/frag/4", K=100, split_k=2, res=1, grid=4), "split3": _c("P/frag/8", N=200, K=96, split_k=3, res=1, alpha=1.0, grid=12),
    "split7": _c("P/frag/4", K=100, split_k=7, res=1, grid=8), "split2_ksks": _c("P/frag/11", am=1, bm=1, M=132, N=176, K=65, split_k=2),
    "split2_kcks_tail": _c("P/frag/4", bm=1, K=68, split_k=2), "atomic1": _c("P/frag/4", atomic=1, res=1), "atomic1_11": _c("P/frag/11", N=340, atomic=1, alpha=1.0),
    # -- K segments (a tail step in every segment: K % 32 = 4, 16; none: 0) and batch members
    "kseg2_K36": _c("P/rows/4", K=36, ksegs=2, res=1), "kseg3_K48": _c("P/rows/8", N=200, K=48, ksegs=3, **FULL), "kseg2_K64": _c("P/rows/11", N=176, K=64, ksegs=2),
    "kseg3_ksks": _c("P/rows/4", am=1, bm=1, M=132, K=33, ksegs=3), "kseg3_frag": _c("P/frag/4", N=50, K=36, ksegs=3, res=1),
    "batch2": _c("P/rows/4", batch=2, alphas=(1.5, -0.75), nobias=(1,), grid=4), "batch3": _c("P/rows/8", N=200, K=36, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(0,), grid=12),
    "batch3_frag": _c("P/frag/4", N=50, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(2,), act=GELU, drop=1),
    "batch2_ksks": _c("P/rows/11", am=1, bm=1, M=132, N=176, K=33, batch=2, alphas=(0.5, 2.0), nobias=()),
    # -- a_rowsum (pipelined kernels only, k-strided A)
    "rowsum_big": _c("P/frag/11", am=1, bm=1, M=1024, N=528, K=512, split_k=16, rowsum=1, alpha=1.0, grid=384),
    "rowsum_tiles": _c("P/rows/4", am=1, bm=1, M=132, N=180, K=65, rowsum=1, alpha=0.5, grid=6),
    "rowsum_split": _c("P/frag/4", am=1, M=260, K=68, split_k=2, rowsum=1, rowsum_init=1, alpha=-1.5, grid=6),
    # -- precision 1 in the pipelined loop: every stager
    "p1_kckc": _c("P/rows/4", K=100, prec=1, act=GELU, res=1), "p1_ksks": _c("P/rows/8", am=1, bm=1, M=132, N=200, K=65, prec=1),
    "p1_kskc_frag": _c("P/frag/11", am=1, M=132, N=342, K=36, prec=1), "p1_kcks": _c("P/rows/11", bm=1, N=176, K=68, prec=1),
    # -- implicit-GEMM convolution, forward: 3x3 at stride 1 / 2 under every padding, 4x4 stride 2, 1x1, the smallest reflectable maps
    "conv3s1_zero": _cv("P/rows/4", 8, conv(2, 5, 7, 4, 3, 3, 1, 1, ZERO)), "conv3s1_reflect": _cv("P/rows/4", 16, conv(3, 6, 5, 12, 3, 3, 1, 1, REFLECT), **FULL),
    "conv3s1_replicate": _cv("P/frag/4", 6, conv(2, 5, 7, 4, 3, 3, 1, 1, REPLICATE)), "conv3s2_zero": _cv("P/rows/4", 8, conv(2, 7, 6, 12, 3, 3, 2, 1, ZERO)),
    "conv3s2_reflect": _cv("P/rows/4", 8, conv(2, 7, 6, 4, 3, 3, 2, 1, REFLECT)), "conv3s2_replicate": _cv("P/rows/4", 8, conv(2, 6, 7, 4, 3, 3, 2, 1, REPLICATE)),
    "conv4s2": _cv("P/rows/8", 128, conv(2, 8, 6, 12, 4, 4, 2, 1, ZERO), act=LRELU), "conv1x1": _cv("P/rows/11", 176, conv(3, 5, 9, 48, 1, 1, 1, 0, ZERO)),
    "conv_map2x3": _cv("P/rows/4", 8, conv(3, 2, 3, 4, 3, 3, 1, 1, REFLECT)), "conv_map3x2": _cv("P/rows/4", 8, conv(3, 3, 2, 4, 3, 3, 1, 1, REFLECT)),
    "conv_frames": _cv("P/rows/4", 8, conv(3, 10, 9, 4, 3, 3, 1, 1, REFLECT), grid=3), "conv_cin48": _cv("P/rows/8", 200, conv(2, 6, 5, 48, 3, 3, 1, 1, REPLICATE), cs=1, act=RELU, res=1, after=1),
    # transposed (gather form): stride 2 with OH = 2 IH, stride 1 (the data gradient of a stride-1 layer), stride 3 (the `/ stride` branch)
    "convT_s2": _cv("P/rows/4", 8, conv(2, 5, 4, 12, 3, 3, 2, 1, tr=1, outpad=1), grid=2), "convT_s1": _cv("P/rows/4", 8, conv(2, 5, 7, 4, 3, 3, 1, 1, tr=1)),
    "convT_s3": _cv("P/rows/4", 8, conv(2, 4, 3, 4, 3, 3, 3, 1, tr=1)), "convT_s2_k4": _cv("P/frag/4", 6, conv(2, 4, 5, 4, 4, 4, 2, 1, tr=1)),
    "conv_split2": _cv("P/frag/4", 8, conv(2, 6, 5, 12, 3, 3, 1, 1, REFLECT), split_k=2), "p1_conv": _cv("P/rows/4", 8, conv(2, 7, 6, 12, 3, 3, 2, 1, REFLECT), prec=1),
    # the four parity classes of ConvTranspose2d(3x3, stride 2, pad 1, output_padding 1) through d_row_w / d_row_off into one NHWC output
    "subpixel_c12": dict(cls="P/frag/4", sub=dict(Fr=2, IH=3, IW=5, Cin=4, Cout=12), cs=1, act=RELU),
    "subpixel_c6": dict(cls="P/frag/4", sub=dict(Fr=3, IH=6, IW=9, Cin=12, Cout=6), grid=2),
    # -- the single-image loop: grids of at least 384 workgroups
    "S_kc_K36": _c("S/serial/4", M=BIG + 128, N=16, K=36, grid=385), "S_kc_K4": _c("S/serial/4", M=BIG, N=16, K=4), "S_kc_K100": _c("S/serial/4", M=BIG, N=16, K=100, **FULL),
    "S_full_serial4": _c("S/serial/4", M=BIG, N=50, K=36, **FULL), "S_full_serial8": _c("S/serial/8", M=BIG, N=127, K=36, **FULL),
    "S_full_serial11": _c("S/serial/11", M=BIG, N=176, K=36, dshift=1, **FULL), "S_full_rh11": _c("S/rows_halves/11", M=BIG, N=176, K=36, **FULL),
    "S_rh11_kcks": _c("S/rows_halves/11", M=192 * 128 - 7, N=352, K=68, bm=1, act=LRELU, drop=1, grid=384),
    "S_rh11_relu_alias": _c("S/rows_halves/11", M=BIG, N=176, K=64, alpha=0.0, act=RELU, res=1, alias=1, rs=1),
    "S_serial_lrelu_nores": _c("S/serial/4", M=BIG, N=16, K=32, act=LRELU, drop=1), "S_serial_alias": _c("S/serial/4", M=BIG, N=16, K=64, alpha=0.0, act=RELU, res=1, alias=1, rs=1),
    "S_serial_drop_n16": _c("S/serial/4", M=BIG, N=16, K=36, drop=1, alpha=-1.5),
    "S_kcks_p1": _c("S/serial/4", M=BIG, N=64, K=36, bm=1, prec=1), "S_kcks_8": _c("S/serial/8", M=BIG, N=128, K=36, bm=1, res=1),
    "S_split_ksks11": _c("S/serial/11", am=1, bm=1, M=1024, N=528, K=512, split_k=16, grid=384), "S_split_ksks8": _c("S/serial/8", am=1, bm=1, M=2048, N=384, K=250, split_k=8, grid=384),
    "S_split_kskc4": _c("S/serial/4", am=1, M=6144, N=64, K=252, split_k=8, res=1, grid=384), "S_split_ksks4_p1": _c("S/serial/4", am=1, bm=1, M=6144, N=64, K=255, split_k=8, prec=1),
    "S_split_kskc11": _c("S/serial/11", am=1, M=1024, N=528, K=508, split_k=16, prec=1), "S_atomic_kskc8": _c("S/serial/8", am=1, M=BIG - 1, N=128, K=36, atomic=1),
    "S_kseg3_K36": _c("S/serial/4", M=BIG, N=16, K=36, ksegs=3, res=1), "S_kseg2_K48": _c("S/serial/4", M=BIG, N=16, K=48, ksegs=2), "S_kseg3_K32": _c("S/serial/4", M=BIG, N=16, K=32, ksegs=3),
    "S_batch3": _c("S/serial/4", M=128 * 128 + 5, N=16, K=36, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(1,), grid=387),
    "S_conv": _cv("S/serial/4", 32, conv(3, 128, 128, 4, 3, 3, 1, 1, REFLECT), grid=384, **FULL), "S_conv_p1": _cv("S/serial/4", 32, conv(3, 128, 128, 4, 3, 3, 1, 1, ZERO), prec=1),
    "S_convT": _cv("S/serial/4", 8, conv(3, 64, 64, 4, 3, 3, 2, 1, tr=1, outpad=1), grid=384),
})
CASES = list(SPEC)
REJECTS = list(range(0, 31))     # 0: the null descriptor; 1 .. 30: one per VPTR_CHECK of vptr_gemm that fp32-staged operands can reach, in source
                                 # order (helpers.gemm_f32_class)


def operand(shape, seed, scale=1.0):
    """Gaussian values whose hi / lo split satisfies the premise of the accumulator bar, |x - bf16(x)| <= 2^-9 |x| (see the module docstring)"""
    g = rn(shape, seed, scale)
    hi = g.to(torch.bfloat16).float()
    x = hi + (g - hi) * 0.5
    assert bool(((x - x.to(torch.bfloat16).float()).abs() <= 2.0 ** -9 * x.abs()).all())
    return x


def cls_of(name):
    loop, epi, nfn = SPEC[name]["cls"].split("/")
    return loop, epi, int(nfn)


# ------------------------------------------------------------------------------------------------------------------ operands
def split_f32(x):
    """helpers.split_bf16 (split2 of csrc/gemm_shared.h) as fp32: (hi, lo)"""
    hi, lo = split_bf16(x)
    return hi.float(), lo.float()


def map_coord(o, kk, I, cg, mut=None):
    """StageConv::map_coord on int64 tensors: the source coordinate, -1 where the tap contributes zero"""
    st, pad = cg["stride"], cg["pad"]
    if cg["tr"]:
        num = o + pad - kk
        q = torch.div(num, st, rounding_mode="trunc")
        ok = (num >= 0) & (q < I)
        if mut != "parity_dropped":
            ok = ok & (q * st == num)
        return torch.where(ok, q, torch.full_like(q, -1))
    c = o * st - pad + kk
    inside = (c >= 0) & (c < I)
    refl = torch.where(c < 0, -c - (1 if mut == "reflect_off_by_one" else 0), 2 * I - 2 - c)
    repl = torch.where(c < 0, torch.zeros_like(c), torch.full_like(c, I - 1))
    outv = torch.full_like(c, -1) if cg["mode"] == ZERO else (refl if cg["mode"] == REFLECT else repl)
    return torch.where(inside, c, outv)


def conv_gather(x, cg, M, mut=None):
    """the implicit-GEMM A matrix [M, KH KW Cin] of an NHWC image x [Fr IH IW, Cin], as StageConv gathers it"""
    IH, IW, Cin, OH, OW, KH, KW = (cg[k] for k in ("IH", "IW", "Cin", "OH", "OW", "KH", "KW"))
    m = torch.arange(M)
    f, rem = m // (OH * OW), m % (OH * OW)
    oy, ox = rem // OW, rem % OW
    ky, kx = torch.arange(KH * KW) // KW, torch.arange(KH * KW) % KW
    iy = map_coord(oy[:, None], ky[None, :], IH, cg, mut)
    ix = map_coord(ox[:, None], kx[None, :], IW, cg, mut)
    ok = (iy >= 0) & (ix >= 0)
    pix = (f[:, None] * IH + iy.clamp_min(0)) * IW + ix.clamp_min(0)
    g = x[pix.reshape(-1)].reshape(M, KH * KW, Cin) * ok[:, :, None]
    return g.reshape(M, KH * KW * Cin)


def conv64(x, w, cg):
    """fp64 torch convolution of the NHWC image x [Fr IH IW, Cin] with B [N, (ky, kx, ci)] -> [Fr OH OW, N]"""
    Fr, IH, IW, Cin, KH, KW = (cg[k] for k in ("Fr", "IH", "IW", "Cin", "KH", "KW"))
    N = w.shape[0]
    xi = x.double().reshape(Fr, IH, IW, Cin).permute(0, 3, 1, 2)
    wk = w.double().reshape(N, KH, KW, Cin)
    if cg["tr"]:
        y = F.conv_transpose2d(xi, wk.permute(3, 0, 1, 2), stride=cg["stride"], padding=cg["pad"], output_padding=cg["outpad"])
    else:
        p = cg["pad"]
        if p:
            xi = F.pad(xi, (p, p, p, p), mode={ZERO: "constant", REFLECT: "reflect", REPLICATE: "replicate"}[cg["mode"]])
        y = F.conv2d(xi, wk.permute(0, 3, 1, 2), stride=cg["stride"])
    assert y.shape[2:] == (cg["OH"], cg["OW"]), (y.shape, cg)
    return y.permute(0, 2, 3, 1).reshape(-1, N)


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
MUTATIONS = ("a_tail_unmasked", "reflect_off_by_one", "parity_dropped", "seg3_reads_seg2", "d_row_off_ignored", "bias_every_split", "rowsum_clamped_rows",
             "drop_index_ldd", "lo_dropped")


class EmuBackend:
    """CPU emulation of vptr_gemm on fp32-staged operands: the operands gathered as the stagers gather them (k-contiguous, k-strided, the NHWC
    gather with its three paddings and the transposed form), split into bf16 hi / lo, al . bh + ah . bl + ah . bh per 32-wide K-step in fp32 and in
    that order (precision 1: ah . bh), K segments and splits in order, bias / residual by the first split only, batch members, the output row
    map, a_rowsum, the epilogue in fp32 in the order of include/vptr_hip.h, and the launcher's refusals (helpers.gemm_f32_class)."""
    dev, dry = "cpu", False

    def __init__(self, mut=None):
        assert mut is None or mut in MUTATIONS
        self.mut, self.err = mut, ""

    def sync(self):
        pass

    def last_error(self):
        return self.err

    def mm64(self, a, b):
        return a.double() @ b.double().t()

    def _operand(self, d, P, mode, rows, K, ld):
        if mode == 2:
            cg = dict(Fr=0, IH=d["conv_IH"], IW=d["conv_IW"], Cin=d["conv_Cin"], OH=d["conv_OH"], OW=d["conv_OW"], KH=d["conv_KH"], KW=d["conv_KW"],
                      stride=d["conv_stride"], pad=d["conv_pad"], mode=d.get("conv_pad_mode", 0), tr=d.get("conv_transposed", 0))
            frames = -(-rows // (cg["OH"] * cg["OW"]))
            x = P.as_strided((frames * cg["IH"] * cg["IW"], cg["Cin"]), (cg["Cin"], 1))
            return conv_gather(x, cg, rows, self.mut)
        if mode == 1:
            return P.as_strided((K, rows), (ld, 1)).t()
        return P.as_strided((rows, K), (ld, 1))

    def _acc(self, A, B, kbeg, kend, prec, am, bm):
        """the accumulator of K-steps [kbeg, kend) of one segment, continued by the caller"""
        acc = 0
        for lo in range(kbeg, kend, 32):
            hi = min(lo + 32, kend)
            a, b = A[:, lo:hi], B[:, lo:hi]
            if hi - lo < 32 and self.mut == "a_tail_unmasked":
                # the kernel zeroes the K tail in A ONLY (KMASK); B's tail keeps its clamped loads.  Without A's mask the products of the two
                # clamped tails, as they stand in the registers, are accumulated
                k = torch.arange(lo, lo + 32)
                ka = torch.where(k < kend, k, (kend - 1) * torch.ones_like(k) if am == 1 else kend - 4 + k % 4)
                kb = torch.where(k < kend, k, (kend - 1) * torch.ones_like(k) if bm == 1 else kend - 4 + k % 4)
                a, b = A[:, ka], B[:, kb]
            ah, al = split_f32(a)
            bh, bl = split_f32(b)
            if self.mut == "lo_dropped":
                al = torch.zeros_like(al)
            if prec == 3:
                acc = acc + al @ bh.t()
                acc = acc + ah @ bl.t()
            acc = acc + ah @ bh.t()
        return acc

    def gemm(self, d):
        if d is None:
            self.err = "emulation: null descriptor"
            return -1
        cls = gemm_f32_class(fields_of(d))
        if cls[0] == "refuse":
            self.err = "emulation: refused by check %d" % cls[1]
            return -1
        g = lambda k, dflt=0: d[k] if d.get(k) is not None else dflt
        M, N, K, am, bm, prec, mut = d["M"], d["N"], d["K"], g("a_mode"), g("b_mode"), d["precision"], self.mut
        lda, ldb, ldd, ldr = g("lda"), g("ldb"), g("ldd"), g("ldr")
        plan = gemm_f32_plan(fields_of(d))
        batch, ksegs, splits, kc = plan["batch"], max(g("ksegs"), 1), plan["splits"], plan["k_chunk"]
        atomic = bool(g("atomic")) or (batch == 1 and splits > 1)
        act, p = g("act"), f32(g("dropout_p"))
        rows, cols = torch.arange(M), torch.arange(N)
        w, off = g("d_row_w"), (0 if mut == "d_row_off_ignored" else g("d_row_off"))
        drow = rows + w * (rows // w) + off if w > 0 else rows
        one = lambda a: torch.tensor(a if a != 0 else 1.0, dtype=torch.float32)
        for m in range(batch):
            sfx = "" if m == 0 else "_x%d" % m
            bias, alpha = d.get("bias" + sfx), one(g("alpha" + sfx))
            segs = [(d["A"], d["B"]), (d.get("A_x1"), d.get("B_x1")), (d.get("A_x2"), d.get("B_x2"))][:ksegs] if ksegs > 1 else [(d["A" + sfx], d["B" + sfx])]
            if mut == "seg3_reads_seg2" and ksegs == 3:
                segs[2] = segs[1]
            ops = [(self._operand(d, Ap, am, M, K, lda), self._operand(d, Bp, bm, N, K, ldb)) for Ap, Bp in segs]
            Dm = d["D" + sfx].as_strided((int(drow.max()) + 1, N), (ldd, 1))
            for s in range(splits):
                kbeg, kend = s * kc, min(K, s * kc + kc)
                v = 0
                for A, B in ops:
                    v = v + self._acc(A, B, kbeg, kend, prec, am, bm)
                first = s == 0 or mut == "bias_every_split"
                if d.get("colscale") is not None:
                    v = v * d["colscale"][:N]
                if bias is not None and first:
                    v = v + bias[:N]
                v = v * alpha
                if d.get("Dpre") is not None:
                    d["Dpre"].as_strided((M, N), (ldd, 1)).copy_(v)
                t = act64(v, act).float()
                if d.get("rowscale") is not None:
                    t = t * d["rowscale"][(rows // d["rs_div"]) % d["rs_mod"]][:, None]
                if p > 0:
                    assert (int(d["seed_dev"][0]), g("site"), p) == (SEED, SITE, f32(DROP_P))
                    t = t * keep_scale(M, N, ldd if mut == "drop_index_ldd" else None)
                t = t + (d["residual"].as_strided((M, N), (ldr, 1)).clone() if d.get("residual") is not None and first else 0.0)
                if g("act_after"):
                    t = torch.relu(t)
                Dm[drow] = Dm[drow] + t if atomic else t
                if d.get("a_rowsum") is not None:
                    rs = ops[0][0][:, kbeg:kend].sum(1) * one(g("alpha"))
                    d["a_rowsum"][:M] += rs
                    if mut == "rowsum_clamped_rows" and M % 128:     # the rows of the clamped out blocks: copies of the last four rows
                        pad = min(128 - M % 128, 32)
                        d["a_rowsum"][M:M + pad] += rs[M - 4:].repeat(pad // 4 + 1)[:pad]
        return 0


# ------------------------------------------------------------------------------------------------------------------ building a call
def _pitches(o, M, N, K):
    tight = o.get("tight")
    lda = (K if o["am"] == 0 else M) + (0 if tight else 8)
    ldb = (K + (0 if tight else 12)) if o["bm"] == 0 else (N + (0 if tight else 4))
    if o["am"] == 0 and lda % 4:
        lda += 4 - lda % 4
    ldd = N if tight else (N + 8 if N % 4 == 0 else N + 5)
    ldr = N if tight else (N + 4 if N % 4 == 0 else N + 3)
    return lda, ldb, ldd, ldr


def build(be, name):
    """the descriptors of a case (one; four for the sub-pixel form) with all their buffers: dict calls, cls, outs, inputs, o"""
    o = dict(am=0, bm=0, **SPEC[name]) if "sub" in SPEC[name] else SPEC[name]
    if "sub" in o:
        return _build_subpixel(be, name, o)
    dry, seed0 = be.dry, o.get("seed", 1000 * (CASES.index(name) + 1))
    M, N, K, am, bm, prec = o["M"], o["N"], o["K"], o["am"], o["bm"], o.get("prec", 3)
    lda, ldb, ldd, ldr = _pitches(o, M, N, K)
    if o.get("alias"):
        ldr = ldd
    batch, ksegs, splits_in = o.get("batch", 1), o.get("ksegs", 1), o.get("split_k", 1)
    cg = o.get("conv")
    d = dict(M=M, N=N, K=K, lda=0 if am == 2 else lda, ldb=ldb, ldd=ldd, a_mode=am, b_mode=bm, precision=prec, split_k=splits_in, alpha=o.get("alpha", 0.75),
             act=o.get("act", NONE))
    if cg:
        d.update(conv_IH=cg["IH"], conv_IW=cg["IW"], conv_Cin=cg["Cin"], conv_OH=cg["OH"], conv_OW=cg["OW"], conv_KH=cg["KH"], conv_KW=cg["KW"],
                 conv_stride=cg["stride"], conv_pad=cg["pad"], conv_pad_mode=cg["mode"], conv_transposed=cg["tr"])
    inputs, outs = [], []

    def inp(rows, cols, ld, data, **kw):
        b = Buf(be, rows, cols, ld, IN_NAN, None if dry else data, **kw)
        inputs.append(b)
        return b

    count = max(batch, ksegs)
    scale = (ksegs * K) ** -0.5
    prs = []
    for i in range(count):
        sfx = "" if i == 0 else "_x%d" % i
        if dry:
            Al = Bl = None
        else:
            Bl = operand((N, K), seed0 + 10 * i + 1, scale)
            Al = operand((cg["Fr"] * cg["IH"] * cg["IW"], cg["Cin"]) if cg else (M, K), seed0 + 10 * i)
        if o.get("pos") and not dry:
            Al, Bl = Al.abs(), Bl.abs()
        if cg:
            Ab = inp(cg["Fr"] * cg["IH"] * cg["IW"], cg["Cin"], cg["Cin"], lambda: Al)
        elif am == 1:
            Ab = inp(K, M, lda, lambda: Al.t())
        else:
            Ab = inp(M, K, lda, lambda: Al)
        Bb = inp(K, N, ldb, lambda: Bl.t()) if bm == 1 else inp(N, K, ldb, lambda: Bl)
        d["A" + sfx], d["B" + sfx] = Ab.ptr, Bb.ptr
        prs.append((Al, Bl))
    d.update(batch=batch if batch > 1 else 0, ksegs=ksegs if ksegs > 1 else 0)
    accumulates = bool(o.get("atomic")) or splits_in > 1
    alphas = o.get("alphas", (o.get("alpha", 0.75),))
    for m in range(batch):
        sfx = "" if m == 0 else "_x%d" % m
        biasb = None
        if o.get("bias", 1) and m not in o.get("nobias", ()):
            biasb = inp(1, N, N, lambda m=m: rn((1, N), seed0 + 3 + m))
            d["bias" + sfx] = biasb.ptr
        if batch > 1:
            d["alpha" + sfx] = alphas[m]
        pre_fill = None
        if accumulates or (o.get("alias") and m == 0):
            pre_fill = None if dry else rn((M, N), seed0 + 40 + m)
        Db = Buf(be, M, N, ldd, ACC_CANARY if accumulates else OUT_CANARY, None if pre_fill is None else (lambda pf=pre_fill: pf), shift=o.get("dshift", 0))
        d["D" + sfx] = Db.ptr
        outs.append(dict(D=Db, ops=prs if ksegs > 1 else [prs[m]], alpha=alphas[m] if batch > 1 else o.get("alpha", 0.75), bias=biasb, prefill=pre_fill))
    o0 = outs[0]
    if o.get("res"):
        if o.get("alias"):
            o0["res"], d["residual"] = o0["prefill"], o0["D"].ptr
        else:
            o0["res"] = None if dry else rn((M, N), seed0 + 50)
            d["residual"] = inp(M, N, ldr, lambda: o0["res"]).ptr
        d["ldr"] = ldr
    if o.get("cs"):
        o0["cs"] = inp(1, N, N, lambda: rn((1, N), seed0 + 51).abs() * 0.5 + 0.5)
        d["colscale"] = o0["cs"].ptr
    if o.get("rs"):
        def rsdata():
            rsv = rn((1, RS_MOD), seed0 + 52).abs() * 0.3 + 0.6
            rsv[0, 1] = 0.0                                   # a dropped path
            return rsv.clamp(max=1.5)
        o0["rs"] = inp(1, RS_MOD, RS_MOD, rsdata)
        d.update(rowscale=o0["rs"].ptr, rs_div=RS_DIV, rs_mod=RS_MOD)
    if o.get("drop"):
        sd = torch.tensor([SEED], dtype=torch.int64)
        d.update(dropout_p=DROP_P, site=SITE, seed_dev=sd if dry else sd.to(be.dev))
    if o.get("dpre"):
        o0["Dpre"] = Buf(be, M, N, ldd, OUT_CANARY)
        d["Dpre"] = o0["Dpre"].ptr
    if o.get("after"):
        d["act_after"] = 1
    if o.get("atomic"):
        d["atomic"] = 1
    if o.get("rowsum"):
        init = None if dry else (rn((1, M), seed0 + 60) if o.get("rowsum_init") else torch.zeros((1, M)))
        o0["rowsum"], o0["rowsum_init"] = Buf(be, 1, M, M, ACC_CANARY, None if dry else (lambda: init), extra=0), init
        d["a_rowsum"] = o0["rowsum"].ptr
    return _finish(name, o, [d], outs, inputs)


def _finish(name, o, calls, outs, inputs):
    loop, epi, nfn = cls_of(name)
    for d in calls:
        got = gemm_f32_class(fields_of(d))
        want = (loop, epi, nfn, ("kc", "ks2", "conv")[d["a_mode"]], ("kc", "ks")[d["b_mode"]], d["precision"])
        assert got == want, "%s reaches %s, not %s" % (name, got, want)
        plan = gemm_f32_plan(fields_of(d))
        if "grid" in o:
            assert plan["grid"] == o["grid"], "%s launches %d workgroups, not %d" % (name, plan["grid"], o["grid"])
        assert (plan["grid"] >= 384 and d.get("a_rowsum") is None) == (loop == "S"), (name, plan)
    return dict(calls=calls, cls=want, outs=outs, inputs=inputs, o=o, name=name, plan=plan)


def _build_subpixel(be, name, o):
    """ops/conv.py conv_nhwc: class (py, px) is a stride-1, pad-0 gather with (1 + py) x (1 + px) taps over the input grid whose row m lands on
    output pixel (2 y + py, 2 x + px): ldd = 2 Cout, d_row_w = IW, d_row_off = py IW, D offset by px Cout"""
    s, dry, seed0 = o["sub"], be.dry, 1000 * (CASES.index(name) + 1)
    Fr, IH, IW, Cin, Cout = (s[k] for k in ("Fr", "IH", "IW", "Cin", "Cout"))
    M = Fr * IH * IW
    x = None if dry else operand((M, Cin), seed0)
    wt = None if dry else operand((Cin, Cout, 3, 3), seed0 + 1, (2.25 * Cin) ** -0.5)           # the ConvTranspose2d weight
    inputs = []

    def inp(rows, cols, ld, data):
        b = Buf(be, rows, cols, ld, IN_NAN, None if dry else data)
        inputs.append(b)
        return b
    Ab = inp(M, Cin, Cin, lambda: x)
    biasb = inp(1, Cout, Cout, lambda: rn((1, Cout), seed0 + 3))
    csb = inp(1, Cout, Cout, lambda: rn((1, Cout), seed0 + 51).abs() * 0.5 + 0.5) if o.get("cs") else None
    Db = Buf(be, 4 * M, Cout, Cout, OUT_CANARY, extra=0)                                  # NHWC [Fr, 2 IH, 2 IW, Cout], tight by construction
    taps = {0: [1], 1: [2, 0]}
    calls = []
    for py in (0, 1):
        for px in (0, 1):
            K = (1 + py) * (1 + px) * Cin
            Bb = inp(Cout, K, K + 12, lambda py=py, px=px: wt[:, :, taps[py]][:, :, :, taps[px]].permute(1, 2, 3, 0).reshape(Cout, -1))
            d = dict(M=M, N=Cout, K=K, lda=0, ldb=K + 12, ldd=2 * Cout, a_mode=2, b_mode=0, precision=3, split_k=1, alpha=o.get("alpha", 0.75), act=o.get("act", NONE),
                     A=Ab.ptr, B=Bb.ptr, D=Db.ptr if dry or px == 0 else Db.ptr[px * Cout:], bias=biasb.ptr, d_row_w=IW, d_row_off=py * IW,
                     conv_IH=IH, conv_IW=IW, conv_Cin=Cin, conv_OH=IH, conv_OW=IW, conv_KH=1 + py, conv_KW=1 + px, conv_stride=1, conv_pad=0, conv_pad_mode=ZERO,
                     conv_transposed=0)
            if dry and px:
                d["D"] = type("P", (), {"data_ptr": lambda self, a=Db.ptr.data_ptr() + 4 * px * Cout: a})()
            if csb is not None:
                d["colscale"] = csb.ptr
            calls.append(d)
    cg = conv(Fr, IH, IW, Cin, 3, 3, 2, 1, tr=1, outpad=1)
    out = dict(D=Db, alpha=o.get("alpha", 0.75), bias=biasb, prefill=None, sub=(x, wt, cg))
    if csb is not None:
        out["cs"] = csb
    return _finish(name, dict(o, M=4 * M, N=Cout, K=4 * Cin), calls, [out], inputs)


def class_census():
    """class -> cases that run it"""
    be, out = DryBackend(0), {}
    for name in CASES:
        out.setdefault(build(be, name)["cls"], []).append(name)
    return out


def census_gaps(census):
    """what the issue's census asks for and the cases do not deliver (empty = complete)"""
    gaps = []
    full = {k for k in FULL}

    def cases(pred):
        return [n for c, ns in census.items() if pred(c) for n in ns]
    for loop, epi, nfn in LOOPS_EPIS:
        got = cases(lambda c: c[:3] == (loop, epi, nfn))
        if len(got) < 2:
            gaps.append(("fewer than two cases", loop, epi, nfn, got))
        if not any(all(SPEC[n].get(k) for k in full) and SPEC[n].get("prec", 3) == 3 for n in got):
            gaps.append(("no case with the full option set at precision 3", loop, epi, nfn))
    assert {c[:3] for c in census} == set(LOOPS_EPIS), sorted({c[:3] for c in census})
    for epi in ("rows", "frag", "rows_halves", "serial"):       # the options the full set cannot hold: ReLU, LeakyReLU, D as its own residual, alpha = 0
        got = cases(lambda c: c[1] == epi)
        for what, pred in (("ReLU", lambda o: o.get("act") == RELU), ("LeakyReLU", lambda o: o.get("act") == LRELU),
                           ("D aliasing the residual", lambda o: o.get("alias")), ("alpha = 0", lambda o: o.get("alpha") == 0.0),
                           ("dropout without a residual", lambda o: o.get("drop") and not o.get("res"))):
            if not any(pred(SPEC[n]) for n in got):
                gaps.append(("no case in this epilogue function with", epi, what))
    for loop in "PS":
        for a, b in MODE_PAIRS:
            if not cases(lambda c: c[0] == loop and c[3:5] == (a, b)):
                gaps.append(("no case for the mode pair", loop, a, b))
        for b in ("kc", "ks"):
            for nfn in (4, 8, 11):
                if not cases(lambda c: c[0] == loop and c[2] == nfn and c[4] == b):
                    gaps.append(("no case for the B stager at this NFN", loop, b, nfn))
            if not cases(lambda c: c[0] == loop and c[4] == b and c[5] == 1):
                gaps.append(("no precision-1 case for the B stager", loop, b))
        for a in ("kc", "ks2", "conv"):
            if not cases(lambda c: c[0] == loop and c[3] == a and c[5] == 1):
                gaps.append(("no precision-1 case for the A stager", loop, a))
    return gaps


# ------------------------------------------------------------------------------------------------------------------ reference and bars
def _products(be, c, out):
    """fp64 products of one output: (element reference, S, raw reference) before the epilogue"""
    o, prec = c["o"], c["calls"][0]["precision"]
    if "sub" in out:
        x, wt, cg = out["sub"]
        wfull = wt.permute(1, 2, 3, 0).reshape(wt.shape[1], -1)
        xs, ws = (sum(split_f32(t)) for t in (x, wfull))
        return conv64(xs, ws, cg), conv64(xs.abs(), ws.abs(), cg), conv64(x, wfull, cg)
    acc = S = raw = 0
    for Al, Bl in out["ops"]:
        sa, sb = split_f32(Al), split_f32(Bl)
        As, Bs = (sa[0] + sa[1], sb[0] + sb[1]) if prec == 3 else (sa[0], sb[0])
        if o.get("conv"):
            acc, S, raw = acc + conv64(As, Bs, o["conv"]), S + conv64(As.abs(), Bs.abs(), o["conv"]), raw + conv64(Al, Bl, o["conv"])
        else:
            acc, S, raw = acc + be.mm64(As, Bs), S + be.mm64(As.abs(), Bs.abs()), raw + be.mm64(Al, Bl)
    return acc, S, raw


_KEEP = {}


def keep_scale(M, N, ld=None):
    """the dropout scale of every element of an M x N output (index row * N + col), computed once per shape"""
    key = (M, N, ld)
    if key not in _KEEP:
        if len(_KEEP) >= 2:
            _KEEP.pop(next(iter(_KEEP)))
        _KEEP[key] = drop_scale_emu(SEED, SITE, torch.arange(M)[:, None] * (ld or N) + torch.arange(N)[None, :], DROP_P)
    return _KEEP[key]


def reference(c, out, first, acc, S):
    """fp64 reference of one output matrix; with S also its per-element bar: dict ref, bar, kink, pre, bar_pre, dropped, res"""
    o = c["o"]
    M, N, K = o["M"], o["N"], o["K"]
    prec, nseg, plan = c["calls"][0]["precision"], o.get("ksegs", 1), c["plan"]
    nk = -(-K // 32) if "sub" in o else sum(-(-(min(K, (s + 1) * plan["k_chunk"]) - s * plan["k_chunk"]) // 32) for s in range(plan["splits"]))
    bar = ((2.0 ** -18 + (32 + 3 * nk * nseg) * U) if prec == 3 else (32 + nk * nseg) * U) * S
    v, mags = acc, torch.zeros_like(acc)
    amag = S.clone()
    if first and "cs" in out:
        cs = out["cs"].live().double()
        v, bar, amag = v * cs, bar * cs.abs(), amag * cs.abs()
        mags = mags + v.abs()
    if out["bias"] is not None:
        b = out["bias"].live().double()
        v, amag = v + b, amag + b.abs()
        mags = mags + v.abs()
    alpha = f32(out["alpha"]) or 1.0
    v, bar, amag = v * alpha, bar * abs(alpha), amag * abs(alpha)
    mags = mags + v.abs()
    pre, bar_pre = v, bar + U * mags
    kink = torch.zeros(v.shape, dtype=torch.bool)
    act = o.get("act", NONE)
    t = act64(v, act)
    if act == GELU:
        bar = bar * 1.13
        mags = mags + 8 * v.abs() + t.abs()
    elif act in (RELU, LRELU):
        kink |= pre.abs() <= bar_pre
        mags = mags + t.abs()
    if first and "rs" in out:
        rs = out["rs"].live().double().view(-1)[(torch.arange(M) // RS_DIV) % RS_MOD][:, None]
        t, bar = t * rs, bar * rs.abs()
        mags = mags + t.abs()
    dropped = None
    if o.get("drop"):
        keep = keep_scale(M, N).double()
        dropped = keep == 0
        share = float(dropped.double().mean())
        assert 0.05 < share < 0.15, share
        t, bar = t * keep, bar * keep
        mags = mags + t.abs()
    res = out.get("res") if first else None
    if res is not None:
        t = t + res.double()
        mags = mags + t.abs()
        amag = amag + res.double().abs()
    if o.get("after"):
        kink |= t.abs() <= bar + U * mags
        t = torch.relu(t)
    if o.get("atomic") or plan["splits"] > 1:
        d0 = out["prefill"].double()
        t = t + d0
        bar = bar + max(plan["splits"], 1) * U * (d0.abs() + amag)
    bar = bar + U * mags
    return dict(ref=t, bar=bar, kink=kink, pre=pre, bar_pre=bar_pre, dropped=dropped, res=res)


def check_matrix(tag, cls, got, ref, bar, kink, ref_raw, tol):
    assert bool(torch.isfinite(got).all()), "%s: NaN or Inf in the output (an element that was never written keeps the canary)" % tag
    err = (got.double() - ref).abs()
    ratio = torch.where(kink, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    worst = float(ratio.max())
    i = int(ratio.reshape(-1).argmax())
    rc = rowcol(got, ref_raw)
    share = float(kink.double().mean())
    print("%s %s: worst element error / bar %.3f at (%d, %d) (ref %.6e, got %.6e, bar %.3e); worst row / column rel-L2 %.3e; kinks %.2e"
          % (tag, cls, worst, i // ref.shape[1], i % ref.shape[1], float(ref.reshape(-1)[i]), float(got.reshape(-1)[i]), float(bar.reshape(-1)[i]), rc,
             share))
    margin("gemm_f32 %s element %s" % (cls, tag), worst, 1.0)
    margin("gemm_f32 %s rowcol %s" % (cls, tag), rc, tol)
    assert share <= KINK_SHARE, (tag, "kinks", share)
    assert worst <= 1.0, (tag, "element over its bar", worst, i // ref.shape[1], i % ref.shape[1])
    assert rc < tol, (tag, "row / column rel-L2", rc)
    return worst, rc


def run_case(be, name):
    c = build(be, name)
    o = c["o"]
    for d in c["calls"]:
        rc = be.gemm(d)
        assert rc == 0, (name, rc, be.last_error())
    be.sync()
    tol = TOL3 if c["calls"][0]["precision"] == 3 else TOL1
    figures = []
    for m, out in enumerate(c["outs"]):
        tag = name if len(c["outs"]) == 1 else "%s[%d]" % (name, m)
        acc, S, raw = _products(be, c, out)
        R = reference(c, out, m == 0, acc, S)
        Rraw = reference(c, out, m == 0, raw, S)
        assert out["D"].guards_intact(), "%s: D written outside its %d x %d elements" % (tag, o["M"], o["N"])
        data = rowcol(R["ref"], Rraw["ref"])       # a property of the seeded data alone: how far the split operands are from the raw ones
        assert data < tol / 3, "%s: the references of the split and of the raw operands are %.2e apart in a row or column: choose another seed" % (tag, data)
        got = out["D"].live()
        if R["dropped"] is not None:          # exactly the emulated pattern: a dropped element is its residual bit for bit, +0 without one
            want = R["res"].float() if R["res"] is not None else torch.zeros_like(got)
            if o.get("after"):
                want = torch.relu(want)
            dm = R["dropped"]
            bad = int((got[dm].view(torch.int32) != want[dm].view(torch.int32)).sum())
            assert bad == 0, "%s: %d of %d dropped elements are not their residual / +0 bit for bit" % (tag, bad, int(dm.sum()))
        figures.append(check_matrix(tag, c["cls"], got, R["ref"], R["bar"], R["kink"], Rraw["ref"], tol))
        if "Dpre" in out:
            assert out["Dpre"].guards_intact(), "%s: Dpre written outside its elements" % tag
            figures.append(check_matrix(tag + " Dpre", c["cls"], out["Dpre"].live(), R["pre"], R["bar_pre"], torch.zeros_like(R["kink"]), Rraw["pre"], tol))
        if "rowsum" in out:
            assert out["rowsum"].guards_intact(), "%s: a_rowsum written outside its %d rows" % (tag, o["M"])
            Al = out["ops"][0][0]
            a64 = sum(split_f32(Al)).double()
            al = f32(out["alpha"]) or 1.0
            init = out["rowsum_init"].double().view(-1)
            want = init + al * a64.sum(1)
            nk, sp = -(-o["K"] // 32), c["plan"]["splits"]
            rbar = abs(al) * (2.0 ** -17 + (2 * nk + 8 + sp) * U) * a64.abs().sum(1) + sp * U * init.abs()
            gr = out["rowsum"].live().double().view(-1)
            assert bool(torch.isfinite(gr).all()), "%s: a row sum was never written" % tag
            w = float(((gr - want).abs() / rbar.clamp_min(1e-300)).max())
            print("%s: a_rowsum worst error / bar %.3f" % (tag, w))
            margin("gemm_f32 %s rowsum %s" % (c["cls"], tag), w, 1.0)
            assert w <= 1.0, (tag, "a_rowsum over its bar", w)
    for b in c["inputs"]:
        assert b.unchanged(), "%s: an input of the call changed" % name
    if o.get("drop"):
        assert int(c["calls"][0]["seed_dev"].cpu()[0]) == SEED, "%s: the seed word changed" % name
    return c["cls"], figures


# ------------------------------------------------------------------------------------------------------------------ rejections
def run_reject(be, k):
    """a valid descriptor bent so that the k-th reachable VPTR_CHECK of vptr_gemm refuses it (helpers.gemm_f32_class numbers them; 0 = no
    descriptor at all): negative return code, a message, every buffer unchanged, and the mirror refuses at the same check"""
    base = "conv3s1_zero" if k in (16, 17, 18) else ("ksks_K33" if k == 13 else "kc_K36")
    c = build(be, base)
    d, extra = dict(c["calls"][0]), []
    M, N = d["M"], d["N"]

    def out_buf():
        b = Buf(be, M, N, d["ldd"], OUT_CANARY)
        extra.append(b)
        return b.ptr
    x12 = dict(A_x1=d["A"], B_x1=d["B"], A_x2=d["A"], B_x2=d["B"])
    if k == 1:
        d["K"] = 0
    elif k == 2:
        d["B"] = None
    elif k == 3:
        d["D_planes"] = out_buf()
    elif k == 4:
        d["precision"] = 2
    elif k == 5:
        d["batch_accum"] = 1
    elif k == 6:
        d["d_p16"] = 1
    elif k == 7:
        d.update(d_row_w=0, d_row_off=4)
    elif k == 8:
        d.update(frame_stats=out_buf(), frame_rows=64)
    elif k == 9:
        d["a_mode"] = 4
    elif k == 10:
        d["A"] = d["A"][1:]
    elif k == 11:
        d["K"] = 34
    elif k == 12:
        d["lda"] = d["lda"] + 2
    elif k == 13:
        d["M"] = M - 2
    elif k == 14:
        d["ldb"] = d["ldb"] + 1
    elif k == 15:
        d.update(b_mode=1, N=50)
    elif k == 16:
        d.update(conv_Cin=6, conv_KH=2, conv_KW=2, K=24)
    elif k == 17:
        d["conv_KH"] = 2
    elif k == 18:
        d["conv_stride"] = 0
    elif k == 19:
        d.update(split_k=2, act=GELU)
    elif k == 20:
        d["dropout_p"] = 0.1
    elif k == 21:
        d.update(rowscale=d["bias"], rs_div=0, rs_mod=5)
    elif k == 22:
        d.update(ksegs=4, **x12)
    elif k == 23:
        d.update(ksegs=2, batch=2, D_x1=out_buf(), **x12)
    elif k == 24:
        d.update(ksegs=2, split_k=2, **x12)
    elif k == 25:
        d.update(ksegs=2, A_x1=d["A"])
    elif k == 26:
        d.update(ksegs=3, A_x1=d["A"], B_x1=d["B"], A_x2=d["A"][1:], B_x2=d["B"])
    elif k == 27:
        d.update(batch=2, A_x1=d["A"], B_x1=d["B"])
    elif k == 28:
        d.update(batch=2, A_x1=d["A"], B_x1=d["B"], D_x1=out_buf(), atomic=1)
    elif k == 29:
        d["a_rowsum"] = out_buf()
    elif k == 30:
        d.update(a_mode=2, b_mode=1, N=64, ldb=68, conv_IH=4, conv_IW=4, conv_Cin=4, conv_OH=4, conv_OW=4, conv_KH=3, conv_KW=3, conv_stride=1, conv_pad=1)
    if k == 0:
        d = None                            # vptr_gemm(NULL, stream): refused before anything is read
    else:
        got = gemm_f32_class(fields_of(d))
        assert got == ("refuse", k), (k, got)
    rc = be.gemm(d)
    be.sync()
    assert rc < 0, (k, rc)
    assert len(be.last_error()) > 0, k
    for out in c["outs"]:
        assert out["D"].unchanged(), "check %d: D was written" % k
    for b in extra + c["inputs"]:
        assert b.unchanged(), "check %d: a buffer changed" % k
