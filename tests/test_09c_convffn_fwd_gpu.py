"""Op-level fp64 parity of the forward half of the conv-FFN through the C ABI: vptr_norm_act_fwd in every launch class (the per-column kernel
with its grid-stride second trip, the row-major LayerNorm kernel, the position-major kernel at and past its threshold; statistics handed in or
derived from the producer's per-frame sums, dropout + DropPath row scale + residual, a P16 output), the large-mean recompute of the one-pass
variance in the four kernels that hold it, the frame_stats epilogue of vptr_dwconv3x3_fwd, the fused norm1 + GELU + depthwise
vptr_dwconv3x3_norm_fwd in its LDS-slab and register forms (y, the fp16 side copy, mean_out / rstd_out, frame_stats), the producer -> consumer
chain on real fp32-atomic sums, and one forward + backward through ops.norm_dwconv3x3.

The cases, the guarded buffers, the references and the bars live in tests/convffn_fwd_cases.py, which tests/test_cpu.py also runs against a CPU
emulation of the calls; this file supplies the backend that hands the pointers to the library.  Every reference is plain torch fp64 on the CPU
from the same seeded inputs (helpers.norm_act_fwd_ref / dwconv3x3_fwd_ref / dwconv_norm_fwd_ref, checked against the modules' NCHW formulation in
tests/test_cpu.py).  Bars (rel-L2): fp32 outputs and statistics 2e-5, a decoded P16 output 2^-16, the fp16 side copy
2^-11 |ref| + 2^-24 per element and 2^-11 rel-L2, gradients 5e-5; bit equality for everything a call must not touch."""
import pytest
import torch
import torch.nn.functional as F

import convffn_fwd_cases as C
from helpers import rel

pytestmark = pytest.mark.gpu

TOLG = 5e-5                      # gradients of the fp32 vector kernels


class LibBackend:
    """the library itself: tensors become raw device pointers, the current stream is appended, the return code comes back"""

    def __init__(self, dev):
        import vptr_amd.ops as ops
        from vptr_amd import _lib
        self.dev, self.ops, self.lib = dev, ops, _lib

    def call(self, name, *args):
        L = self.lib
        for a in args:
            assert not isinstance(a, torch.Tensor) or (a.is_cuda and a.is_contiguous())
        raw = [L.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
        return getattr(L.lib, "vptr_" + name)(*raw, L.stream())

    def seed(self, value):
        self.ops.manual_seed(self.dev, value)
        return self.ops.new_seed_scope(self.dev)

    def dropout_mask(self, n, p, seed, site):
        L = self.lib
        ones, md = torch.ones(n, device=self.dev), torch.empty(n, device=self.dev)
        L.check(L.lib.vptr_dropout(L.ptr(ones), L.ptr(md), n, p, L.ptr(seed), site, L.stream()), "vptr_dropout")
        return md

    def p16_decode(self, t):
        return self.ops.p16_decode(t.to(self.dev)).cpu()

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a conv-FFN forward call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


def _geom_id(g):
    return "x".join(str(v) for v in g)


# --------------------------------------------------------------------------------------------------------------- a. vptr_norm_act_fwd
@pytest.mark.parametrize("gid,variant", C.na_cases(), ids=["%s-%s" % c for c in C.na_cases()])
def test_norm_act_fwd(be, gid, variant):
    """one geometry per launch class (convffn_fwd_cases.NA_GEOMS) x plain (no activation, statistics handed in) / full (GELU, dropout 0.1 with
    the regenerated mask, rowscale[(row / 7) % 5] -- 7 does not divide HW --, residual) / raw (GELU, mean and rstd derived from the per-frame
    sums and written out) / p16 (GELU, P16 output) and ReLU once; the rows of a grid-stride second trip and the frames of a ragged last trip of
    the position-major kernel are compared on their own as well"""
    C.run_norm_act(be, gid, variant)


def test_norm_act_fwd_rejects(be):
    C.run_norm_act_rejects(be)


# ------------------------------------------------------------------------------------------------------------ b. the large-mean guard
@pytest.mark.parametrize("r", C.GUARD_RATIOS)
@pytest.mark.parametrize("place", sorted(C.GUARD_PLACES))
def test_large_mean_guard(be, place, r):
    """|mean| = r std (r = 9: below the guard, one-pass variance; 12, 25, 100: redone around the mean) in norm_act_fwd_kernel,
    norm_act_fwd_pos_kernel, dwconv_norm_lds_kernel and dwconv_norm_fwd3_kernel.  With the guard at var < 1e-3 E[x^2] (|mean| > 31.6 std) r = 25
    took the one-pass branch and missed the bar (profiles/convffn_fwd_margins.md); the guard is var < 1e-2 E[x^2] now"""
    C.run_guard(be, place, r)


# ----------------------------------------------------------------------------------------- c. vptr_dwconv3x3_fwd with frame_stats
@pytest.mark.parametrize("geom", sorted(C.DW_STATS_GEOMS), ids=_geom_id)
def test_dwconv3x3_fwd_frame_stats(be, geom):
    C.run_dwconv_stats(be, geom)


def test_dwconv3x3_fwd_frame_stats_rejects(be):
    C.run_dwconv_stats_rejects(be)


# ------------------------------------------------------------------------------------------------- d. vptr_dwconv3x3_norm_fwd
@pytest.mark.parametrize("geom,variant", C.dwn_cases(), ids=["%s-%s" % (_geom_id(g), v) for g, v in C.dwn_cases()])
def test_dwconv3x3_norm_fwd(be, geom, variant):
    """GELU with every output present on each geometry of the LDS-slab and the register kernel; on the model's map and on the F % 64 != 0 one
    also no activation, a_half = NULL, frame_stats = NULL and b = NULL.  The 16 x 16 map asks for a 64 KB dynamic slab next to the kernel's
    32-byte static array: the launch is accepted as it is (measured; no launcher change)"""
    C.run_dwn(be, geom, variant)


@pytest.mark.parametrize("geom,variant", C.dwn_cases(True), ids=["%s-%s" % (_geom_id(g), v) for g, v in C.dwn_cases(True)])
def test_dwconv3x3_norm_fwd_half_copy_elements(be, geom, variant):
    """every element of the fp16 side copy within 2^-11 |ref| + 2^-24 of the fp64 activated tensor: round-to-nearest of a correct value, so the
    fp32 activation itself has to be right to about 2^-22 |ref| + 2^-24 where a value sits just above a power of two.  With the five-term
    erfc polynomial (absolute error 1.5e-7) 2 - 12 GELU elements per case near a pre-activation of -3.7 exceeded the bound by up to 1.17 x on five
    of the seven geometries; vptr_phi now uses a degree-8 polynomial fitted in relative error, and the worst element of every case sits at
    0.98 - 1.00 of the bound (profiles/convffn_fwd_margins.md)"""
    C.run_dwn_half_elements(be, geom, variant)


def test_dwconv3x3_norm_fwd_rejects(be):
    C.run_dwn_rejects(be)


# --------------------------------------------------------------------------------------------------- e. chain with real producer sums
@pytest.mark.parametrize("geom", C.CHAIN_GEOMS, ids=_geom_id)
def test_producer_sums_feed_the_normalisation(be, geom):
    C.run_chain(be, geom)


# ----------------------------------------------------------------------------------------- f. forward + backward through ops.norm_dwconv3x3
def test_norm_dwconv3x3_through_ops(ops, dev):
    """ops.norm_dwconv3x3 at 5 x 8 x 8 x 64 against fp64 autograd of conv2d(gelu(layer_norm(x))): y, dx, the affine gradients, dw9 / db9 (the
    weight gradient reads the fp16 side copy: its reference reads the fp64 activated tensor rounded to fp16, as
    test_09b::test_dwconv3x3_bwd_weight_classes does) -- the statistics the forward leaves are the ones the backward reads"""
    frames, H, W, Fc = 5, 8, 8, 64
    HW, rows = H * W, frames * H * W
    x, dy = C.rn((rows, Fc), 9000, 2.0) + 0.3, C.rn((rows, Fc), 9001)
    aw, ab = C.rn((HW, Fc), 9002).abs() + 0.5, C.rn((HW, Fc), 9003, 0.3)
    wt, b9 = C.rn((Fc, 1, 3, 3), 9004, 0.3), 1.0 + C.rn((Fc,), 9005, 0.3)

    def nchw(t):
        return t.reshape(frames, H, W, Fc).permute(0, 3, 1, 2)

    def rows_of(t):
        return t.permute(0, 2, 3, 1).reshape(rows, Fc)
    xr, awr, abr = (t.double().requires_grad_(True) for t in (x, aw, ab))
    wr, br = wt.double().requires_grad_(True), b9.double().requires_grad_(True)
    a = F.gelu(F.layer_norm(xr.view(frames, HW, Fc), (HW, Fc), awr, abr, 1e-5)).reshape(rows, Fc)
    y_ref = rows_of(F.conv2d(nchw(a), wr, br, padding=1, groups=Fc))
    y_ref.backward(dy.double())
    wh = wt.double().requires_grad_(True)
    F.conv2d(nchw(a.detach().half().double()), wh, None, padding=1, groups=Fc).backward(nchw(dy.double()))

    raw = torch.zeros((frames, ops.FRAME_STATS_STRIDE))
    s0, s1 = C.ideal_sums(x, frames)
    raw[:, 0], raw[:, 1] = s0.float(), s1.float()
    xd, awd, abd = (t.to(dev).requires_grad_(True) for t in (x, aw, ab))
    wd, bd = wt.to(dev).requires_grad_(True), b9.to(dev).requires_grad_(True)
    stats = torch.zeros((frames, ops.FRAME_STATS_STRIDE), device=dev)
    y = ops.norm_dwconv3x3(xd, awd, abd, wd, bd, frames, H, W, raw.to(dev), stats)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    yf = y_ref.detach().view(frames, -1)
    assert rel(y, y_ref) < C.TOLV
    assert rel(stats[:, 0], yf.sum(1)) < C.TOLV and rel(stats[:, 1], (yf * yf).sum(1)) < C.TOLV
    assert rel(xd.grad, xr.grad) < TOLG
    assert rel(awd.grad, awr.grad) < TOLG and rel(abd.grad, abr.grad) < TOLG
    assert rel(wd.grad, wh.grad) < TOLG
    assert rel(bd.grad, br.grad) < TOLG
