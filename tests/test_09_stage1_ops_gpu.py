"""Op-level fp64 parity of the stage-1 training kernels (auto-encoder + PatchGAN; the stage-2 GAN step uses them too): the trainable
convolution `ops.conv2d_nhwc` with every piece of its backward, the 7x7 input convolution's raw forward and weight gradient, train-mode
BatchNorm as the auto-encoder uses it, and the small kernels behind them called directly through the C ABI.

Every reference is plain torch fp64 on the CPU (F.conv2d, F.conv_transpose2d, F.pad, F.batch_norm, autograd) on the same seeded inputs.
Bars (rel-L2): outputs of precision-3 GEMM-backed ops 3e-5, their weight / bias gradients 5e-5; fp32 vector kernels
2e-5, their gradients 5e-5; pure data movement exact.

Activation kinks: a ReLU / LeakyReLU gradient flips where fp32 and fp64 disagree on the sign of a pre-activation next to zero, which is
no kernel error.  The upstream gradient is therefore zeroed where the fp64 pre-activation satisfies |pre| < 1e-3 * rms(pre); the zeroed
share must stay <= 0.5 % (Gaussian inputs give 0.07 - 0.11 %) -- a condition on the inputs, not a tolerance.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import reflect_fold_ref, rel, unfold_kkc
from oracle import fill

pytestmark = pytest.mark.gpu

TOL3, TOLV = 3e-5, 2e-5          # precision-3 GEMM outputs; fp32 vector kernels
TOLG = 5e-5                      # weight / bias gradients of GEMM-backed ops, gradients of fp32 vector kernels
KINK, KINK_CAP = 1e-3, 5e-3
NONE, RELU, LRELU = 0, 2, 3      # ops.ACT_*


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


def act64(z, act):
    return torch.relu(z) if act == RELU else (F.leaky_relu(z, 0.2) if act == LRELU else z)


def off_kink(go, pre, act):
    """upstream gradient with the elements next to the activation's kink zeroed (module docstring); asserts the cap on their share"""
    if act == NONE:
        return go
    near = pre.detach().abs() < KINK * pre.detach().pow(2).mean().sqrt()
    share = float(near.double().mean())
    assert share <= KINK_CAP, "%.3f %% of the pre-activations lie next to the kink: pick other seeds" % (100 * share)
    return torch.where(near, torch.zeros_like(go), go)


def tokens(x):      # NCHW -> [(b, h, w), C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ A1. conv2d_nhwc autograd matrix
# id: (frames, IH, IW, Cin, Cout, K, stride, pad, pad_mode, transposed, act, bias, x_grad, split_k > 1 expected)
CONV_CASES = {
    # encoder down-sampling: 3x3 stride 2, zero padding
    "down_small": (2, 6, 10, 8, 12, 3, 2, 1, "zero", False, RELU, True, True, False),
    "down_64_128": (3, 16, 12, 64, 128, 3, 2, 1, "zero", False, NONE, False, True, False),
    # ResnetBlock: 3x3 stride 1, reflection padding -> gradient on the padded grid + vptr_reflect_fold
    "res_reflect_48": (3, 5, 7, 48, 48, 3, 1, 1, "reflect", False, RELU, True, True, False),
    "res_reflect_528": (2, 8, 8, 528, 528, 3, 1, 1, "reflect", False, NONE, True, True, False),
    "res_reflect_2x3": (3, 2, 3, 8, 8, 3, 1, 1, "reflect", False, LRELU, True, True, False),   # smallest map the fold takes: 3 pre-images along W
    "res_reflect_splitk": (3, 14, 13, 16, 24, 3, 1, 1, "reflect", False, NONE, False, True, True),
    "zero_s1": (2, 7, 9, 16, 24, 3, 1, 1, "zero", False, LRELU, True, True, False),
    # PatchGAN: 4x4 kernels.  First layer 4 (zero-padded image channels) -> 64 with LeakyReLU on an odd-sized map
    "patchgan_first": (3, 33, 27, 4, 64, 4, 2, 1, "zero", False, LRELU, True, True, True),
    "patchgan_first_nodx": (3, 33, 27, 4, 64, 4, 2, 1, "zero", False, LRELU, True, False, True),   # the image needs no gradient
    "patchgan_64_128": (2, 17, 13, 64, 128, 4, 2, 1, "zero", False, NONE, False, True, False),
    "patchgan_s1_128_256": (2, 9, 7, 128, 256, 4, 1, 1, "zero", False, NONE, False, True, False),   # stride 1: the output shrinks by one
    "patchgan_head_256_4": (3, 9, 7, 256, 4, 4, 1, 1, "zero", False, NONE, True, True, False),      # zero-padded one-channel logits head
    # decoder up-sampling: ConvTranspose2d 3x3 stride 2, pad 1, output_padding 1
    "convt_528_256": (2, 8, 8, 528, 256, 3, 2, 1, "zero", True, NONE, False, True, False),
    "convt_small_odd": (3, 3, 5, 8, 12, 3, 2, 1, "zero", True, RELU, True, True, False),
    "convt_splitk_nodx": (2, 16, 18, 24, 16, 3, 2, 1, "zero", True, LRELU, True, False, True),
}


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv2d_nhwc_autograd(ops, dev, case):
    """forward, dx, dW, db of ops.conv2d_nhwc vs fp64 autograd: vptr_act_bwd from the layer output, the gather-form transposed convolution
    (or, for ConvTranspose2d, the strided convolution) as data gradient, vptr_reflect_fold, vptr_im2col_nhwc + the split-K atomic GEMM,
    vptr_colsum"""
    frames, IH, IW, Cin, Cout, K, stride, pad, pad_mode, transposed, act, has_b, x_grad, want_split = CONV_CASES[case]
    seed = 1000 + 10 * sorted(CONV_CASES).index(case)
    out_pad = 1 if transposed else 0
    x = rn((frames, Cin, IH, IW), seed)
    w = rn((Cin, Cout, K, K) if transposed else (Cout, Cin, K, K), seed + 1, (K * K * Cin / (stride * stride if transposed else 1)) ** -0.5)
    b = rn((Cout,), seed + 2, 0.5) if has_b else None
    xr = x.double().requires_grad_(x_grad)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if has_b else None
    if transposed:
        pre = F.conv_transpose2d(xr, wr, br, stride=stride, padding=pad, output_padding=out_pad)
    elif pad_mode == "zero":
        pre = F.conv2d(xr, wr, br, stride=stride, padding=pad)
    else:
        pre = F.conv2d(F.pad(xr, (pad,) * 4, mode=pad_mode), wr, br, stride=stride)
    ref = act64(pre, act)
    OHr, OWr = ref.shape[2:]
    go = off_kink(rn(tuple(ref.shape), seed + 3).double(), pre, act)
    ref.backward(go)
    # which weight-gradient launch this geometry takes (the GEMM is [Cout or Cin] x [taps * C]; its K dimension is the pixel count)
    pix = frames * (IH * IW if transposed else OHr * OWr)
    rows_, cols_ = (Cin, K * K * Cout) if transposed else (Cout, K * K * Cin)
    assert (ops._split_k_for(((rows_ + 127) // 128) * ((cols_ + 175) // 176), pix) > 1) == want_split

    xd = tokens(x).to(dev).requires_grad_(x_grad)
    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if has_b else None
    y, OH, OW = ops.conv2d_nhwc(xd, wd, bd, frames, IH, IW, stride=stride, pad=pad, pad_mode=pad_mode, transposed=transposed,
                                output_padding=out_pad, act=act)
    assert (OH, OW) == (OHr, OWr) and y.shape == (frames * OH * OW, Cout)
    y.backward(tokens(go.float()).to(dev))
    assert rel(nchw(y, frames, OH, OW), ref) < TOL3
    if x_grad:
        assert rel(nchw(xd.grad, frames, IH, IW), xr.grad) < TOL3
    else:
        assert xd.grad is None
    assert rel(wd.grad, wr.grad) < TOLG
    if has_b:
        assert rel(bd.grad, br.grad) < TOLG


def test_conv2d_nhwc_documented_non_features(ops, dev):
    """the three backward paths conv.py names as not implemented raise their Python error before any gradient kernel is launched (the
    forward passes used here are supported geometries)"""
    frames, H, W, C = 2, 6, 6, 8
    x, w = rn((frames * H * W, C), 1), rn((C, C, 3, 3), 2, 0.1)

    def run(**kw):
        xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
        y, _, _ = ops.conv2d_nhwc(xd, wd, None, frames, H, W, **kw)
        y.backward(torch.ones_like(y))
    with pytest.raises(NotImplementedError, match="replicate"):
        run(stride=1, pad=1, pad_mode="replicate")
    with pytest.raises(NotImplementedError, match="stride 2"):
        run(stride=2, pad=1, pad_mode="reflect")
    with pytest.raises(RuntimeError, match="GELU"):
        run(stride=1, pad=1, act=ops.ACT_GELU)
    with pytest.raises(RuntimeError, match="zero padding only"):
        ops.conv2d_nhwc(x.to(dev), w.to(dev), None, frames, H, W, stride=2, pad=1, pad_mode="reflect", transposed=True, output_padding=1)


# ------------------------------------------------------------------------------------------------------------ A2. conv7_in autograd
@pytest.mark.parametrize("cimg", [1, 3])
@pytest.mark.parametrize("geom", [(7, 16, 24), (1, 64, 64), (3, 9, 11)])   # 2688 pixels: two workgroups add into dw, the second a partial 2048-pixel chunk;
def test_conv7_in_raw_forward_and_weight_gradient(ops, dev, cimg, geom):     # 4096: two whole chunks; 9 x 11: odd sizes (first-generation forward), one partial chunk
    """ops.conv7_in: vptr_conv7_in_fwd with scale == NULL (the raw convolution in front of a train-mode BatchNorm) and
    vptr_conv7_in_bwd_weight vs fp64 F.conv2d(F.pad(x, 3, reflect), w) and its weight gradient"""
    B, H, W = geom
    x, w, go = rn((B, cimg, H, W), 300), rn((64, cimg, 7, 7), 301, (49 * cimg) ** -0.5), rn((B, 64, H, W), 302)
    wr = w.double().requires_grad_(True)
    ref = F.conv2d(F.pad(x.double(), (3, 3, 3, 3), mode="reflect"), wr)
    ref.backward(go.double())
    wd = w.to(dev).requires_grad_(True)
    y = ops.conv7_in(x.to(dev), wd)
    y.backward(tokens(go).to(dev))
    assert rel(nchw(y, B, H, W), ref) < TOLV
    assert rel(wd.grad, wr.grad) < TOLG


@pytest.mark.parametrize("geom", [(2, 16, 24), (1, 64, 64)])
def test_conv7_in_planes_output(dev, abi, geom):
    """vptr_conv7_in_fwd_planes: the decoded hi + lo planes equal the fp64 folded-BatchNorm + ReLU result at the plane round-off (2^-16 relative),
    and the last row, which the caller zeroed, stays zero"""
    B, H, W = geom
    x, w = rn((B, 1, H, W), 310), rn((64, 1, 7, 7), 311, 1.0 / 7)
    sc, sh = rn((64,), 312).abs() + 0.5, rn((64,), 313, 0.3)
    ref = torch.relu(F.conv2d(F.pad(x.double(), (3, 3, 3, 3), mode="reflect"), w.double()) * sc.double()[None, :, None, None]
                     + sh.double()[None, :, None, None])
    xd, wd, scd, shd = x.to(dev), w.to(dev), sc.to(dev), sh.to(dev)
    planes = torch.zeros((B * H * W + 1, 2, 64), device=dev, dtype=torch.bfloat16)
    abi.check(abi.lib.vptr_conv7_in_fwd_planes(abi.ptr(xd), abi.ptr(wd), abi.ptr(scd), abi.ptr(shd), abi.ptr(planes), B, 1, H, W, 64, abi.stream()),
              "vptr_conv7_in_fwd_planes")
    assert float(planes[-1].float().abs().max()) == 0.0
    rec = (planes[:-1, :, :32].float() + planes[:-1, :, 32:].float()).reshape(B * H * W, 64)
    assert rel(nchw(rec, B, H, W), ref) < 2.0 ** -16


# ---------------------------------------------------------------------------------------- A3. train-mode BatchNorm of the auto-encoder
def _bn_reference(x, w, b, rm, rv, res, go, act, training):
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if res is not None else None
    rmr, rvr = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(xr, rmr, rvr, wr, br, training, 0.1, 1e-5)
    y = act64(z, act)
    if rr is not None:
        y = y + rr
    g = off_kink(go.double(), z, act)
    y.backward(g)
    return y.detach(), xr.grad, wr.grad, br.grad, (rr.grad if rr is not None else None), rmr, rvr, g


# rows: 257 = one chunk of 256 + a last chunk of ONE row; 1000; 874 = 2 * 23 * 19; 10500 = 42 chunks (not a multiple of the 8 records
# colstats_final_kernel keeps in flight) with a 4-row tail.  Widths: 4, 64, 132 (33 float4 columns: a partial second column block), 528.
BN_CASES = [(257, 4, RELU), (257, 132, NONE), (1000, 64, LRELU), (1000, 528, RELU), (1000, 4, NONE), (874, 132, LRELU), (874, 64, NONE), (874, 528, RELU),
            (10500, 528, NONE), (10500, 4, RELU), (10500, 132, LRELU), (10500, 64, RELU)]


@pytest.mark.parametrize("rows,Fc,act", BN_CASES)
def test_batchnorm_train_multi_chunk(ops, dev, rows, Fc, act):
    """ops.norm_act(mode="bn", training=True) with the activations the auto-encoder uses (ReLU, LeakyReLU, none + residual) vs fp64
    F.batch_norm: y, dx, dw, db, d residual and the UPDATED running statistics (Chan merge over several 256-row chunks, the row tail of the
    last chunk, the n / (n - 1) unbiasing with n % 256 != 0) and num_batches_tracked"""
    seed = 400 + rows % 97 + Fc
    x, go = rn((rows, Fc), seed, 2.0) + 0.3, rn((rows, Fc), seed + 1)
    w, b = rn((Fc,), seed + 2).abs() + 0.5, rn((Fc,), seed + 3, 0.5)
    rm, rv = rn((Fc,), seed + 4, 0.1), rn((Fc,), seed + 5).abs() + 0.5
    res = rn((rows, Fc), seed + 6) if act == NONE else None
    y, dx, dw, db, dres, rmr, rvr, g = _bn_reference(x, w, b, rm, rv, res, go, act, True)
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    resd = res.to(dev).requires_grad_(True) if res is not None else None
    rmg, rvg, nbt = rm.to(dev), rv.to(dev), torch.full((1,), 3, device=dev, dtype=torch.int64)
    yd = ops.norm_act(xd, wd, bd, "bn", rows, True, rmg, rvg, act=act, residual=resd, num_batches_tracked=nbt)
    yd.backward(g.float().to(dev))
    assert rel(yd, y) < TOLV
    assert rel(rmg, rmr) < TOLV and rel(rvg, rvr) < TOLV and int(nbt) == 4
    assert rel(xd.grad, dx) < TOLG
    assert rel(wd.grad, dw) < TOLG and rel(bd.grad, db) < TOLG
    if res is not None:
        assert torch.equal(resd.grad.cpu(), g.float())


@pytest.mark.parametrize("rows,Fc,act", [(874, 132, RELU), (257, 64, NONE)])
def test_batchnorm_eval_const_stats(ops, dev, rows, Fc, act):
    """eval mode: the running statistics are constants (const_stats: no statistics terms in dx) and stay bit-unchanged"""
    x, go = rn((rows, Fc), 450, 2.0) + 0.3, rn((rows, Fc), 451)
    w, b = rn((Fc,), 452).abs() + 0.5, rn((Fc,), 453, 0.5)
    rm, rv = rn((Fc,), 454, 0.3), rn((Fc,), 455).abs() + 0.5
    res = rn((rows, Fc), 456) if act == NONE else None
    y, dx, dw, db, dres, rmr, rvr, g = _bn_reference(x, w, b, rm, rv, res, go, act, False)
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    resd = res.to(dev).requires_grad_(True) if res is not None else None
    rmg, rvg, nbt = rm.to(dev), rv.to(dev), torch.full((1,), 3, device=dev, dtype=torch.int64)
    yd = ops.norm_act(xd, wd, bd, "bn", rows, False, rmg, rvg, act=act, residual=resd, num_batches_tracked=nbt)
    yd.backward(g.float().to(dev))
    assert torch.equal(rmg.cpu(), rm) and torch.equal(rvg.cpu(), rv) and int(nbt) == 3
    assert rel(yd, y) < TOLV
    assert rel(xd.grad, dx) < TOLG and rel(wd.grad, dw) < TOLG and rel(bd.grad, db) < TOLG


@pytest.mark.parametrize("rows,Fc,offset", [(874, 132, 0.3), (257, 4, 0.3), (10500, 64, 0.3), (1000, 64, 1e3), (2300, 528, 1e3)])
def test_colstats_direct(dev, abi, rows, Fc, offset):
    """vptr_colstats / vptr_colstats_running through the C ABI, each optional pointer NULL in turn, vs fp64 mean / biased variance.  offset 1e3:
    x = 1e3 + N(0, 1) -- the pivoted one-pass sums must hold the variance where E[x^2] - E[x]^2 in fp32 would lose it entirely"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    x = rn((rows, Fc), 460) + offset
    xd = x.to(dev)
    mref, vref = x.double().mean(0), x.double().var(0, unbiased=False)
    nchunk = (rows + 255) // 256

    def bufs():
        return (torch.empty(Fc, device=dev), torch.empty(Fc, device=dev), torch.empty(Fc, device=dev), torch.empty(2 * Fc * nchunk, device=dev))
    mean, var, rstd, scratch = bufs()
    check(lib.vptr_colstats(ptr(xd), ptr(mean), ptr(var), ptr(rstd), 1e-5, ptr(scratch), rows, Fc, stream()), "vptr_colstats")
    assert rel(mean, mref) < TOLV and rel(var, vref) < TOLV and rel(rstd, (vref + 1e-5).rsqrt()) < TOLV
    mean2, var2, _, scratch = bufs()
    check(lib.vptr_colstats(ptr(xd), ptr(mean2), ptr(var2), None, 1e-5, ptr(scratch), rows, Fc, stream()), "vptr_colstats")
    assert torch.equal(mean2, mean) and torch.equal(var2, var)
    rm0, rv0 = rn((Fc,), 461, 0.2), rn((Fc,), 462).abs() + 0.5
    rm_ref = 0.7 * rm0.double() + 0.3 * mref
    rv_ref = 0.7 * rv0.double() + 0.3 * vref * rows / (rows - 1)
    for with_running, with_nbt, with_rstd in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
        mean3, var3, rstd3, scratch = bufs()
        rmg, rvg, nbt = rm0.to(dev), rv0.to(dev), torch.full((1,), 41, device=dev, dtype=torch.int64)
        check(lib.vptr_colstats_running(ptr(xd), ptr(mean3), ptr(var3), ptr(rstd3) if with_rstd else None, 1e-5, ptr(scratch), rows, Fc,
                                        ptr(rmg) if with_running else None, ptr(rvg) if with_running else None, 0.3, ptr(nbt) if with_nbt else None,
                                        stream()), "vptr_colstats_running")
        assert torch.equal(mean3, mean) and torch.equal(var3, var)
        if with_rstd:
            assert torch.equal(rstd3, rstd)
        if with_running:
            assert rel(rmg, rm_ref) < TOLV and rel(rvg, rv_ref) < TOLV
        else:
            assert torch.equal(rmg.cpu(), rm0) and torch.equal(rvg.cpu(), rv0)
        assert int(nbt) == (42 if with_nbt else 41)


@pytest.mark.parametrize("elems", [4, 1024 * 4 + 8, 2112 * 64])   # one float4; a second, partial round of the 1024-thread float4 loop; a K64 frame
@pytest.mark.parametrize("offset", [0.3, 1e3])   # (not 0: the mean of 135 168 standard normals is 0 +- 0.003, and a RELATIVE error of it says nothing)
def test_groupstats_direct(dev, abi, elems, offset):
    """vptr_groupstats through the C ABI vs fp64 mean / biased variance, rstd NULL and not; offset 1e3 as in test_colstats_direct"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    groups = 5
    x = rn((groups, elems), 470) + offset
    xd = x.to(dev)
    mean, var, rstd = torch.empty(groups, device=dev), torch.empty(groups, device=dev), torch.empty(groups, device=dev)
    check(lib.vptr_groupstats(ptr(xd), ptr(mean), ptr(var), ptr(rstd), 1e-5, groups, elems, stream()), "vptr_groupstats")
    mref, vref = x.double().mean(1), x.double().var(1, unbiased=False)
    assert rel(mean, mref) < TOLV and rel(var, vref) < TOLV and rel(rstd, (vref + 1e-5).rsqrt()) < TOLV
    mean2, var2 = torch.empty(groups, device=dev), torch.empty(groups, device=dev)
    check(lib.vptr_groupstats(ptr(xd), ptr(mean2), ptr(var2), None, 1e-5, groups, elems, stream()), "vptr_groupstats")
    assert torch.equal(mean2, mean) and torch.equal(var2, var)


# ------------------------------------------------------------------------------------------- A4. the small kernels through the C ABI
IM2COL_CASES = [(3, 1, 1, "zero"), (3, 1, 1, "reflect"), (3, 2, 1, "zero"), (3, 2, 1, "reflect"), (4, 2, 1, "zero"), (4, 1, 1, "zero"), (7, 1, 3, "reflect")]


@pytest.mark.parametrize("K,stride,pad,pad_mode", IM2COL_CASES)
@pytest.mark.parametrize("IH,IW", [(9, 7), (10, 6)])   # (10, 6) with 3 / 2 / 1: the ConvTranspose2d use -- "input" is the larger output-gradient grid, OH x OW the 5 x 3 layer input
def test_im2col_nhwc(ops, dev, abi, K, stride, pad, pad_mode, IH, IW):
    """vptr_im2col_nhwc == F.unfold of the (reflect-)padded input in (ky, kx, c) column order, bit for bit; vptr_im2col_nhwc_p16 == the P16 image of it"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    B, C = 2, 16
    x = rn((B, C, IH, IW), 500)
    ref = unfold_kkc(x.double(), K, K, stride, pad, pad_mode).float()
    OH, OW = (IH + 2 * pad - K) // stride + 1, (IW + 2 * pad - K) // stride + 1
    assert ref.shape == (B * OH * OW, K * K * C)
    xd = tokens(x).to(dev)
    out = torch.full(tuple(ref.shape), float("nan"), device=dev)
    check(lib.vptr_im2col_nhwc(ptr(xd), ptr(out), B, IH, IW, C, OH, OW, K, K, stride, pad, ops.PAD_MODES[pad_mode], stream()), "vptr_im2col_nhwc")
    assert torch.equal(out.cpu(), ref)
    out16 = torch.zeros_like(out)
    check(lib.vptr_im2col_nhwc_p16(ptr(xd), ptr(out16), B, IH, IW, C, OH, OW, K, K, stride, pad, ops.PAD_MODES[pad_mode], stream()), "vptr_im2col_nhwc_p16")
    assert torch.equal(out16.view(torch.int32), ops.to_p16(out).view(torch.int32))


@pytest.mark.parametrize("H,W,C,pad", [(5, 7, 8, 1), (2, 3, 4, 1), (3, 2, 4, 1), (4, 6, 8, 3), (8, 4, 4, 3), (16, 12, 132, 1)])   # H or W = pad + 1 included
def test_reflect_fold(dev, abi, H, W, C, pad):
    """vptr_reflect_fold == the autograd of F.pad(mode="reflect"), exactly: the inputs are multiples of 1/8, so every sum of up to nine of them is
    exact in fp32 whatever its order"""
    B = 3
    g = (rn((B, C, H + 2 * pad, W + 2 * pad), 510) * 8).round() / 8
    x = torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(F.pad(x, (pad,) * 4, mode="reflect"), x, g.double())
    assert torch.equal(reflect_fold_ref(g.double(), pad), ref)
    gd = tokens(g).to(dev)
    dx = torch.full((B * H * W, C), float("nan"), device=dev)
    abi.check(abi.lib.vptr_reflect_fold(abi.ptr(gd), abi.ptr(dx), B, H, W, C, pad, abi.stream()), "vptr_reflect_fold")
    assert torch.equal(nchw(dx, B, H, W).cpu(), ref.float())


@pytest.mark.parametrize("rows,C", [(700, 132), (1, 4), (513, 64)])   # C not a multiple of 128, rows not a multiple of 512
def test_bnrelu_bwd_separate_kernels(dev, abi, rows, C):
    """vptr_bnrelu_bwd and vptr_bnrelu_bwd_params vs autograd of y = relu(w * xhat + b), and vs vptr_bnrelu_bwd_fused on the same inputs"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    xh, dy = rn((rows, C), 520), rn((rows, C), 521)
    w, b, sc = rn((C,), 522).abs() + 0.5, rn((C,), 523, 0.3), rn((C,), 524).abs() + 0.2
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = torch.relu(xh.double() * wr + br)
    (y * dy.double()).sum().backward()
    yd, dyd, wg, bg, sg = y.detach().float().to(dev), dy.to(dev), w.to(dev), b.to(dev), sc.to(dev)
    dx, dw, db = torch.empty((rows, C), device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    check(lib.vptr_bnrelu_bwd(ptr(dyd), ptr(yd), ptr(sg), ptr(dx), rows, C, stream()), "vptr_bnrelu_bwd")
    check(lib.vptr_bnrelu_bwd_params(ptr(dyd), ptr(yd), ptr(wg), ptr(bg), ptr(dw), ptr(db), rows, C, stream()), "vptr_bnrelu_bwd_params")
    assert rel(dx, (y.detach() > 0).double() * dy.double() * sc.double()) < 1e-6
    assert rel(dw, wr.grad) < TOLV and rel(db, br.grad) < TOLV
    dx2, dw2, db2 = torch.empty((rows, C), device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    check(lib.vptr_bnrelu_bwd_fused(ptr(dyd), ptr(yd), ptr(sg), ptr(wg), ptr(bg), ptr(dx2), ptr(dw2), ptr(db2), rows, C, stream()), "vptr_bnrelu_bwd_fused")
    assert torch.equal(dx2, dx)
    assert rel(dw2, dw.double().cpu()) < TOLV and rel(db2, db.double().cpu()) < TOLV


@pytest.mark.parametrize("rows,C,div,mod", [(77, 10, 3, 5), (100, 48, 7, 4), (64, 3, 1, 9)])   # div * mod does not divide the row count
def test_rowscale(dev, abi, rows, C, div, mod):
    dy, rs = rn((rows, C), 530), rn((mod,), 531)
    dyd, rsd = dy.to(dev), rs.to(dev)
    dx = torch.empty((rows, C), device=dev)
    abi.check(abi.lib.vptr_rowscale(abi.ptr(dyd), abi.ptr(rsd), abi.ptr(dx), rows, C, div, mod, abi.stream()), "vptr_rowscale")
    idx = (torch.arange(rows) // div) % mod
    assert rel(dx, dy.double() * rs.double()[idx][:, None]) < 1e-7


@pytest.fixture(params=["default", "deterministic"])
def det_mode(request, ops):
    """vptr_colsum / vptr_rowmod_sum pick other launch geometries (one adder per destination) under ops.set_deterministic"""
    prev = ops.config.deterministic
    ops.set_deterministic(request.param == "deterministic")
    try:
        yield request.param
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("rows,C", [(777, 132), (777, 50), (5, 4), (300, 1030)])   # float4 kernel (C % 4 == 0) and the row-run kernel (C % 4 != 0)
def test_colsum(dev, abi, det_mode, rows, C):
    src, out0 = rn((rows, C), 540), rn((C,), 541)
    sd, out = src.to(dev), out0.to(dev)
    abi.check(abi.lib.vptr_colsum(abi.ptr(sd), abi.ptr(out), rows, C, abi.stream()), "vptr_colsum")
    assert rel(out, out0.double() + src.double().sum(0)) < TOLV      # accumulates into its destination


@pytest.mark.parametrize("rows,C,div,mod", [(43, 48, 1, 5), (104, 50, 1, 3), (67, 48, 3, 4), (1000, 264, 7, 5), (23, 8, 40, 2)])
def test_rowmod_sum(dev, abi, det_mode, rows, C, div, mod):
    """div == 1 fast path with 9 and 35 periods (not multiples of the 4 it unrolls, the last one partial); div > 1 with a row tail inside a run"""
    src = rn((rows, C), 550)
    sd, out = src.to(dev), torch.zeros((mod, C), device=dev)
    abi.check(abi.lib.vptr_rowmod_sum(abi.ptr(sd), abi.ptr(out), rows, C, div, mod, abi.stream()), "vptr_rowmod_sum")
    ref = torch.zeros((mod, C), dtype=torch.float64).index_add_(0, (torch.arange(rows) // div) % mod, src.double())
    assert rel(out, ref) < TOLV


@pytest.mark.parametrize("n", [10007, 4096, 3])
@pytest.mark.parametrize("nws", [1, 1024])
@pytest.mark.parametrize("shift", [0, 1])    # 1: a view that starts one float past a 16-byte boundary
def test_sumsq_ws(dev, abi, n, nws, shift):
    g = rn((n + 1,), 560)
    gd = g.to(dev)[shift:shift + n]
    ws, out = torch.full((nws,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    abi.check(abi.lib.vptr_sumsq_ws(abi.ptr(gd), n, abi.ptr(out), abi.ptr(ws), nws, abi.stream()), "vptr_sumsq_ws")
    assert rel(out, (g[shift:shift + n].double() ** 2).sum()) < TOLV


@pytest.mark.parametrize("act", [NONE, RELU, LRELU])
@pytest.mark.parametrize("C,p16", [(10, False), (48, False), (48, True)])   # scalar kernel (C % 4 != 0), float4 kernel, float4 kernel with a P16 output
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_act_bwd(ops, dev, abi, act, C, p16, p):
    """vptr_act_bwd: dx = dy * alpha * dropout(site) * rowscale[(row / div) % mod] * act'(h), the dropout mask regenerated through vptr_dropout"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    rows, div, mod, alpha, site = 123, 3, 4, 0.7, 11
    dy, h, rs = rn((rows, C), 570), rn((rows, C), 571), rn((mod,), 572).abs() + 0.5
    dyd, hd, rsd = dy.to(dev), h.to(dev), rs.to(dev)
    mask = torch.ones((rows, C), dtype=torch.float64)
    seed = None
    if p > 0:
        ops.manual_seed(dev, 97531)
        seed = ops.new_seed_scope(dev)
        ones, md = torch.ones(rows * C, device=dev), torch.empty(rows * C, device=dev)
        check(lib.vptr_dropout(ptr(ones), ptr(md), rows * C, p, ptr(seed), site, stream()), "vptr_dropout")
        mask = md.reshape(rows, C).double().cpu()
        assert 0.05 < float((mask == 0).double().mean()) < 0.15
    dx = torch.full((rows, C), float("nan"), device=dev)
    check(lib.vptr_act_bwd(ptr(dyd), ptr(hd), ptr(dx), rows, C, act, alpha, ptr(rsd), div, mod, p, ptr(seed), site, int(p16), stream()), "vptr_act_bwd")
    slope = torch.ones_like(h.double()) if act == NONE else torch.where(h > 0, 1.0, 0.0 if act == RELU else 0.2).double()
    ref = dy.double() * alpha * mask * rs.double()[(torch.arange(rows) // div) % mod][:, None] * slope
    if p16:
        assert rel(ops.p16_decode(dx), ref) < 2.0 ** -16
    else:
        assert rel(dx, ref) < 1e-6
