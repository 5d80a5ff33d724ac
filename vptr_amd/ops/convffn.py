"""Conv-FFN pieces: normalise + activation (BatchNorm2d / LayerNorm((F,H,W))), depthwise 3x3, and their fused form."""

import torch

from .._lib import check, lib, ptr, stream
from .core import ACT_GELU, _c, _direct_apply, config, seed_tensor
from .wgrad import defer_partial_reduce
from .grads import _bw_zeros, flat_grad_for
from .linear import frame_stats_ok


# ------------------------------------------------------------------------------------------------------------------
# conv-FFN pieces
# ------------------------------------------------------------------------------------------------------------------
def _norm_act_backward(dy, x, w, b, mean, rstd, rowscale, HW, per_col, act, const_stats, p, seed, site, rs_div, rs_mod, dx_p16, sums_only=False):
    """backward of y = dropout(act(norm(x) * w + b)) (* rowscale): (dx, dw, db); dw / db are None when the affine gradients were accumulated
    in place (flat gradient slab) -- directly or through the backward pass's deferred partial-sum reduction.
    sums_only (LayerNorm((F,H,W)) mode without a row scale): no dx pass -- the first result is the scratch buffer whose head holds the frame
    sums s1[f], s2[f] for the kernel that applies the dx arithmetic itself (vptr_dwconv3x3_norm_bwd)"""
    rows, F = x.shape
    dx = None if sums_only else torch.empty_like(x)
    sw, sb = flat_grad_for(w), flat_grad_for(b)   # accumulate straight into the flat gradient slab when both live there
    in_slab = sw is not None and sb is not None
    dw, db = (sw, sb) if in_slab else (_bw_zeros(w.shape, w.device), _bw_zeros(b.shape, b.device))
    frames = rows // HW
    scratch = torch.empty((max(2 * F, 2 * frames * (1 + 4 * ((HW * F // 4 + 255) // 256))),), device=x.device, dtype=torch.float32)
    nparts = lib.vptr_norm_act_bwd_partials(rows, F, HW, int(per_col)) if (in_slab and config.defer_ln_param_grads) else 0
    if sums_only:
        if per_col or rowscale is not None or const_stats:
            raise RuntimeError("norm_act backward: the sums-only form belongs to the LayerNorm((F,H,W)) mode without a row scale")
        part = torch.empty((nparts, 2, HW * F), device=x.device, dtype=torch.float32) if nparts > 0 else None
        check(lib.vptr_norm_act_bwd_sums(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(dw), ptr(db), ptr(scratch), rows, F, HW, act, p,
                                         ptr(seed), site, ptr(part), stream()), "vptr_norm_act_bwd_sums")
        if nparts > 0:
            defer_partial_reduce(part, sw, sb, nparts, HW * F)
        dx = scratch
    elif nparts > 0:
        # affine gradients with an in-place destination: per-chunk partial sums, added by the backward pass's one reduction launch
        part = torch.empty((nparts, 2, HW * F), device=x.device, dtype=torch.float32)
        check(lib.vptr_norm_act_bwd_deferred(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(dx), ptr(scratch), rows, F, HW,
                                             act, int(const_stats), p, ptr(seed), site, ptr(rowscale), rs_div, rs_mod, int(dx_p16),
                                             ptr(part), stream()), "vptr_norm_act_bwd_deferred")
        defer_partial_reduce(part, sw, sb, nparts, HW * F)
    else:
        check(lib.vptr_norm_act_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(dx), ptr(dw), ptr(db),
                                    ptr(scratch), rows, F, HW, int(per_col), act, int(const_stats), p,
                                    ptr(seed), site, ptr(rowscale), rs_div, rs_mod, int(dx_p16),
                                    stream()), "vptr_norm_act_bwd")
    if in_slab:
        dw = db = None
    return dx, dw, db


class _NormActFn(torch.autograd.Function):
    """y = dropout(act(norm(x) * w + b)) on channel-last [rows, F].

    mode 'bn'   : BatchNorm2d semantics (VidHRFormer_modules.py:397-419 with AR_model=False); batch statistics when
                  `training`, running statistics otherwise; running stats updated in place (momentum 0.1, unbiased var).
    mode 'ln'   : LayerNorm((F,H,W)) per frame; w, b given channel-last as [HW, F].
    """

    @staticmethod
    def forward(ctx, x, w, b, running_mean, running_var, mode, HW, training, act, eps, p, site, momentum, rowscale, rs_div,
                rs_mod, residual, out_p16, dx_p16, num_batches_tracked, raw_stats=None):
        x, w, b = _c(x), _c(w), _c(b)
        residual = _c(residual) if residual is not None else None
        rows, F = x.shape
        dev = x.device
        per_col = mode == "bn"
        const_stats = False
        if per_col:
            if training:
                mean = torch.empty((F,), device=dev, dtype=torch.float32)
                var = torch.empty_like(mean)
                nchunk = (rows + 255) // 256
                scratch = torch.empty((2 * F * nchunk,), device=dev, dtype=torch.float32)
                rstd = torch.empty_like(mean)
                # batch statistics + BatchNorm2d's running-statistics / num_batches_tracked bookkeeping in one launch pair
                check(lib.vptr_colstats_running(ptr(x), ptr(mean), ptr(var), ptr(rstd), eps, ptr(scratch), rows, F, ptr(running_mean),
                                                ptr(running_var), momentum, ptr(num_batches_tracked), stream()), "vptr_colstats_running")
            else:
                mean, var = running_mean, running_var
                rstd = torch.rsqrt(var + eps)
                const_stats = True
        else:
            frames = rows // HW
            mean = torch.empty((frames,), device=dev, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            if raw_stats is None:
                var = torch.empty_like(mean)
                check(lib.vptr_groupstats(ptr(x), ptr(mean), ptr(var), ptr(rstd), eps, frames, HW * F, stream()), "vptr_groupstats")
            # else: x's producer accumulated the per-frame sums; the normalise kernel derives mean / rstd and writes them for backward
        if raw_stats is not None and per_col:
            raise RuntimeError("norm_act: raw_stats belong to the LayerNorm((F,H,W)) mode")
        y = torch.empty_like(x)
        ctx.seed = seed_tensor(dev) if p > 0 else None
        check(lib.vptr_norm_act_fwd(ptr(x), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(y), rows, F, HW, int(per_col), act, p,
                                    ptr(ctx.seed), site, ptr(rowscale), rs_div, rs_mod,
                                    ptr(residual), int(out_p16), ptr(raw_stats), eps, stream()), "vptr_norm_act_fwd")
        ctx.save_for_backward(x, w, b, mean, rstd, rowscale)
        ctx.cfg = (HW, per_col, act, const_stats, p, site, rs_div, rs_mod, residual is not None, dx_p16)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, mean, rstd, rowscale = ctx.saved_tensors
        HW, per_col, act, const_stats, p, site, rs_div, rs_mod, has_res, dx_p16 = ctx.cfg
        dy = _c(dy)
        dx, dw, db = _norm_act_backward(dy, x, w, b, mean, rstd, rowscale, HW, per_col, act, const_stats, p, ctx.seed, site, rs_div, rs_mod, dx_p16)
        dres = dy if has_res else None
        return dx, dw, db, None, None, None, None, None, None, None, None, None, None, None, None, None, dres, None, None, None, None


_NormActFn_apply = _direct_apply(_NormActFn)


def norm_act(x, w, b, mode, HW, training, running_mean=None, running_var=None, act=ACT_GELU, eps=1e-5, dropout_p=0.0, site=0,
             momentum=0.1, rowscale=None, rs_div=1, rs_mod=1, residual=None, out_p16=False, dx_p16=False, num_batches_tracked=None,
             raw_stats=None):
    """y = rowscale * dropout(act(norm(x)*w + b)) + residual  (one elementwise pass; see _NormActFn).
    out_p16: y is written as a P16 tensor (it only feeds a GEMM); dx_p16: the gradient w.r.t. x is returned as a P16 tensor (x is
    the output of a linear(..., dy_p16=True) and nothing else)."""
    return _NormActFn_apply(x, w, b, running_mean, running_var, mode, int(HW), bool(training), int(act), float(eps),
                            float(dropout_p), int(site), float(momentum), rowscale, int(rs_div), int(rs_mod), residual,
                            bool(out_p16), bool(dx_p16), num_batches_tracked, raw_stats)


class _DWConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w9, b, frames, H, W, frame_stats=None):
        x, w9 = _c(x), _c(w9)
        F = x.shape[1]
        y = torch.empty_like(x)
        check(lib.vptr_dwconv3x3_fwd(ptr(x), ptr(w9), ptr(b), ptr(y), frames, H, W, F, ptr(frame_stats), stream()), "vptr_dwconv3x3_fwd")
        ctx.save_for_backward(x, w9)
        ctx.cfg = (frames, H, W)
        ctx.bias_ref = b.detach() if b is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w9 = ctx.saved_tensors
        frames, H, W = ctx.cfg
        dy = _c(dy)
        F = x.shape[1]
        dx = torch.empty_like(x)
        sw, sb = flat_grad_for(w9), flat_grad_for(ctx.bias_ref)
        in_slab = sw is not None and sb is not None
        dw9 = sw if in_slab else _bw_zeros(w9.shape, w9.device)
        db = sb if in_slab else _bw_zeros((F,), x.device)
        check(lib.vptr_dwconv3x3_bwd(ptr(dy), ptr(x), ptr(w9), ptr(dx), ptr(dw9), ptr(db), frames, H, W, F, stream()),
              "vptr_dwconv3x3_bwd")
        if in_slab:
            dw9 = db = None
        return dx, dw9, db, None, None, None, None


_DWConvFn_apply = _direct_apply(_DWConvFn)


def dwconv3x3(x, weight, bias, frames, H, W, frame_stats=None):
    """Depthwise 3x3 (pad 1) on channel-last x [frames*H*W, F]; weight is the PyTorch parameter [F,1,3,3].  frame_stats: see linear."""
    F = x.shape[1]
    w9 = weight.reshape(F, 9).t().contiguous()  # tap-major [9, F] for coalesced reads
    return _DWConvFn_apply(x, w9, bias, int(frames), int(H), int(W), frame_stats)


def norm_dwconv_ok(rows, HW, F, H, W):
    """can the conv-FFN's first normalisation + activation run inside the depthwise kernel's load path? (LayerNorm((F,H,W)) statistics
    delivered by fc1's epilogue, x pairs of a channel quad in adjacent lanes, whole waves inside one frame)"""
    W2 = W // 2
    # where it pays (profiles/r06_cfg4 / cfg5_kernel_stats.md): maps of at most 64 pixels (16 KB LDS slabs: four workgroups per CU) and hidden tensors
    # that stay in the 256 MB Infinity Cache -- on 16 x 16 maps (KTH 128 x 128: 164 us against 48 + 48) and on 251 MB tensors (BAIR, 29 frames per
    # clip: 175 against 65 + 86) the two-launch form is faster; VPTR_FUSED_NORM_DW=2 forces the fused launch wherever it is valid
    if config.fused_norm_dwconv_mode != 2 and (H * W > 64 or rows * F * 4 > (128 << 20)):
        return False
    return (config.fused_norm_dwconv_mode != 0 and not config.deterministic and frame_stats_ok(rows, HW, F, W) and W % 2 == 0 and W2 >= 1 and 16 % W2 == 0
            and H * W == HW)


def norm_dwconv_bwd_ok(HW, F, H, W):
    """where norm_dwconv_ok() holds: can the backward pass between norm2 and the depthwise 3x3 run as vptr_norm_act_bwd_sums +
    vptr_dwconv3x3_norm_bwd (the gradient w.r.t. the depthwise output never written)?  Geometry of that kernel; the deterministic mode keeps the
    three launches (the kernel's workgroups meet in atomics); config.fused_convffn_bwd = False switches the route off (tests, A/B by hand)."""
    W2 = W // 2
    return (config.fused_convffn_bwd and not config.deterministic and H * W == HW and HW <= 64 and F % 64 == 0 and W % 2 == 0 and W2 >= 1
            and 16 % W2 == 0 and (W2 * (F // 4)) % 64 == 0)


fused_bwd_calls = 0   # backward passes that took vptr_dwconv3x3_norm_bwd (tests assert on the route with it)


class _NormDWConvFn(torch.autograd.Function):
    """y = dw3x3(act(LayerNorm((F,H,W))(x))) with the normalisation + activation applied in the depthwise kernel's load path
    (VidHRFormer_modules.py:430-434).  x: fc1's raw output, raw_stats: its per-frame sums (fc1's epilogue).  The activated tensor is kept
    only as an fp16 side copy -- the x operand of the depthwise weight gradient; the backward pass runs the depthwise data / weight
    gradients and then the ordinary two-phase backward of the normalisation on (dy_act, x)."""

    @staticmethod
    def forward(ctx, x, aw, ab, w9, b9, frames, H, W, raw_stats, frame_stats, act, eps, dx_p16):
        x, aw, ab, w9 = _c(x), _c(aw), _c(ab), _c(w9)
        rows, F = x.shape
        y = torch.empty_like(x)
        ah = torch.empty((rows, F), device=x.device, dtype=torch.float16) if any(ctx.needs_input_grad) else None   # no-grad forward: not written
        mean = torch.empty((frames,), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        check(lib.vptr_dwconv3x3_norm_fwd(ptr(x), ptr(raw_stats), ptr(aw), ptr(ab), eps, act, ptr(w9), ptr(b9), ptr(y), ptr(ah), ptr(mean), ptr(rstd),
                                          frames, H, W, F, ptr(frame_stats), stream()), "vptr_dwconv3x3_norm_fwd")
        ctx.save_for_backward(x, aw, ab, w9, mean, rstd, ah)
        ctx.cfg = (frames, H, W, act, dx_p16)
        ctx.bias_ref = b9.detach() if b9 is not None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, aw, ab, w9, mean, rstd, ah = ctx.saved_tensors
        frames, H, W, act, dx_p16 = ctx.cfg
        dy = _c(dy)
        F = x.shape[1]
        da = torch.empty_like(x)
        sw, sb = flat_grad_for(w9), flat_grad_for(ctx.bias_ref)
        in_slab = sw is not None and sb is not None
        dw9 = sw if in_slab else _bw_zeros(w9.shape, w9.device)
        db9 = sb if in_slab else _bw_zeros((F,), x.device)
        check(lib.vptr_dwconv3x3_bwd_xh(ptr(dy), ptr(ah), ptr(w9), ptr(da), ptr(dw9), ptr(db9), frames, H, W, F, stream()), "vptr_dwconv3x3_bwd_xh")
        if in_slab:
            dw9 = db9 = None
        dx, daw, dab = _norm_act_backward(da, x, aw, ab, mean, rstd, None, H * W, False, act, False, 0.0, None, 0, 1, 1, dx_p16)
        return dx, daw, dab, dw9, db9, None, None, None, None, None, None, None, None


_NormDWConvFn_apply = _direct_apply(_NormDWConvFn)


class _NormDWConvNormFn(torch.autograd.Function):
    """out = dropout(act2(norm2(dw3x3(act1(norm1(x)))))) with both LayerNorm((F,H,W)): _NormDWConvFn and norm2's _NormActFn as ONE node, so that
    the backward pass can skip the gradient w.r.t. the depthwise output.  Forward: the two launches of the two-node form, unchanged.
    Backward: norm2's affine gradients and frame sums (vptr_norm_act_bwd_sums), then norm2's dx arithmetic in the load path of the depthwise
    data / weight / bias gradients (vptr_dwconv3x3_norm_bwd), then norm1's ordinary backward on (da, x).  With config.fused_convffn_bwd off or the
    deterministic mode on AT BACKWARD TIME the node runs the three launches of the two-node form instead."""

    @staticmethod
    def forward(ctx, x, aw, ab, w9, b9, w2, b2, frames, H, W, raw_stats, frame_stats, act1, eps1, act2, eps2, p, site, out_p16, dx_p16):
        x, aw, ab, w9, w2, b2 = _c(x), _c(aw), _c(ab), _c(w9), _c(w2), _c(b2)
        rows, F = x.shape
        dev = x.device
        y2 = torch.empty_like(x)
        ah = torch.empty((rows, F), device=dev, dtype=torch.float16) if any(ctx.needs_input_grad) else None   # no-grad forward: not written
        mean1 = torch.empty((frames,), device=dev, dtype=torch.float32)
        rstd1, mean2, rstd2 = torch.empty_like(mean1), torch.empty_like(mean1), torch.empty_like(mean1)
        check(lib.vptr_dwconv3x3_norm_fwd(ptr(x), ptr(raw_stats), ptr(aw), ptr(ab), eps1, act1, ptr(w9), ptr(b9), ptr(y2), ptr(ah), ptr(mean1), ptr(rstd1),
                                          frames, H, W, F, ptr(frame_stats), stream()), "vptr_dwconv3x3_norm_fwd")
        out = torch.empty_like(x)
        ctx.seed = seed_tensor(dev) if p > 0 else None
        check(lib.vptr_norm_act_fwd(ptr(y2), ptr(mean2), ptr(rstd2), ptr(w2), ptr(b2), ptr(out), rows, F, H * W, 0, act2, p, ptr(ctx.seed), site,
                                    None, 1, 1, None, int(out_p16), ptr(frame_stats), eps2, stream()), "vptr_norm_act_fwd")
        ctx.save_for_backward(x, aw, ab, w9, mean1, rstd1, ah, y2, w2, b2, mean2, rstd2)
        ctx.cfg = (frames, H, W, act1, act2, p, site, dx_p16)
        ctx.bias_ref = b9.detach() if b9 is not None else None
        return out

    @staticmethod
    def backward(ctx, dy):
        global fused_bwd_calls
        x, aw, ab, w9, mean1, rstd1, ah, y2, w2, b2, mean2, rstd2 = ctx.saved_tensors
        frames, H, W, act1, act2, p, site, dx_p16 = ctx.cfg
        dy = _c(dy)
        F = x.shape[1]
        # the switches are read again here: a node built before set_deterministic(True) / fused_convffn_bwd = False takes the three launches
        fused = config.fused_convffn_bwd and not config.deterministic
        g2, dw2, db2 = _norm_act_backward(dy, y2, w2, b2, mean2, rstd2, None, H * W, False, act2, False, p, ctx.seed, site, 1, 1, False, sums_only=fused)
        da = torch.empty_like(x)
        sw, sb = flat_grad_for(w9), flat_grad_for(ctx.bias_ref)
        in_slab = sw is not None and sb is not None
        dw9 = sw if in_slab else _bw_zeros(w9.shape, w9.device)
        db9 = sb if in_slab else _bw_zeros((F,), x.device)
        if fused:   # g2: the frame sums only
            check(lib.vptr_dwconv3x3_norm_bwd(ptr(dy), ptr(y2), ptr(mean2), ptr(rstd2), ptr(w2), ptr(b2), ptr(g2), act2, p, ptr(ctx.seed), site, ptr(ah),
                                              ptr(w9), ptr(da), ptr(dw9), ptr(db9), frames, H, W, F, 0, stream()), "vptr_dwconv3x3_norm_bwd")
            fused_bwd_calls += 1
        else:
            check(lib.vptr_dwconv3x3_bwd_xh(ptr(g2), ptr(ah), ptr(w9), ptr(da), ptr(dw9), ptr(db9), frames, H, W, F, stream()), "vptr_dwconv3x3_bwd_xh")
        if in_slab:
            dw9 = db9 = None
        dx, daw, dab = _norm_act_backward(da, x, aw, ab, mean1, rstd1, None, H * W, False, act1, False, 0.0, None, 0, 1, 1, dx_p16)
        return dx, daw, dab, dw9, db9, dw2, db2, None, None, None, None, None, None, None, None, None, None, None, None, None


_NormDWConvNormFn_apply = _direct_apply(_NormDWConvNormFn)


def norm_dwconv3x3_norm(x, aff_w, aff_b, weight, bias, aff_w2, aff_b2, frames, H, W, raw_stats, frame_stats, act=ACT_GELU, eps=1e-5, act2=ACT_GELU,
                        eps2=1e-5, dropout_p=0.0, site=0, out_p16=False, dx_p16=False):
    """norm_dwconv3x3 followed by norm_act(..., "ln", raw_stats=frame_stats) as one autograd node (where norm_dwconv_ok() and norm_dwconv_bwd_ok()
    hold): same forward launches, a backward pass without the gradient tensor between the two.  aff_w2 / aff_b2: norm2's affine, channel-last
    [H*W, F]; frame_stats (required): the depthwise kernel accumulates norm2's per-frame sums there."""
    if frame_stats is None or raw_stats is None:
        raise RuntimeError("norm_dwconv3x3_norm: both normalisations take their statistics from their producers' per-frame sums")
    F = x.shape[1]
    w9 = weight.reshape(F, 9).t().contiguous()
    return _NormDWConvNormFn_apply(x, aff_w, aff_b, w9, bias, aff_w2, aff_b2, int(frames), int(H), int(W), raw_stats, frame_stats, int(act), float(eps),
                                   int(act2), float(eps2), float(dropout_p), int(site), bool(out_p16), bool(dx_p16))


def norm_dwconv3x3(x, aff_w, aff_b, weight, bias, frames, H, W, raw_stats, frame_stats=None, act=ACT_GELU, eps=1e-5, dx_p16=False):
    """dw3x3(act(LayerNorm((F,H,W))(x))) in one launch (norm_dwconv_ok() decides where): aff_w / aff_b channel-last [H*W, F], weight the
    PyTorch depthwise parameter [F,1,3,3], raw_stats the per-frame sums of x from its producer, frame_stats as in dwconv3x3."""
    F = x.shape[1]
    w9 = weight.reshape(F, 9).t().contiguous()
    return _NormDWConvFn_apply(x, aff_w, aff_b, w9, bias, int(frames), int(H), int(W), raw_stats, frame_stats, int(act), float(eps), bool(dx_p16))
