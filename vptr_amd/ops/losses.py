"""Fused loss kernels: MSE + GDL, the reconstruction losses with temporal weights / L1 / a GDL exponent, the adversarial losses, BiPatchNCE."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream
from .core import _c


# ------------------------------------------------------------------------------------------------------------------
# losses of the train steps as plain kernel launches (csrc/losses.hip): no ATen reductions (-> no memset nodes) in a captured step
# ------------------------------------------------------------------------------------------------------------------
class _MseGdlFn(torch.autograd.Function):
    """(MSELoss()(gt, pred), GDL(alpha=1)(gt, pred)) of model/criterion.py:105-132,134-204 in two launches (partials + fixed-order
    sum); backward: ONE elementwise launch that takes both upstream gradients as device scalars."""

    @staticmethod
    def forward(ctx, pred, gt):
        _lib.require_cuda(pred, gt)
        if pred.shape != gt.shape or pred.dim() < 3:
            raise RuntimeError("mse_gdl: pred %s and gt %s must share a [..., H, W] shape" % (tuple(pred.shape), tuple(gt.shape)))
        pred, gt = _c(pred), _c(gt)
        H, W = pred.shape[-2], pred.shape[-1]
        planes = pred.numel() // (H * W)
        scratch = torch.empty(planes * ((H + 15) // 16) * 3, device=pred.device, dtype=torch.float32)
        mse = torch.empty((), device=pred.device, dtype=torch.float32)
        gdl = torch.empty((), device=pred.device, dtype=torch.float32)
        check(lib.vptr_mse_gdl_fwd(ptr(pred), ptr(gt), ptr(scratch), ptr(mse), ptr(gdl), planes, H, W, stream()), "vptr_mse_gdl_fwd")
        ctx.save_for_backward(pred, gt)
        return mse, gdl

    @staticmethod
    def backward(ctx, g_mse, g_gdl):
        pred, gt = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("mse_gdl: the target (gt) is data; it has no gradient path here")
        H, W = pred.shape[-2], pred.shape[-1]
        dpred = torch.empty_like(pred)
        check(lib.vptr_mse_gdl_bwd(ptr(pred), ptr(gt), ptr(_c(g_mse)), ptr(_c(g_gdl)), ptr(dpred), pred.numel() // (H * W), H, W, stream()),
              "vptr_mse_gdl_bwd")
        return dpred, None


def mse_gdl(pred, gt):
    """-> (mse, gdl) 0-dim device tensors; replaces MSELoss()(gt, pred) and GDL(alpha=1)(gt, pred) (no temporal weights, no norm_dim)"""
    return _MseGdlFn.apply(pred, gt)


class _ReconLossFn(torch.autograd.Function):
    """(MSELoss(w)(gt, pred), L1Loss(w)(gt, pred), GDL(alpha, w_gdl)(gt, pred)) of model/criterion.py:76-204 (csrc/recon_loss.hip): two
    launches forward, ONE elementwise launch backward that takes the three upstream gradients as device scalars.  A term nobody
    differentiates hands the backward no tensor (set_materialize_grads(False)): its scalar is NULL = 0, no fill launch is issued."""

    @staticmethod
    def forward(ctx, pred, gt, w_point, w_gdl, alpha, ppf, T):
        H, W = pred.shape[-2], pred.shape[-1]
        planes = pred.numel() // (H * W)
        scratch = torch.empty(planes * ((H + 15) // 16) * 4, device=pred.device, dtype=torch.float32)
        out3 = torch.empty(3, device=pred.device, dtype=torch.float32)
        check(lib.vptr_recon_loss_fwd(ptr(pred), ptr(gt), ptr(w_point), ptr(w_gdl), ptr(scratch), ptr(out3), planes, ppf, T, H, W, alpha, stream()),
              "vptr_recon_loss_fwd")
        ctx.save_for_backward(pred, gt)
        ctx.weights = (w_point, w_gdl)            # owned by the caller and read by address at every launch: not a saved tensor (no version check)
        ctx.cfg = (planes, ppf, T, H, W, alpha)
        ctx.set_materialize_grads(False)
        mse, l1, gdl = out3.unbind(0)
        return mse, l1, gdl

    @staticmethod
    def backward(ctx, g_mse, g_l1, g_gdl):
        pred, gt = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("recon_losses: the target (gt) is data; it has no gradient path here")
        planes, ppf, T, H, W, alpha = ctx.cfg
        w_point, w_gdl = ctx.weights
        dpred = torch.empty_like(pred)
        gs = [None if g is None else _c(g) for g in (g_mse, g_l1, g_gdl)]
        check(lib.vptr_recon_loss_bwd(ptr(pred), ptr(gt), ptr(w_point), ptr(w_gdl), ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(dpred), planes, ppf, T,
                                      H, W, alpha, stream()), "vptr_recon_loss_bwd")
        return dpred, None, None, None, None, None, None


def _time_weight(w, name, T, device):
    if w is None:
        return None
    if not isinstance(w, torch.Tensor) or not w.is_cuda or w.device != device:
        raise ValueError("recon_losses: %s must be a tensor on %s (the kernels read it by address)" % (name, device))
    if w.dtype != torch.float32 or w.dim() != 1 or w.numel() != T or not w.is_contiguous():
        raise ValueError("recon_losses: %s must be a contiguous fp32 vector of length %d (got %s %s)" % (name, T, w.dtype, tuple(w.shape)))
    return w


def recon_losses(pred, gt, w_point=None, w_gdl=None, gdl_alpha=1.0, time_dim=1):
    """-> (mse, l1, gdl) 0-dim device tensors: MSELoss(temporal_weight=w_point)(gt, pred), L1Loss(temporal_weight=w_point)(gt, pred) and
    GDL(alpha=gdl_alpha, temporal_weight=w_gdl)(gt, pred) of model/criterion.py (no norm_dim) on (N, T, C, H, W) or (N, T, TP, C, H, W)
    tensors.  The weights are fp32 device vectors of length shape[time_dim] (None: 1), read by address at every launch -- rewriting one
    in place changes the next call, also inside a captured graph.  gdl_alpha: finite, >= 1.  gt gets no gradient."""
    _lib.require_cuda(pred, gt)
    if pred.shape != gt.shape or pred.dim() not in (5, 6):
        raise RuntimeError("recon_losses: pred %s and gt %s must share a 5-D or 6-D [N, T, ..., H, W] shape" % (tuple(pred.shape), tuple(gt.shape)))
    if not 0 <= time_dim < pred.dim() - 2:
        raise ValueError("recon_losses: time_dim %r is no leading dimension of %s" % (time_dim, tuple(pred.shape)))
    alpha = float(gdl_alpha)
    if not (alpha >= 1.0 and alpha != float("inf")):
        raise ValueError("recon_losses: gdl_alpha must be finite and >= 1 (got %r)" % (gdl_alpha,))
    T = pred.shape[time_dim]
    ppf = 1
    for s in pred.shape[time_dim + 1:-2]:
        ppf *= s
    w_point, w_gdl = _time_weight(w_point, "w_point", T, pred.device), _time_weight(w_gdl, "w_gdl", T, pred.device)
    return _ReconLossFn.apply(_c(pred), _c(gt), w_point, w_gdl, alpha, ppf, T)


# ------------------------------------------------------------------------------------------------------------------
# adversarial losses (csrc/gan_loss.hip, include/vptr_hip_gan.h): GANLoss of model/criterion.py as fixed-order kernels
# ------------------------------------------------------------------------------------------------------------------
GAN_MODES = {"vanilla": 0, "lsgan": 1, "wgangp": 2}
GAN_CHUNK = 2048   # elements per forward workgroup: the scratch holds one float per chunk of each tensor


def _elem_stride(t):
    """the one stride (in elements) between consecutive logical elements of t, or None when t has no such stride: a contiguous tensor
    gives 1, a channel slice y[:, :1] of a [R, 4] buffer gives 4"""
    dims = [(n, s) for n, s in zip(t.shape, t.stride()) if n != 1]
    if not dims:
        return 1
    for (_, s), (n1, s1) in zip(dims[:-1], dims[1:]):
        if s != s1 * n1:
            return None
    return dims[-1][1] if dims[-1][1] >= 1 else None


def _gan_operand(x, name):
    """-> (the tensor the kernel reads in place, its element stride)"""
    if x.dtype != torch.float32:
        raise RuntimeError("%s: fp32 logits expected (got %s)" % (name, x.dtype))
    if x.numel() < 1:
        raise RuntimeError("%s: at least one logit expected (got shape %s)" % (name, tuple(x.shape)))
    s = _elem_stride(x)
    return (x, s) if s is not None else (x.contiguous(), 1)


def _gan_cfg(name, mode, real_label, fake_label, coef=1.0):
    if mode not in GAN_MODES:
        raise ValueError("%s: mode must be one of %s (got %r)" % (name, sorted(GAN_MODES), mode))
    vals = tuple(float(v) for v in (real_label, fake_label, coef))
    if any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        raise ValueError("%s: real_label, fake_label and coef must be finite (got %r)" % (name, vals))
    return (GAN_MODES[mode],) + vals


class _GanLossFn(torch.autograd.Function):
    """GANLoss(mode)(xa, a_is_real) -- and, with an xb, GANLoss(mode)(xb, b_is_real) and coef * (their sum) -- in two launches forward
    and ONE elementwise launch backward that takes the upstream gradients of the three outputs as device scalars and forms
    (g + coef * g_total) / n in the kernel.  An output nobody differentiates hands the backward no tensor
    (set_materialize_grads(False)): its scalar is NULL = 0."""

    @staticmethod
    def forward(ctx, xa, sa, a_is_real, xb, sb, b_is_real, cfg):
        mode, real_label, fake_label, coef = cfg
        na, nb = xa.numel(), (0 if xb is None else xb.numel())
        scratch = torch.empty(-(-na // GAN_CHUNK) - (-nb // GAN_CHUNK), device=xa.device, dtype=torch.float32)
        out3 = torch.empty(3, device=xa.device, dtype=torch.float32)
        check(lib.vptr_gan_loss_fwd(ptr(xa), na, sa, int(a_is_real), ptr(xb), nb, sb, int(b_is_real), mode, real_label, fake_label, coef,
                                    ptr(scratch), ptr(out3), stream()), "vptr_gan_loss_fwd")
        ctx.save_for_backward(xa, xb)
        ctx.cfg = (sa, int(a_is_real), sb, int(b_is_real)) + cfg
        ctx.set_materialize_grads(False)
        la, lb, total = out3.unbind(0)
        return la, lb, total

    @staticmethod
    def backward(ctx, g_a, g_b, g_total):
        xa, xb = ctx.saved_tensors
        sa, a_is_real, sb, b_is_real, mode, real_label, fake_label, coef = ctx.cfg
        dxa = torch.empty(xa.shape, device=xa.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dxb = torch.empty(xb.shape, device=xb.device, dtype=torch.float32) if (xb is not None and ctx.needs_input_grad[3]) else None
        gs = [None if g is None else _c(g) for g in (g_a, g_b, g_total)]
        check(lib.vptr_gan_loss_bwd(ptr(xa), xa.numel(), sa, a_is_real, ptr(dxa), ptr(xb), 0 if xb is None else xb.numel(), sb, b_is_real, ptr(dxb),
                                    mode, real_label, fake_label, coef, ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), stream()), "vptr_gan_loss_bwd")
        return dxa, None, None, dxb, None, None, None


def gan_loss(logits, target_is_real, mode="vanilla", real_label=1.0, fake_label=0.0):
    """-> 0-dim device tensor: GANLoss(mode, real_label, fake_label)(logits, target_is_real) of model/criterion.py.  A contiguous tensor,
    or a view with one uniform element stride such as y[:, :1], is read in place; anything else is made contiguous first."""
    _lib.require_cuda(logits)
    cfg = _gan_cfg("gan_loss", mode, real_label, fake_label)
    x, s = _gan_operand(logits, "gan_loss")
    return _GanLossFn.apply(x, s, bool(target_is_real), None, 1, False, cfg)[0]


def gan_loss_pair(fake_logits, real_logits, coef, mode="vanilla", real_label=1.0, fake_label=0.0):
    """-> (l_fake, l_real, total) 0-dim device tensors of one discriminator update: l_fake = GANLoss(mode)(fake_logits, False), l_real =
    GANLoss(mode)(real_logits, True), total = coef * (l_fake + l_real), formed on the device (cal_lossD: coef = 0.5 * lam_gan).  The two
    tensors may differ in size; each is read in place under the rule of `gan_loss`."""
    _lib.require_cuda(fake_logits, real_logits)
    cfg = _gan_cfg("gan_loss_pair", mode, real_label, fake_label, coef)
    xa, sa = _gan_operand(fake_logits, "gan_loss_pair")
    xb, sb = _gan_operand(real_logits, "gan_loss_pair")
    return _GanLossFn.apply(xa, sa, False, xb, sb, True, cfg)


class _NceFn(torch.autograd.Function):
    """BiPatchNCE(temperature)(F.normalize(g, dim=channel), F.normalize(p, dim=channel)) of train_NAR.py:81-84 / criterion.py:206-259
    on token-major projections g, p [frames * L, C] (g: ground-truth features, p: predicted features): 4 launches forward, 1 backward."""

    @staticmethod
    def forward(ctx, g, p, frames, L, temperature):
        _lib.require_cuda(g, p)
        g, p = _c(g), _c(p)
        R, C = g.shape
        if R != frames * L or p.shape != g.shape:
            raise RuntimeError("nce_loss: g %s / p %s do not hold %d frames of %d patches" % (tuple(g.shape), tuple(p.shape), frames, L))
        scratch = torch.empty(frames * L * (4 + L) + frames, device=g.device, dtype=torch.float32)
        loss = torch.empty((), device=g.device, dtype=torch.float32)
        check(lib.vptr_nce_fwd(ptr(g), ptr(p), ptr(scratch), ptr(loss), frames, L, C, temperature, stream()), "vptr_nce_fwd")
        ctx.save_for_backward(g, p, scratch)
        ctx.cfg = (frames, L, temperature)
        return loss

    @staticmethod
    def backward(ctx, gout):
        g, p, scratch = ctx.saved_tensors
        frames, L, temperature = ctx.cfg
        dg, dp = torch.empty_like(g), torch.empty_like(p)
        check(lib.vptr_nce_bwd(ptr(g), ptr(p), ptr(scratch), ptr(_c(gout)), ptr(dg), ptr(dp), frames, L, g.shape[1], temperature, stream()),
              "vptr_nce_bwd")
        return dg, dp, None, None, None


def nce_loss(g_tok, p_tok, frames, L, temperature=1.0):
    """bidirectional patch-wise contrastive loss of the un-normalised projector outputs (see _NceFn)"""
    return _NceFn.apply(g_tok, p_tok, int(frames), int(L), float(temperature))
