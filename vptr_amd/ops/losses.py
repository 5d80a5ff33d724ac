"""Fused loss kernels: MSE + GDL, the reconstruction losses with temporal weights / L1 / a GDL exponent, BiPatchNCE."""

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
