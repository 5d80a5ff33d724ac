"""Evaluation metrics of a rollout as one kernel call: per-frame PSNR / summed squared error / SSIM (csrc/metrics.hip)."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream
from .core import _c

FRAME_METRICS_BAND = 16      # rows per workgroup of the tile kernel (FM_BAND): sizes the scratch buffer
FRAME_METRICS_MAX_W = 256


def _per_channel(v, C, device, what):
    """float, or a length-C sequence / tensor -> fp32 device tensor [C]"""
    if isinstance(v, (int, float)):
        return torch.full((C,), float(v), device=device, dtype=torch.float32)
    if isinstance(v, torch.Tensor):
        t = v.detach().to(device=device, dtype=torch.float32).reshape(-1)
    else:
        t = torch.tensor([float(e) for e in v], dtype=torch.float32).to(device)
    if t.numel() != C:
        raise RuntimeError("frame_metrics: %s has %d entries for %d channels" % (what, t.numel(), C))
    return t.contiguous()


def frame_metrics(pred, gt, mean=0.0, std=1.0, clamp=False, data_range=1.0, acc=None):
    """pred, gt: (N, T, C, H, W) or (N, C, H, W) (= T 1) fp32 frames in the model's normalised range -> [N, T, 3] fp32 device tensor
    of (PSNR in dB, summed squared error, SSIM) per frame, computed on x * std[c] + mean[c] (clamped to [0, 1] if `clamp`): the per-image
    values behind PSNR / MSEScore / SSIM(size_average=False) of vptr_amd.metrics.  Two launches, no host sync, no autograd.
    acc: optional [T, 3] fp64 device tensor; acc[t] += sum over n of the result[n, t] (one more launch)."""
    _lib.require_cuda(pred, gt, acc)
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("frame_metrics: pred (%s) and gt (%s) must be float32" % (pred.dtype, gt.dtype))
    if pred.shape != gt.shape or pred.dim() not in (4, 5):
        raise RuntimeError("frame_metrics: pred %s and gt %s must share a (N, T, C, H, W) or (N, C, H, W) shape" % (tuple(pred.shape), tuple(gt.shape)))
    if pred.dim() == 4:
        pred, gt = pred.unsqueeze(1), gt.unsqueeze(1)
    N, T, C, H, W = pred.shape
    if min(N, T, C, H) < 1 or not 1 <= W <= FRAME_METRICS_MAX_W:
        raise RuntimeError("frame_metrics: shape %s: every size must be >= 1 and W <= %d" % (tuple(pred.shape), FRAME_METRICS_MAX_W))
    if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (T, 3) or not acc.is_contiguous()):
        raise RuntimeError("frame_metrics: acc must be a contiguous float64 [%d, 3] tensor, got %s %s" % (T, acc.dtype, tuple(acc.shape)))
    mean_d = _per_channel(mean, C, pred.device, "mean")
    std_d = _per_channel(std, C, pred.device, "std")
    pred, gt = _c(pred.detach()), _c(gt.detach())
    frames = N * T
    scratch = torch.empty(frames * C * ((H + FRAME_METRICS_BAND - 1) // FRAME_METRICS_BAND) * 2, device=pred.device, dtype=torch.float32)
    out = torch.empty((N, T, 3), device=pred.device, dtype=torch.float32)
    check(lib.vptr_frame_metrics(ptr(pred), ptr(gt), ptr(mean_d), ptr(std_d), ptr(scratch), ptr(out), frames, C, H, W, int(bool(clamp)),
                                 float(data_range), stream()), "vptr_frame_metrics")
    if acc is not None:
        check(lib.vptr_frame_metrics_accumulate(ptr(out), ptr(acc), N, T, stream()), "vptr_frame_metrics_accumulate")
    return out
