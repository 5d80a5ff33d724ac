"""Scoring of test-time rollouts on the device: the PSNR / SSIM / MSE curves over the predicted frame index that the reference's
notebook builds in its evaluation cell (`pred_ave_metrics`, utils/metrics.py:108-137) and reports in Table II.

The reference calls one metric function per (metric, time index) and reads every result back with `.item()`.  Here a batch is scored
by ONE `ops.frame_metrics` call (csrc/metrics.hip: every frame's PSNR, summed squared error and SSIM, renormalisation fused) and
one accumulate launch into a [T, 3] fp64 device buffer; nothing reaches the host before `compute()`.

All three metrics are batch means of per-image values, so the notebook loop's  sum_batches metric(batch) * N / sample_num  is the mean
of the per-image values over all samples: `acc / samples`.
"""
import numpy as np
import torch

from . import ops


class FrameMetrics:
    """Running per-time-index PSNR / SSIM / MSE of predicted frames.

    mean, std: the dataset's renormalisation (x * std + mean, VidReNormalize), a float or one value per channel; clamp: clamp the
    renormalised frames to [0, 1] first (the notebook's plotting path does, its metric loop does not)."""

    def __init__(self, num_frames, mean=0.0, std=1.0, clamp=False, data_range=1.0, device="cuda"):
        if int(num_frames) < 1:
            raise ValueError("FrameMetrics: num_frames must be >= 1")
        self.num_frames = int(num_frames)
        self.mean, self.std = mean, std
        self.clamp, self.data_range = bool(clamp), float(data_range)
        self.device = torch.device(device)
        self._mean_d = self._std_d = None          # per-channel device copies, made at the first update (C is known then)
        self.acc = torch.zeros((self.num_frames, 3), dtype=torch.float64, device=self.device)
        self.samples = 0

    def reset(self):
        self.acc.zero_()
        self.samples = 0

    def update(self, pred, gt):
        """pred, gt: (N, num_frames, C, H, W) device tensors in the model's normalised range; no host sync"""
        if pred.dim() != 5 or pred.shape[1] != self.num_frames:
            raise RuntimeError("FrameMetrics.update: expected (N, %d, C, H, W) frames, got %s" % (self.num_frames, tuple(pred.shape)))
        C = pred.shape[2]
        if self._mean_d is None or self._mean_d.numel() != C:
            self._mean_d = ops.metrics._per_channel(self.mean, C, pred.device, "mean")
            self._std_d = ops.metrics._per_channel(self.std, C, pred.device, "std")
        ops.frame_metrics(pred, gt, self._mean_d, self._std_d, self.clamp, self.data_range, acc=self.acc)
        self.samples += int(pred.shape[0])

    def compute(self):
        """-> {"psnr": np[T], "ssim": np[T], "mse": np[T], "samples": int}: per-time-index means over every sample seen (the one
        device-to-host transfer of an evaluation)"""
        if self.samples == 0:
            raise RuntimeError("FrameMetrics.compute: no samples were added")
        a = self.acc.cpu().numpy() / float(self.samples)
        return {"psnr": a[:, 0].copy(), "ssim": a[:, 2].copy(), "mse": a[:, 1].copy(), "samples": self.samples}


def evaluate_rollout(predict, loader, num_future_frames, mean=0.0, std=1.0, clamp=False, data_range=1.0, device="cuda"):
    """Metric curves of a predictor over a data loader.

    predict(past) -> predicted frames (N, >= num_future_frames, C, H, W), e.g.
        lambda p: far_rollout(enc, dec, T, p, n, mode="RIP", kv_cache=True),  NARTrainer.predict,  nar_bair_2_to_28;
    loader yields (past, future) pairs.  The first `num_future_frames` predicted frames are scored against the first
    `num_future_frames` frames of `future`.  Returns FrameMetrics.compute()."""
    fm = FrameMetrics(num_future_frames, mean, std, clamp, data_range, device)
    with torch.no_grad():
        for past, future in loader:
            past = past.to(fm.device, non_blocking=True)
            future = future.to(fm.device, non_blocking=True)
            pred = predict(past)
            if not isinstance(pred, torch.Tensor) or pred.dim() != 5 or pred.shape[1] < fm.num_frames or future.shape[1] < fm.num_frames:
                raise RuntimeError("evaluate_rollout: predict(past) and future must hold at least %d frames (N, T, C, H, W)" % fm.num_frames)
            fm.update(pred[:, :fm.num_frames], future[:, :fm.num_frames])
    return fm.compute()
