"""Sample panels: predicted clips back to images, on the device.

The reference's scripts call `visualize_batch_clips` (utils/train_summary.py:162-198) every epoch: it pads past / future / predicted clips
to one length, concatenates them along W in fp32, copies that tensor to the host and then, per frame in Python, runs VidReNormalize's two
Normalize calls, a clamp and ToPILImage before it writes GIFs.  Here ONE `ops.clip_panels` call (csrc/panels.hip) does everything up to
the uint8 image on the device, with the reference's own fp32 operations (the bytes are equal), and one byte per value is copied to the
host instead of four.  The same call with quantize="nearest" exports rollouts as uint8 [N, T, H, W, C] videos, the input of the standard
LPIPS / FVD tools (which stay out of scope).
"""
from pathlib import Path

import torch

from . import ops


class ReNorm:
    """The constants of the reference's VidReNormalize(mean, std): z = (x / a) - b with a = 1.0 / std (computed in double, rounded to fp32
    when Normalize makes a tensor of it) and b = -mean.  mean, std: a float or one value per channel; or pass any object that has
    `inv_std` / `inv_mean` attributes (a VidReNormalize instance) as the only argument."""

    def __init__(self, mean, std=None):
        if std is None:
            if not (hasattr(mean, "inv_std") and hasattr(mean, "inv_mean")):
                raise ValueError("ReNorm: give (mean, std), or an object with inv_std / inv_mean attributes")
            self.inv_std, self.inv_mean = mean.inv_std, mean.inv_mean
        else:
            try:
                inv_std, inv_mean = [1.0 / float(s) for s in std], [-float(m) for m in mean]
            except TypeError:
                inv_std, inv_mean = 1.0 / float(std), -float(mean)
            self.inv_std, self.inv_mean = inv_std, inv_mean
        self._dev = {}

    @classmethod
    def of(cls, renorm):
        """None, a ReNorm, or an object with inv_std / inv_mean -> None or a ReNorm"""
        return renorm if renorm is None or isinstance(renorm, cls) else cls(renorm)

    def constants(self, channels):
        """(a, b): fp32 CPU tensors [channels]"""
        def per_channel(v, what):
            vals = [float(v)] * channels if isinstance(v, (int, float)) else [float(e) for e in v]
            if len(vals) != channels:
                raise ValueError("ReNorm: %s has %d entries for %d channels" % (what, len(vals), channels))
            return torch.tensor(vals, dtype=torch.float64).to(torch.float32)
        a, b = per_channel(self.inv_std, "inv_std"), per_channel(self.inv_mean, "inv_mean")
        if bool((a == 0).any()):
            raise ValueError("ReNorm: 1 / std must not be zero")
        return a, b

    def tensors(self, channels, device):
        """(a, b) on `device`, made once per (channels, device)"""
        key = (int(channels), str(device))
        if key not in self._dev:
            a, b = self.constants(channels)
            self._dev[key] = (a.to(device), b.to(device))
        return self._dev[key]


def clips_to_uint8(clips, renorm=None, clamp=None, quantize="floor", layout="frames", pad="reference", gray_to_rgb=False, out=None,
                   to_host=False):
    """clips: 1 .. 4 fp32 device tensors [N, T_k, C, H, W] (views are read in place) -> the uint8 channel-last panel of `ops.clip_panels`
    ("frames": [N, max T_k, H, K * W, Cout]; "sheet": [N, K * H, max T_k * W, Cout]), a device tensor, or with to_host=True a numpy array
    that arrives through one pinned, non-blocking copy.  renorm: None, a ReNorm, or the reference's VidReNormalize instance; clamp
    defaults to `renorm is not None`, as in visualize_batch_clips.  pad="reference" repeats frame T_k - 2 of a shorter clip (append_frames'
    batch[:, -2:-1]; with 2 frames that is frame 0), "last" its last frame, "blank" writes bytes of 0."""
    clips = list(clips) if isinstance(clips, (tuple, list)) else [clips]
    renorm = ReNorm.of(renorm)
    a = b = None
    if renorm is not None and clips and isinstance(clips[0], torch.Tensor) and clips[0].dim() == 5:
        a, b = renorm.tensors(int(clips[0].shape[2]), clips[0].device)
    if clamp is None:
        clamp = renorm is not None
    dev = ops.clip_panels(clips, a, b, clamp=clamp, quantize=quantize, layout=layout, pad=pad, gray_to_rgb=gray_to_rgb, out=out)
    if not to_host:
        return dev
    host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream(dev.device).synchronize()
    return host.numpy()


def save_gifs(panels, file_dir, desc=None):
    """panels: uint8 numpy [N, L, H, W, C], C in {1, 3} -> `{desc}_clip_{n}.gif` per sample, written as the reference's save_clip does
    (PIL images of mode L or RGB, save_all with the other frames appended).  Returns the paths."""
    from PIL import Image
    file_dir = Path(file_dir)
    file_dir.mkdir(parents=True, exist_ok=True)
    if panels.ndim != 5 or panels.shape[-1] not in (1, 3) or str(panels.dtype) != "uint8":
        raise ValueError("save_gifs: expected uint8 [N, L, H, W, C] with C in {1, 3}, got %s %s" % (panels.dtype, panels.shape))
    paths = []
    for n in range(panels.shape[0]):
        if panels.shape[-1] == 1:
            imgs = [Image.fromarray(panels[n, t, :, :, 0], "L") for t in range(panels.shape[1])]
        else:
            imgs = [Image.fromarray(panels[n, t], "RGB") for t in range(panels.shape[1])]
        path = file_dir.joinpath("%s_clip_%d.gif" % (desc, n))
        imgs[0].save(str(path.absolute()), save_all=True, append_images=imgs[1:])
        paths.append(path)
    return paths


def visualize_batch_clips(gt_past_frames_batch, gt_future_frames_batch, pred_frames_batch, file_dir, renorm_transform=None, desc=None):
    """The reference's function (same signature, same file names `{desc}_clip_{n}.gif`, same bytes): past | future | predicted side by
    side, shorter clips padded with their frame T - 2.  One kernel call and one uint8 copy; returns the panels, uint8 numpy
    [N, L, H, 3 W, C].  (The reference pads to max(T_past, T_future) and needs the prediction to be as long as the future; here every clip
    is padded to the longest of the three.)"""
    panels = clips_to_uint8([gt_past_frames_batch, gt_future_frames_batch, pred_frames_batch], renorm=renorm_transform, pad="reference",
                            to_host=True)
    save_gifs(panels, file_dir, desc)
    return panels


def _zero_pad(clip, length):
    """the scripts' torch.cat with zeros in the model's range (they renormalise to the dataset mean, not to black)"""
    N, T, C, H, W = clip.shape
    return clip if T >= length else torch.cat([clip, torch.zeros((N, length - T, C, H, W), device=clip.device, dtype=clip.dtype)], dim=1)


def _sample(sample, device):
    past, future = sample
    if device is not None:
        past, future = past.to(device), future.to(device)
    return past, future


@torch.no_grad()
def ae_show_samples(enc, dec, sample, save_dir, renorm_transform=None, device=None):
    """train_AutoEncoder.py's show_samples: past | reconstructed future | reconstructed past of the first min(N, 4) samples as
    `ae_clip_{n}.gif`.  sample: (past, future); returns {"ae": panels}."""
    enc.eval(), dec.eval()
    past, future = _sample(sample, device)
    rec_past, rec_future = dec(enc(past)), dec(enc(future))
    idx = min(int(future.shape[0]), 4)
    return {"ae": visualize_batch_clips(past[0:idx], rec_future[0:idx], rec_past[0:idx], save_dir, renorm_transform, desc="ae")}


@torch.no_grad()
def nar_show_samples(enc, dec, T, sample, save_dir, renorm_transform=None, device=None):
    """train_NAR.py's NAR_show_samples: `pred_clip_{n}.gif` (past | future | predicted future) and `ae_clip_{n}.gif` (past | reconstructed
    future | reconstructed past) of the first min(N, 4) samples.  With fewer past than future frames the past and its reconstruction are
    zero-padded in the model's range, as the script does.  Returns {"pred": panels, "ae": panels}."""
    T.eval()
    past, future = _sample(sample, device)
    past_feats, future_feats = enc(past), enc(future)
    rec_past, rec_future = dec(past_feats), dec(future_feats)
    pred_future = dec(T(past_feats))
    idx = min(int(pred_future.shape[0]), 4)
    TF = int(future.shape[1])
    past, rec_past = _zero_pad(past, TF), _zero_pad(rec_past, TF)
    return {"pred": visualize_batch_clips(past[0:idx], future[0:idx], pred_future[0:idx], save_dir, renorm_transform, desc="pred"),
            "ae": visualize_batch_clips(past[0:idx], rec_future[0:idx], rec_past[0:idx], save_dir, renorm_transform, desc="ae")}


@torch.no_grad()
def far_show_samples(enc, dec, T, num_pred, sample, save_dir, renorm_transform=None, device=None, test_phase=True, kv_cache=False):
    """train_FAR.py's FAR_show_sample: `pred_future_clip_{n}.gif` (past | future | predicted future) and `pred_past_clip_{n}.gif`
    (past[1:] | re-predicted past | predicted future[:-1]) of the first min(N, 4) samples; the sliced clips are read as views.
    test_phase=True is `far_rollout(mode="train")`, which is the script's loop line by line (train_FAR.py:113-123: growing window,
    Dec -> Enc from the second prediction on, one decoder pass at the end); far_rollout's "RIP" mode is NOT that loop -- it is the
    notebook's FAR_RIP_test_single_iter, which decodes every step and slides the window.  test_phase=False feeds the true future
    features (teacher forcing, one pass).  As train_FAR_mp.py does, the past and the re-predicted past are zero-padded in the model's
    range when there are fewer past than future frames.  Returns {"pred_future": panels, "pred_past": panels}."""
    from .inference import far_rollout
    T.eval()
    past, future = _sample(sample, device)
    if test_phase:
        pred_past, pred_future = far_rollout(enc, dec, T, past, num_pred, mode="train", kv_cache=kv_cache)
    else:
        frames = dec(T(torch.cat([enc(past), enc(future)[:, 0:-1]], dim=1)))
        pred_past, pred_future = frames[:, 0:-num_pred], frames[:, -num_pred:]
    idx = min(int(pred_future.shape[0]), 4)
    TP, TF = int(past.shape[1]), int(future.shape[1])
    if TP < TF:
        past, pred_past = _zero_pad(past, TF), _zero_pad(pred_past, pred_past.shape[1] + TF - TP)
    return {"pred_future": visualize_batch_clips(past[0:idx], future[0:idx], pred_future[0:idx], save_dir, renorm_transform, desc="pred_future"),
            "pred_past": visualize_batch_clips(past[0:idx, 1:], pred_past[0:idx], pred_future[0:idx, :-1], save_dir, renorm_transform,
                                               desc="pred_past")}


def export_rollout(predict, loader, num_future_frames, renorm=None, quantize="nearest", gray_to_rgb=False, device="cuda"):
    """The hand-over to external LPIPS / FVD tools: yields (pred_u8, gt_u8) numpy arrays [N, num_future_frames, H, W, C] per batch.
    predict and loader are those of `evaluate_rollout`: predict(past) -> (N, >= num_future_frames, C, H, W), loader yields (past, future).
    quantize="nearest" returns the original bytes of ground truth that came from uint8 frames; gray_to_rgb gives grey clips the three
    channels LPIPS wants."""
    device = torch.device(device)
    T = int(num_future_frames)
    with torch.no_grad():
        for past, future in loader:
            past, future = past.to(device, non_blocking=True), future.to(device, non_blocking=True)
            pred = predict(past)
            if not isinstance(pred, torch.Tensor) or pred.dim() != 5 or pred.shape[1] < T or future.shape[1] < T:
                raise RuntimeError("export_rollout: predict(past) and future must hold at least %d frames (N, T, C, H, W)" % T)
            yield tuple(clips_to_uint8([x[:, :T]], renorm=renorm, quantize=quantize, gray_to_rgb=gray_to_rgb, to_host=True) for x in (pred, future))
