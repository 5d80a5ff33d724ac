"""Clip ingest: from decoded uint8 frames to the normalised fp32 (past, future) device tensors of the trainers and the evaluation.

The reference prepares every clip on the host, frame by frame, with PIL and torchvision (utils/dataset.py: VidCenterCrop, VidResize,
VidRandomHorizontalFlip / VerticalFlip, VidToTensor, VidNormalize).  Here a batch of decoded frames is uploaded as uint8 and ONE
`ops.ingest_clips` call (csrc/ingest.hip) does all of it on the device, bit for bit:

  * PIL's 8-bit bilinear resize is integer arithmetic on coefficient tables; `resize_tables` builds those tables exactly as Pillow's
    `precompute_coeffs` / `normalize_coeffs_8bpc` do (tests/test_ingest_cpu.py pins them against PIL itself);
  * ToTensor + Normalize of a uint8 value is a 256-entry table per channel, built with the same fp32 operations (`normalize_lut`).

File discovery and image decoding stay with the caller: the feature starts at uint8 arrays [N, T, H, W, C].
"""
import math

import numpy as np
import torch

PRECISION_BITS = 22      # Pillow: 32 - 8 - 2

KTH_MEAN, KTH_STD = 0.6013795, 2.7570653                                                # utils/dataset.py:23
BAIR_MEAN, BAIR_STD = (0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673)   # utils/dataset.py:49


def center_crop_box(h, w, th, tw):
    """(top, left, th, tw) of torchvision's CenterCrop((th, tw)) on an h x w image.  A crop larger than the image is rejected (torchvision
    would pad)."""
    h, w, th, tw = int(h), int(w), int(th), int(tw)
    if th < 1 or tw < 1 or th > h or tw > w:
        raise ValueError("center_crop_box: crop %d x %d does not fit in the %d x %d image (padding crops are not supported)" % (th, tw, h, w))
    return int(round((h - th) / 2.0)), int(round((w - tw) / 2.0)), th, tw


def resize_tables(in_size, out_size):
    """Pillow's bilinear coefficient tables for resizing one axis from in_size to out_size pixels of an 8-bit image:
    (k int32 [out_size, ksize], bounds int32 [out_size, 2] = (first input pixel, count)).  Float64 arithmetic in Pillow's order."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_tables: sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs                                   # the triangle filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)       # int() truncates, as the C cast does
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((j + xmin - center + 0.5) * ss)) for j in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for j in range(n):
            wj = w[j] / ww if ww != 0.0 else w[j]
            k[xx, j] = int(0.5 + wj * (1 << PRECISION_BITS))   # weights of this filter are never negative
        bounds[xx] = (xmin, n)
    return k, bounds


def normalize_lut(mean, std, channels):
    """fp32 [channels, 256]: ToTensor (uint8 / 255) followed by Normalize ((x - mean) / std) for every uint8 value, with the fp32
    operations the two transforms run.  mean, std: a float or one value per channel."""
    def per_channel(v, what):
        vals = [float(v)] * channels if isinstance(v, (int, float)) else [float(e) for e in v]
        if len(vals) != channels:
            raise ValueError("normalize_lut: %s has %d entries for %d channels" % (what, len(vals), channels))
        return vals
    m, s = per_channel(mean, "mean"), per_channel(std, "std")
    if any(e == 0.0 for e in s):
        raise ValueError("normalize_lut: std must not be zero")
    return torch.stack([torch.arange(256, dtype=torch.float32).div(255).sub(m[c]).div(s[c]) for c in range(channels)])


class IngestPlan:
    """Everything `ops.ingest_clips` needs for one dataset geometry, built once and kept on `device`.

    in_hw: (H, W) of the decoded frames; channels: 1 or 3; out_hw: (H, W) of the model input; crop: None (whole image), (th, tw) for a
    centre crop, or an explicit (top, left, th, tw); mean, std: the Normalize constants (0 and 1: ToTensor only)."""

    def __init__(self, in_hw, channels, out_hw, crop=None, mean=0.0, std=1.0, device="cuda"):
        self.in_hw = (int(in_hw[0]), int(in_hw[1]))
        self.channels = int(channels)
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        if self.channels not in (1, 3):
            raise ValueError("IngestPlan: channels must be 1 or 3, got %d" % self.channels)
        if min(self.in_hw) < 1 or min(self.out_hw) < 1:
            raise ValueError("IngestPlan: sizes must be >= 1")
        H, W = self.in_hw
        if crop is None:
            self.crop = (0, 0, H, W)
        elif len(crop) == 2:
            self.crop = center_crop_box(H, W, crop[0], crop[1])
        else:
            self.crop = tuple(int(e) for e in crop)
            top, left, th, tw = self.crop
            if min(top, left) < 0 or min(th, tw) < 1 or top + th > H or left + tw > W:
                raise ValueError("IngestPlan: crop box %s is empty or not inside the %d x %d image" % (self.crop, H, W))
        self.mean, self.std = mean, std
        self.device = torch.device(device)
        _, _, Hc, Wc = self.crop
        self.kx = self.bx = self.ky = self.by = None       # a pass whose size does not change is not run (PIL runs none either)
        self.ksx = self.ksy = 0
        if self.out_hw[1] != Wc:
            k, b = resize_tables(Wc, self.out_hw[1])
            self.ksx = int(k.shape[1])
            self.kx, self.bx = torch.from_numpy(k).to(self.device), torch.from_numpy(b).to(self.device)
        if self.out_hw[0] != Hc:
            k, b = resize_tables(Hc, self.out_hw[0])
            self.ksy = int(k.shape[1])
            self.ky, self.by = torch.from_numpy(k).to(self.device), torch.from_numpy(b).to(self.device)
        self.lut = normalize_lut(mean, std, self.channels).to(self.device)

    # the reference's constants (get_dataloader, utils/dataset.py:21-64)
    @classmethod
    def kth(cls, size=64, device="cuda"):
        """KTH: 120 x 160 grey frames, VidCenterCrop((120, 120)), VidResize((size, size)), VidNormalize"""
        return cls((120, 160), 1, (size, size), crop=(120, 120), mean=KTH_MEAN, std=KTH_STD, device=device)

    @classmethod
    def bair(cls, device="cuda"):
        """BAIR: 64 x 64 RGB frames, VidToTensor + VidNormalize"""
        return cls((64, 64), 3, (64, 64), mean=BAIR_MEAN, std=BAIR_STD, device=device)

    @classmethod
    def mnist(cls, device="cuda"):
        """MovingMNIST: 64 x 64 grey frames, VidToTensor only"""
        return cls((64, 64), 1, (64, 64), device=device)


class ClipIngest:
    """The reference's train / test transform of a dataset as a callable on uint8 batches.

    __call__(raw) takes [N, num_past + num_future, H, W, C] uint8 frames (host tensor, numpy array or device tensor) and returns the
    (past, future) fp32 device tensors.  hflip_p / vflip_p: per-clip flip probabilities (VidRandomHorizontalFlip / VerticalFlip; 0.5 in
    the KTH and MovingMNIST train transforms, 0 at test time); the flags come from this object's own seeded RandomState."""

    def __init__(self, plan, num_past, num_future, hflip_p=0.0, vflip_p=0.0, seed=None):
        if int(num_past) < 0 or int(num_future) < 0 or int(num_past) + int(num_future) < 1:
            raise ValueError("ClipIngest: num_past and num_future must be >= 0 and not both 0")
        if not (0.0 <= hflip_p <= 1.0 and 0.0 <= vflip_p <= 1.0):
            raise ValueError("ClipIngest: invalid flip probability")
        self.plan = plan
        self.num_past, self.num_future = int(num_past), int(num_future)
        self.hflip_p, self.vflip_p = float(hflip_p), float(vflip_p)
        self.rng = np.random.RandomState(seed)
        self.last_flips = None

    def draw_flips(self, n):
        """int32 [n]: bit 0 = horizontal, bit 1 = vertical flip of clip i; None when both probabilities are 0"""
        if self.hflip_p == 0.0 and self.vflip_p == 0.0:
            return None
        u = self.rng.rand(n, 2)
        return ((u[:, 0] < self.hflip_p).astype(np.int32) | ((u[:, 1] < self.vflip_p).astype(np.int32) << 1)).astype(np.int32)

    def __call__(self, raw, flips=None, out=None):
        from . import ops
        dev = self.plan.device
        if isinstance(raw, np.ndarray):
            raw = torch.from_numpy(np.ascontiguousarray(raw))
        if not raw.is_cuda:
            raw = raw.contiguous()
            if dev.type == "cuda":
                if not raw.is_pinned():
                    raw = raw.pin_memory()
                raw = raw.to(dev, non_blocking=True)
        T = self.num_past + self.num_future
        if raw.dim() != 5 or raw.shape[1] != T:
            raise RuntimeError("ClipIngest: expected (N, %d, H, W, C) frames, got %s" % (T, tuple(raw.shape)))
        if flips is None:
            flips = self.draw_flips(int(raw.shape[0]))
        if flips is not None and not isinstance(flips, torch.Tensor):
            flips = torch.from_numpy(np.ascontiguousarray(np.asarray(flips, dtype=np.int32)))
        self.last_flips = np.zeros(int(raw.shape[0]), dtype=np.int32) if flips is None else flips.detach().cpu().numpy().astype(np.int32)
        if flips is not None:
            flips = flips.to(device=dev, dtype=torch.int32).contiguous()
        return ops.ingest_clips(raw, self.plan, flips=flips, split=(self.num_past, self.num_future), out=out)


class DeviceClipLoader:
    """Wraps a loader of uint8 clip batches [N, Tp + Tf, H, W, C]: iterating yields the (past, future) device tensors, which is what
    `evaluate_rollout` and a training loop take."""

    def __init__(self, loader, ingest):
        self.loader, self.ingest = loader, ingest

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for raw in self.loader:
            yield self.ingest(raw)
