"""Clip ingest: from decoded uint8 frames to the normalised fp32 (past, future) device tensors of the trainers and the evaluation.

The reference prepares every clip on the host, frame by frame, with PIL and torchvision (utils/dataset.py: VidCenterCrop, VidResize,
VidRandomHorizontalFlip / VerticalFlip, VidToTensor, VidNormalize).  Here a batch of decoded frames is uploaded as uint8 and ONE
`ops.ingest_clips` call (csrc/ingest.hip) does all of it on the device, bit for bit:

  * PIL's 8-bit bilinear resize is integer arithmetic on coefficient tables; `resize_tables` builds those tables exactly as Pillow's
    `precompute_coeffs` / `normalize_coeffs_8bpc` do (tests/test_ingest_cpu.py pins them against PIL itself);
  * ToTensor + Normalize of a uint8 value is a 256-entry table per channel, built with the same fp32 operations (`normalize_lut`).

File discovery and image decoding stay with the caller: the feature starts at uint8 arrays [N, T, H, W, C].

`DeviceClipStore` + `StoreLoader` keep a whole training set on the device as uint8 frames instead: a batch is then drawn
(`ops.clip_draw`) and gathered + ingested (`ops.ingest_gather`, the same kernel body) there, two launches and no host work per step.
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


# ---- the HBM-resident clip store (csrc/clipstore.hip, include/vptr_hip_data.h) -----------------------------------------------------
# cursor words, as the header names them
CUR_SEED_LO, CUR_SEED_HI, CUR_EPOCH, CUR_BATCH, CUR_BPE, CUR_DRAWN_LO, CUR_DRAWN_HI, CUR_WORDS = 0, 1, 2, 3, 4, 5, 6, 16
SEL_PAST, SEL_FUTURE, SEL_FLIPS, SEL_CLIP, SEL_WORDS = 0, 1, 2, 3, 4
UPLOAD_CHUNK_BYTES = 64 << 20     # the pinned staging buffer of DeviceClipStore's upload


def _s32(v):
    """the int32 that holds the low 32 bits of v"""
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def _as_frames(a, what):
    """one uint8 [F, H, W, C] host tensor (or device tensor, left where it is) from an array or tensor"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor) or a.dtype != torch.uint8 or a.dim() != 4:
        raise ValueError("DeviceClipStore: %s must be uint8 [F, H, W, C], got %s %s"
                         % (what, getattr(a, "dtype", type(a)), tuple(getattr(a, "shape", ()))))
    return a


class DeviceClipStore:
    """A training set resident on the device: `frames`, uint8 [F, H, W, C], uploaded once, and `clip_table`, int32 [n_clips, 2] = (first
    past frame, first future frame) of every clip.  A batch is then a table of frame indices (`StoreLoader`); nothing crosses the bus
    per step.

    frames: a uint8 [F, H, W, C] array or tensor, or a list of per-video arrays [F_v, H, W, C] stored one after the other; clips:
    integer [n_clips, 2] frame indices into the concatenated store.  The upload goes through one pinned staging buffer of at most
    `UPLOAD_CHUNK_BYTES`.  device "cpu" keeps everything on the host: the clip rules can then be checked without a GPU (no kernel runs
    there).  num_past / num_future: the clip lengths the table was built for, when the builder knows them."""

    def __init__(self, frames, clips, device="cuda", num_past=None, num_future=None):
        pieces = [_as_frames(v, "a video") for v in frames] if isinstance(frames, (list, tuple)) else [_as_frames(frames, "frames")]
        if not pieces:
            raise ValueError("DeviceClipStore: no frames")
        shape = tuple(pieces[0].shape[1:])
        if any(tuple(p.shape[1:]) != shape for p in pieces):
            raise ValueError("DeviceClipStore: the videos differ in frame shape")
        F = sum(int(p.shape[0]) for p in pieces)
        if F < 1 or F > 0x7FFFFFFF or min(shape) < 1:
            raise ValueError("DeviceClipStore: %d frames of shape %s (1 .. 2^31 - 1 non-empty frames are supported)" % (F, shape))
        clips = np.asarray(clips.cpu() if isinstance(clips, torch.Tensor) else clips)
        if clips.ndim != 2 or clips.shape[1] != 2 or clips.shape[0] < 1 or clips.dtype.kind not in "iu":
            raise ValueError("DeviceClipStore: clips must be integers [n_clips, 2] with n_clips >= 1, got %s %s" % (clips.dtype, clips.shape))
        if clips.min() < 0 or clips.max() >= F:
            raise ValueError("DeviceClipStore: a clip starts outside the store's %d frames" % F)
        self.device = torch.device(device)
        self.n_frames, self.frame_shape = F, shape
        self.num_past, self.num_future = num_past, num_future
        self.clips_host = np.ascontiguousarray(clips.astype(np.int32))
        self.clip_table = torch.from_numpy(self.clips_host).to(self.device)
        self.frames = torch.empty((F,) + shape, dtype=torch.uint8, device=self.device)
        self._upload(pieces)

    def _upload(self, pieces):
        if self.device.type != "cuda":
            torch.cat(pieces, out=self.frames)
            return
        per = int(np.prod(self.frame_shape))
        chunk = max(1, UPLOAD_CHUNK_BYTES // per)
        stage, at = None, 0
        for p in pieces:
            for lo in range(0, int(p.shape[0]), chunk):
                part = p[lo:lo + chunk]
                n = int(part.shape[0])
                if part.is_cuda:
                    self.frames[at:at + n].copy_(part)
                else:
                    if stage is None:
                        stage = torch.empty((min(chunk, self.n_frames),) + self.frame_shape, dtype=torch.uint8).pin_memory()
                    stage[:n].copy_(part)
                    self.frames[at:at + n].copy_(stage[:n], non_blocking=True)
                    torch.cuda.current_stream(self.device).synchronize()      # the staging buffer is free again
                at += n

    @property
    def n_clips(self):
        return int(self.clips_host.shape[0])

    def nbytes(self):
        return self.frames.numel()

    @classmethod
    def from_videos(cls, videos, num_past, num_future, device="cuda"):
        """The reference's `__getClips__` (KTH, BAIR: utils/dataset.py): per video, non-overlapping clips of num_past + num_future frames;
        the remainder `rem` is dropped, `rem // 2` frames of it in front.  Only the kept span of a video is stored.  videos: a list of
        uint8 [F_v, H, W, C] arrays, in the order the reference lists their folders."""
        L = int(num_past) + int(num_future)
        if int(num_past) < 0 or int(num_future) < 0 or L < 1:
            raise ValueError("from_videos: num_past and num_future must be >= 0 and not both 0")
        kept, clips, at = [], [], 0
        for v in videos:
            v = _as_frames(v, "a video")
            n = int(v.shape[0])
            clip_num, rem = n // L, n % L
            if clip_num == 0:
                continue
            kept.append(v[rem // 2:rem // 2 + clip_num * L])
            clips.extend((at + i * L, at + i * L + int(num_past)) for i in range(clip_num))
            at += clip_num * L
        if not clips:
            raise ValueError("from_videos: no video holds a clip of %d frames" % L)
        return cls(kept, np.asarray(clips, dtype=np.int64), device=device, num_past=int(num_past), num_future=int(num_future))

    @classmethod
    def from_moving_mnist(cls, data, num_past=None, num_future=None, device="cuda"):
        """The reference's `MovingMNISTDataset.__getitem__`: data["clips"] is [2, n_clips, 2] = (start, length) of the past ([0]) and the
        future ([1]) part of every clip, two independent starts into data["input_raw_data"], uint8 [F, 1, H, W] (or [F, H, W]).
        num_past / num_future default to the lengths of the first clip; every clip must have them."""
        clips, raw = np.asarray(data["clips"]), np.asarray(data["input_raw_data"])
        if clips.ndim != 3 or clips.shape[0] != 2 or clips.shape[2] != 2 or clips.shape[1] < 1:
            raise ValueError("from_moving_mnist: clips must be [2, n_clips, 2], got %s" % (clips.shape,))
        if raw.ndim == 4 and raw.shape[1] == 1:
            raw = raw[:, 0]
        if raw.ndim != 3:
            raise ValueError("from_moving_mnist: input_raw_data must be [F, 1, H, W] or [F, H, W], got %s" % (raw.shape,))
        if raw.dtype != np.uint8:
            raise ValueError("from_moving_mnist: input_raw_data must be uint8, got %s" % raw.dtype)
        Tp = int(clips[0, 0, 1]) if num_past is None else int(num_past)
        Tf = int(clips[1, 0, 1]) if num_future is None else int(num_future)
        if not (np.all(clips[0, :, 1] == Tp) and np.all(clips[1, :, 1] == Tf)):
            raise ValueError("from_moving_mnist: a clip's lengths differ from num_past %d / num_future %d" % (Tp, Tf))
        starts = np.stack([clips[0, :, 0], clips[1, :, 0]], axis=1).astype(np.int64)
        F = int(raw.shape[0])
        if starts.min() < 0 or (starts[:, 0] + Tp).max() > F or (starts[:, 1] + Tf).max() > F:
            raise ValueError("from_moving_mnist: a clip's frames leave the %d frames of input_raw_data" % F)
        return cls(raw[..., None], starts, device=device, num_past=Tp, num_future=Tf)


class StoreLoader:
    """One epoch of (past, future) device tensors per iteration, drawn and gathered on the device: per batch `ops.clip_draw` (which clips,
    which flips, from the device cursor) and `ops.ingest_gather` (their frames out of the store through `plan`), and nothing else -- no
    host batch, no copy, no sync.  It stands where `DataLoader(shuffle=True, drop_last=True)` / `DistributedSampler` + the host
    transforms stand in the reference: the epoch's order is a permutation of the clip list keyed on (seed, epoch), rank r of `world`
    takes positions (batch * world + r) * N .. + N - 1 of it.

    out: a (past, future) pair to write every batch into, e.g. `trainer.static_inputs()`: `step` then skips its copy.
    drop_last=False (sequential evaluation: shuffle=False, no flips, world 1) adds the tail of n_clips % N clips as a last, smaller batch
    through a host-written table.

    The host mirrors the cursor's (epoch, batch) through its own launches, `seek` and `load_state_dict`; iterating yields the rest of the
    current epoch.  `state_dict()` reads the device cursor (one sync)."""

    def __init__(self, store, plan, N, num_past, num_future, shuffle=True, hflip_p=0.0, vflip_p=0.0, seed=0, rank=0, world=1, out=None,
                 drop_last=True):
        N, Tp, Tf, rank, world = int(N), int(num_past), int(num_future), int(rank), int(world)
        if N < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("StoreLoader: N %d and world %d must be >= 1 and rank %d in 0 .. world - 1" % (N, world, rank))
        if Tp < 0 or Tf < 0 or Tp + Tf < 1:
            raise ValueError("StoreLoader: num_past and num_future must be >= 0 and not both 0")
        if not (0.0 <= float(hflip_p) <= 1.0 and 0.0 <= float(vflip_p) <= 1.0):
            raise ValueError("StoreLoader: flip probabilities %r, %r must lie in [0, 1]" % (hflip_p, vflip_p))
        if store.n_clips < N * world:
            raise ValueError("StoreLoader: %d clips are fewer than N %d x world %d" % (store.n_clips, N, world))
        if tuple(plan.in_hw) != tuple(store.frame_shape[:2]) or plan.channels != store.frame_shape[2]:
            raise ValueError("StoreLoader: the plan expects %d x %d x %d frames, the store holds %s"
                             % (plan.in_hw[0], plan.in_hw[1], plan.channels, "%d x %d x %d" % tuple(store.frame_shape)))
        if (store.num_past is not None and store.num_past != Tp) or (store.num_future is not None and store.num_future != Tf):
            raise ValueError("StoreLoader: the store's clips were built for %s + %s frames, not %d + %d"
                             % (store.num_past, store.num_future, Tp, Tf))
        c = store.clips_host.astype(np.int64)
        if (c[:, 0] + Tp).max() > store.n_frames or (c[:, 1] + Tf).max() > store.n_frames:
            raise ValueError("StoreLoader: a clip's frames leave the store's %d frames" % store.n_frames)
        if not drop_last and (shuffle or float(hflip_p) != 0.0 or float(vflip_p) != 0.0 or world != 1):
            raise ValueError("StoreLoader: drop_last=False is the sequential pass: shuffle=False, no flips, world 1")
        if not 0 <= int(seed) < (1 << 64):
            raise ValueError("StoreLoader: seed must be a 64-bit unsigned value")
        self.store, self.plan, self.N, self.num_past, self.num_future = store, plan, N, Tp, Tf
        self.shuffle, self.hflip_p, self.vflip_p, self.seed = bool(shuffle), float(hflip_p), float(vflip_p), int(seed)
        self.rank, self.world, self.out = rank, world, (None if out is None else tuple(out))
        self.batches_per_epoch = store.n_clips // (N * world)
        dev = store.device
        self.cursor = torch.zeros(CUR_WORDS, dtype=torch.int32, device=dev)
        if self.cursor.data_ptr() % 64:
            raise RuntimeError("StoreLoader: the allocator returned a cursor record that is not 64-byte aligned")
        self.sel = torch.zeros((N, SEL_WORDS), dtype=torch.int32, device=dev)
        self._put(CUR_SEED_LO, self.seed)
        self._put(CUR_SEED_HI, self.seed >> 32)
        self._put(CUR_BPE, self.batches_per_epoch)
        self.epoch, self.batch = 0, 0
        self._tail_sel = None
        tail = store.n_clips - self.batches_per_epoch * N
        if not drop_last and tail > 0:
            ids = np.arange(store.n_clips - tail, store.n_clips)
            rows = np.stack([store.clips_host[ids, 0], store.clips_host[ids, 1], np.zeros(tail, dtype=np.int32), ids.astype(np.int32)], axis=1)
            self._tail_sel = torch.from_numpy(np.ascontiguousarray(rows.astype(np.int32))).to(dev)
        self._last_sel = self.sel

    def _put(self, idx, value):
        self.cursor[idx:idx + 1].fill_(_s32(value))      # a fill kernel: stream-ordered, no memset node

    def __len__(self):
        return self.batches_per_epoch + (1 if self._tail_sel is not None else 0)

    def draw(self):
        """the two launches of one batch -> (past, future); what a captured graph of the loader would hold"""
        from . import ops
        ops.clip_draw(self.cursor, self.store.clip_table, self.sel, rank=self.rank, world=self.world, shuffle=self.shuffle,
                      hflip_p=self.hflip_p, vflip_p=self.vflip_p)
        self._last_sel = self.sel
        self.batch += 1
        if self.batch >= self.batches_per_epoch:
            self.batch, self.epoch = 0, (self.epoch + 1) & 0xFFFFFFFF
        return ops.ingest_gather(self.store.frames, self.sel, self.plan, (self.num_past, self.num_future), out=self.out)

    def __iter__(self):
        from . import ops
        for _ in range(self.batches_per_epoch - self.batch):
            yield self.draw()
        if self._tail_sel is not None:
            self._last_sel = self._tail_sel
            yield ops.ingest_gather(self.store.frames, self._tail_sel, self.plan, (self.num_past, self.num_future))

    def last_selection(self):
        """int32 [N, 4] device view of the last batch's table: first past frame, first future frame, flip bits, clip id"""
        return self._last_sel

    def seek(self, epoch, batch=0):
        """the next draw is batch `batch` of epoch `epoch` (stream-ordered)"""
        epoch, batch = int(epoch), int(batch)
        if not (0 <= epoch < (1 << 32) and 0 <= batch < self.batches_per_epoch):
            raise ValueError("StoreLoader.seek: epoch %d, batch %d (of %d per epoch)" % (epoch, batch, self.batches_per_epoch))
        self._put(CUR_EPOCH, epoch)
        self._put(CUR_BATCH, batch)
        self.epoch, self.batch = epoch, batch

    def state_dict(self):
        w = [int(v) & 0xFFFFFFFF for v in self.cursor.cpu().tolist()]
        return {"seed": w[CUR_SEED_LO] | (w[CUR_SEED_HI] << 32), "epoch": w[CUR_EPOCH], "batch": w[CUR_BATCH] % self.batches_per_epoch,
                "drawn": w[CUR_DRAWN_LO] | (w[CUR_DRAWN_HI] << 32), "batches_per_epoch": self.batches_per_epoch}

    def load_state_dict(self, state):
        if int(state.get("batches_per_epoch", self.batches_per_epoch)) != self.batches_per_epoch:
            raise ValueError("StoreLoader.load_state_dict: the state was taken at %s batches per epoch, this loader has %d"
                             % (state.get("batches_per_epoch"), self.batches_per_epoch))
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        self._put(CUR_SEED_LO, self.seed)
        self._put(CUR_SEED_HI, self.seed >> 32)
        self._put(CUR_DRAWN_LO, int(state.get("drawn", 0)))
        self._put(CUR_DRAWN_HI, int(state.get("drawn", 0)) >> 32)
        self.seek(state["epoch"], state["batch"])
