"""Sample panels as one kernel call: fp32 clips in the model's range -> renormalised, quantised, tiled uint8 images (csrc/panels.hip)."""
import ctypes

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream

PANELS_MAX_CLIPS = 4     # PN_MAX_CLIPS
QUANTIZE = ("floor", "nearest")
LAYOUTS = ("frames", "sheet")
PADS = ("reference", "last", "blank")


def pad_indices(lengths, pad="reference"):
    """The frame of clip k that a cell t >= T_k of the panel shows, per clip (-1: bytes of 0), for panels of max(lengths) frames.
    "reference": frame T_k - 2, what visualize_batch_clips' append_frames repeats (batch[:, -2:-1]); a clip that has to be padded needs
    T_k >= 2 (with 2 frames it repeats frame 0).  "last": frame T_k - 1.  "blank": -1.  A clip of full length is never padded: -1."""
    if pad not in PADS:
        raise ValueError("clip_panels: pad must be one of %s, got %r" % (PADS, pad))
    lengths = [int(t) for t in lengths]
    if not lengths or min(lengths) < 1:
        raise RuntimeError("clip_panels: every clip needs T >= 1 frames, got %s" % (lengths,))
    L = max(lengths)
    out = []
    for k, t in enumerate(lengths):
        if t == L or pad == "blank":
            out.append(-1)
        elif pad == "last":
            out.append(t - 1)
        else:
            if t < 2:
                raise RuntimeError("clip_panels: pad='reference' repeats frame T - 2, but clip %d has T = %d < 2 frames (of %d)" % (k, t, L))
            out.append(t - 2)
    return out


def panel_shape(N, lengths, C, H, W, layout="frames", gray_to_rgb=False):
    """shape of the uint8 output: frames [N, L, H, K * W, Cout], sheet [N, K * H, L * W, Cout]; Cout = 3 if gray_to_rgb and C == 1 else C"""
    if layout not in LAYOUTS:
        raise ValueError("clip_panels: layout must be one of %s, got %r" % (LAYOUTS, layout))
    K, L = len(lengths), max(int(t) for t in lengths)
    Cout = 3 if gray_to_rgb and C == 1 else C
    return (N, L, H, K * W, Cout) if layout == "frames" else (N, K * H, L * W, Cout)


def _strides(x, k):
    """(sample stride, frame stride) in elements of a clip whose inner (C, H, W) block is contiguous; the stride of a dimension of size 1
    is never used and is passed as 0"""
    _, _, C, H, W = x.shape
    want = (H * W, W, 1)
    for d in (2, 3, 4):
        if x.shape[d] > 1 and x.stride(d) != want[d - 2]:
            raise RuntimeError("clip_panels: the (C, H, W) block of clip %d must be contiguous (shape %s, strides %s)"
                               % (k, tuple(x.shape), tuple(x.stride())))
    return (x.stride(0) if x.shape[0] > 1 else 0), (x.stride(1) if x.shape[1] > 1 else 0)


def clip_panels(clips, a=None, b=None, clamp=None, quantize="floor", layout="frames", pad="reference", gray_to_rgb=False, out=None):
    """clips: 1 .. 4 fp32 device tensors [N, T_k, C, H, W] (same N, C, H, W; C in {1, 3}; views with their own sample / frame strides are
    read in place) -> uint8 channel-last panels, `panel_shape`: "frames" [N, max T_k, H, K * W, Cout] (the clips side by side, the
    reference's torch.cat(dim=-1) as HWC) or "sheet" [N, K * H, max T_k * W, Cout] (one row of frames per clip).
    a, b: fp32 device tensors [C], both or neither: z = (x / a[c]) - b[c], VidReNormalize with a = 1 / std, b = -mean
    (`vptr_amd.visualize.ReNorm`).  clamp: clamp z to [0, 1] (default: when a is given, as visualize_batch_clips does).
    quantize: "floor" = ToPILImage's mul(255).byte(), "nearest" = trunc(z * 255 + 0.5) (returns every byte of frames that came from uint8
    data); saturating, NaN -> 0.  pad: what a cell past a clip's end shows (`pad_indices`).  gray_to_rgb: C == 1 -> three equal channels.
    out: a contiguous uint8 tensor of the panel shape to write into.  One launch, no host sync, no autograd."""
    clips = list(clips) if isinstance(clips, (tuple, list)) else [clips]
    if not 1 <= len(clips) <= PANELS_MAX_CLIPS:
        raise RuntimeError("clip_panels: between 1 and %d clips, got %d" % (PANELS_MAX_CLIPS, len(clips)))
    if quantize not in QUANTIZE:
        raise ValueError("clip_panels: quantize must be one of %s, got %r" % (QUANTIZE, quantize))
    if layout not in LAYOUTS:
        raise ValueError("clip_panels: layout must be one of %s, got %r" % (LAYOUTS, layout))
    if pad not in PADS:
        raise ValueError("clip_panels: pad must be one of %s, got %r" % (PADS, pad))
    _lib.require_cuda(*clips, a, b, out)
    x0 = clips[0]
    for k, x in enumerate(clips):
        if x.dtype != torch.float32 or x.dim() != 5:
            raise RuntimeError("clip_panels: clip %d must be a float32 (N, T, C, H, W) tensor, got %s %s" % (k, x.dtype, tuple(x.shape)))
        if min(x.shape) < 1:
            raise RuntimeError("clip_panels: clip %d has an empty dimension: %s" % (k, tuple(x.shape)))
        if x.shape[0] != x0.shape[0] or tuple(x.shape[2:]) != tuple(x0.shape[2:]) or x.device != x0.device:
            raise RuntimeError("clip_panels: clip %d %s does not match clip 0 %s in (N, C, H, W) or device" % (k, tuple(x.shape), tuple(x0.shape)))
    N, _, C, H, W = (int(s) for s in x0.shape)
    if C not in (1, 3):
        raise RuntimeError("clip_panels: C %d must be 1 or 3" % C)
    if (a is None) != (b is None):
        raise RuntimeError("clip_panels: a and b must be given together")
    for name, v in (("a", a), ("b", b)):
        if v is not None and (v.dtype != torch.float32 or tuple(v.shape) != (C,) or not v.is_contiguous() or v.device != x0.device):
            raise RuntimeError("clip_panels: %s must be a contiguous float32 [%d] tensor on the clips' device, got %s %s"
                               % (name, C, v.dtype, tuple(v.shape)))
    lengths = [int(x.shape[1]) for x in clips]
    pads = pad_indices(lengths, pad)
    strides = [_strides(x, k) for k, x in enumerate(clips)]
    shape = panel_shape(N, lengths, C, H, W, layout, gray_to_rgb)
    if out is None:
        out = torch.empty(shape, device=x0.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != x0.device:
        raise RuntimeError("clip_panels: out must be a contiguous uint8 %s tensor on the clips' device, got %s %s" % (list(shape), out.dtype, tuple(out.shape)))
    if clamp is None:
        clamp = a is not None
    K = len(clips)
    check(lib.vptr_clip_panels((ctypes.c_void_p * K)(*[x.data_ptr() for x in clips]), (ctypes.c_int32 * K)(*lengths),
                               (ctypes.c_int64 * K)(*[s[0] for s in strides]), (ctypes.c_int64 * K)(*[s[1] for s in strides]),
                               (ctypes.c_int32 * K)(*pads), ptr(a), ptr(b), ptr(out), K, N, C, H, W, int(bool(clamp)),
                               int(quantize == "nearest"), int(bool(gray_to_rgb)), LAYOUTS.index(layout), stream()), "vptr_clip_panels")
    return out
