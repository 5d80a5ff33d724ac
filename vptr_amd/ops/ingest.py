"""Clip ingest as one kernel call: uint8 frames -> cropped, resized, flipped, normalised fp32 model inputs (csrc/ingest.hip)."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream

INGEST_MAX_OUT = 256     # IG_MAX_OUT
INGEST_MAX_KSIZE = 17    # IG_MAX_KS: a downscale of at most 8x per axis


def _table(t, shape, what):
    if t is None:
        return
    if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise RuntimeError("ingest_clips: plan.%s must be a contiguous int32 %s tensor, got %s %s" % (what, list(shape), t.dtype, tuple(t.shape)))


def ingest_clips(raw, plan, flips=None, split=None, out=None):
    """raw: uint8 device tensor [N, T, Hin, Win, C] (channel-last, as decoded); plan: a `vptr_amd.data.IngestPlan` (crop box, PIL's
    resize tables, the ToTensor + Normalize table, all on the device) -> fp32 [N, T, C, Hout, Wout], bit-identical to the reference's
    host transforms.  flips: optional int32 device tensor [N], bit 0 = horizontal, bit 1 = vertical flip of the whole clip.
    split: Tp, or (Tp, Tf) with Tp + Tf == T: returns (frames[:, :Tp], frames[:, Tp:]) as two contiguous tensors.
    out: a tensor, or a pair of tensors, to write into (e.g. a trainer's static graph inputs); a pair implies the split.
    One launch, no host sync, no autograd."""
    outs = None
    if out is not None:
        outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        if len(outs) not in (1, 2):
            raise RuntimeError("ingest_clips: out must be one tensor or a pair of tensors")
    _lib.require_cuda(raw, flips, plan.lut, *(outs or ()))
    if raw.dtype != torch.uint8:
        raise RuntimeError("ingest_clips: raw (%s) must be uint8" % raw.dtype)
    Hin, Win = plan.in_hw
    C = plan.channels
    if raw.dim() != 5 or tuple(raw.shape[2:]) != (Hin, Win, C) or raw.shape[0] < 1 or raw.shape[1] < 1:
        raise RuntimeError("ingest_clips: raw %s must be (N, T, %d, %d, %d) with N, T >= 1 for this plan" % (tuple(raw.shape), Hin, Win, C))
    if not raw.is_contiguous():
        raise RuntimeError("ingest_clips: raw must be contiguous (N, T, H, W, C)")
    N, T = int(raw.shape[0]), int(raw.shape[1])
    top, left, Hc, Wc = plan.crop
    Hout, Wout = plan.out_hw
    if C not in (1, 3):
        raise RuntimeError("ingest_clips: C %d must be 1 or 3" % C)
    if not (1 <= Hout <= INGEST_MAX_OUT and 1 <= Wout <= INGEST_MAX_OUT):
        raise RuntimeError("ingest_clips: output size %d x %d is outside 1 .. %d per axis" % (Hout, Wout, INGEST_MAX_OUT))
    if min(top, left) < 0 or min(Hc, Wc) < 1 or top + Hc > Hin or left + Wc > Win:
        raise RuntimeError("ingest_clips: crop box %s is empty or not inside the %d x %d image" % ((top, left, Hc, Wc), Hin, Win))
    hpass, vpass = Wout != Wc, Hout != Hc
    if (hpass and not 1 <= plan.ksx <= INGEST_MAX_KSIZE) or (vpass and not 1 <= plan.ksy <= INGEST_MAX_KSIZE):
        raise RuntimeError("ingest_clips: ksize (%d, %d) is outside 1 .. %d: a downscale of at most 8x per axis is supported"
                           % (plan.ksx, plan.ksy, INGEST_MAX_KSIZE))
    if (hpass and (plan.kx is None or plan.bx is None)) or (vpass and (plan.ky is None or plan.by is None)):
        raise RuntimeError("ingest_clips: the plan has no tables for a pass it needs")
    _lib.require_cuda(plan.kx, plan.bx, plan.ky, plan.by)
    if hpass:
        _table(plan.kx, (Wout, plan.ksx), "kx")
        _table(plan.bx, (Wout, 2), "bx")
    if vpass:
        _table(plan.ky, (Hout, plan.ksy), "ky")
        _table(plan.by, (Hout, 2), "by")
    if plan.lut.dtype != torch.float32 or tuple(plan.lut.shape) != (C, 256) or not plan.lut.is_contiguous():
        raise RuntimeError("ingest_clips: plan.lut must be a contiguous float32 [%d, 256] tensor" % C)
    if flips is not None and (flips.dtype != torch.int32 or tuple(flips.shape) != (N,) or not flips.is_contiguous()):
        raise RuntimeError("ingest_clips: flips must be a contiguous int32 [%d] tensor, got %s %s" % (N, flips.dtype, tuple(flips.shape)))

    two = split is not None or (outs is not None and len(outs) == 2)
    if split is None:
        Tp = int(outs[0].shape[1]) if two and outs[0].dim() == 5 else T
    elif isinstance(split, (tuple, list)):
        if len(split) != 2 or int(split[0]) + int(split[1]) != T:
            raise RuntimeError("ingest_clips: split %s must be (Tp, Tf) with Tp + Tf == T = %d" % (tuple(split), T))
        Tp = int(split[0])
    else:
        Tp = int(split)
    if not 0 <= Tp <= T:
        raise RuntimeError("ingest_clips: split Tp %d is outside 0 .. T = %d" % (Tp, T))
    shapes = [(N, Tp, C, Hout, Wout), (N, T - Tp, C, Hout, Wout)] if two else [(N, T, C, Hout, Wout)]
    if outs is None:
        outs = tuple(torch.empty(s, device=raw.device, dtype=torch.float32) for s in shapes)
    else:
        if len(outs) != len(shapes):
            raise RuntimeError("ingest_clips: a split needs a pair of out tensors")
        for o, s in zip(outs, shapes):
            if o.dtype != torch.float32 or tuple(o.shape) != s or not o.is_contiguous():
                raise RuntimeError("ingest_clips: out must be contiguous float32 %s, got %s %s" % (list(s), o.dtype, tuple(o.shape)))
    o0 = outs[0] if Tp > 0 else None
    o1 = outs[1] if two and Tp < T else None
    check(lib.vptr_clip_ingest(ptr(raw), ptr(plan.kx) if hpass else None, ptr(plan.bx) if hpass else None, ptr(plan.ky) if vpass else None,
                               ptr(plan.by) if vpass else None, ptr(plan.lut), ptr(flips), ptr(o0), ptr(o1), N, T, Tp, Hin, Win, C,
                               top, left, Hc, Wc, Hout, Wout, plan.ksx if hpass else 0, plan.ksy if vpass else 0, stream()),
          "vptr_clip_ingest")
    return (outs[0], outs[1]) if two else outs[0]
