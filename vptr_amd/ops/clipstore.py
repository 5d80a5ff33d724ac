"""The HBM-resident clip store as two kernel calls (csrc/clipstore.hip, include/vptr_hip_data.h): `clip_draw` writes which clips form the
next batch from a device cursor, `ingest_gather` is `ingest_clips` reading its frames out of the store through that table."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream
from .ingest import INGEST_MAX_KSIZE, INGEST_MAX_OUT, _table

CURSOR_WORDS = 16        # VPTR_CUR_WORDS
SEL_WORDS = 4            # VPTR_SEL_WORDS


def _i32(t, shape, what, who):
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous int32 %s tensor, got %s %s" % (who, what, list(shape), t.dtype, tuple(t.shape)))


def clip_draw(cursor, clip_table, sel, rank=0, world=1, shuffle=True, hflip_p=0.0, vflip_p=0.0):
    """cursor: int32 [16] device record (include/vptr_hip_data.h), 64-byte aligned; clip_table: int32 [n_clips, 2]; sel: int32 [N, 4],
    written with {first past frame, first future frame, flip bits, clip id} of this rank's N clips of the cursor's batch; the cursor
    moves on by one batch.  One launch of one workgroup, no host sync."""
    _lib.require_cuda(cursor, clip_table, sel)
    _i32(cursor, (CURSOR_WORDS,), "cursor", "clip_draw")
    if clip_table.dim() != 2:
        raise RuntimeError("clip_draw: clip_table must be int32 [n_clips, 2]")
    _i32(clip_table, (clip_table.shape[0], 2), "clip_table", "clip_draw")
    if sel.dim() != 2:
        raise RuntimeError("clip_draw: sel must be int32 [N, 4]")
    _i32(sel, (sel.shape[0], SEL_WORDS), "sel", "clip_draw")
    check(lib.vptr_clip_draw(ptr(cursor), ptr(clip_table), ptr(sel), int(clip_table.shape[0]), int(sel.shape[0]), int(rank), int(world),
                             1 if shuffle else 0, float(hflip_p), float(vflip_p), stream()), "vptr_clip_draw")
    return sel


def ingest_gather(store, sel, plan, split, out=None):
    """store: uint8 device tensor [F, Hin, Win, C]; sel: int32 device tensor [N, 4] (`clip_draw`, or written by the host); plan: a
    `vptr_amd.data.IngestPlan`; split: (Tp, Tf) -> the (past [N, Tp, C, Hout, Wout], future [N, Tf, C, Hout, Wout]) fp32 tensors,
    bit-identical to `ingest_clips` on the gathered batch.  out: a pair of tensors to write into (a trainer's static graph inputs).
    One launch, no host sync, no autograd."""
    Hin, Win = plan.in_hw
    C = plan.channels
    _lib.require_cuda(store, sel, plan.lut)
    if store.dtype != torch.uint8 or store.dim() != 4 or tuple(store.shape[1:]) != (Hin, Win, C) or store.shape[0] < 1 or not store.is_contiguous():
        raise RuntimeError("ingest_gather: store %s %s must be contiguous uint8 (F, %d, %d, %d) with F >= 1 for this plan"
                           % (store.dtype, tuple(store.shape), Hin, Win, C))
    if sel.dim() != 2 or sel.shape[0] < 1:
        raise RuntimeError("ingest_gather: sel must be int32 [N, 4] with N >= 1")
    _i32(sel, (sel.shape[0], SEL_WORDS), "sel", "ingest_gather")
    N = int(sel.shape[0])
    Tp, Tf = int(split[0]), int(split[1])
    if Tp < 0 or Tf < 0 or Tp + Tf < 1:
        raise RuntimeError("ingest_gather: split %s must be (Tp, Tf), both >= 0 and not both 0" % (tuple(split),))
    T = Tp + Tf
    top, left, Hc, Wc = plan.crop
    Hout, Wout = plan.out_hw
    if not (1 <= Hout <= INGEST_MAX_OUT and 1 <= Wout <= INGEST_MAX_OUT):
        raise RuntimeError("ingest_gather: output size %d x %d is outside 1 .. %d per axis" % (Hout, Wout, INGEST_MAX_OUT))
    hpass, vpass = Wout != Wc, Hout != Hc
    if (hpass and not 1 <= plan.ksx <= INGEST_MAX_KSIZE) or (vpass and not 1 <= plan.ksy <= INGEST_MAX_KSIZE):
        raise RuntimeError("ingest_gather: ksize (%d, %d) is outside 1 .. %d: a downscale of at most 8x per axis is supported"
                           % (plan.ksx, plan.ksy, INGEST_MAX_KSIZE))
    if (hpass and (plan.kx is None or plan.bx is None)) or (vpass and (plan.ky is None or plan.by is None)):
        raise RuntimeError("ingest_gather: the plan has no tables for a pass it needs")
    _lib.require_cuda(plan.kx, plan.bx, plan.ky, plan.by)
    if hpass:
        _table(plan.kx, (Wout, plan.ksx), "kx")
        _table(plan.bx, (Wout, 2), "bx")
    if vpass:
        _table(plan.ky, (Hout, plan.ksy), "ky")
        _table(plan.by, (Hout, 2), "by")
    if plan.lut.dtype != torch.float32 or tuple(plan.lut.shape) != (C, 256) or not plan.lut.is_contiguous():
        raise RuntimeError("ingest_gather: plan.lut must be a contiguous float32 [%d, 256] tensor" % C)
    shapes = [(N, Tp, C, Hout, Wout), (N, Tf, C, Hout, Wout)]
    if out is None:
        outs = tuple(torch.empty(s, device=store.device, dtype=torch.float32) for s in shapes)
    else:
        outs = tuple(out)
        if len(outs) != 2:
            raise RuntimeError("ingest_gather: out must be a pair of tensors")
        _lib.require_cuda(*outs)
        for o, s in zip(outs, shapes):
            if o.dtype != torch.float32 or tuple(o.shape) != s or not o.is_contiguous():
                raise RuntimeError("ingest_gather: out must be contiguous float32 %s, got %s %s" % (list(s), o.dtype, tuple(o.shape)))
    check(lib.vptr_clip_ingest_gather(ptr(store), int(store.shape[0]), ptr(sel), ptr(plan.kx) if hpass else None, ptr(plan.bx) if hpass else None,
                                      ptr(plan.ky) if vpass else None, ptr(plan.by) if vpass else None, ptr(plan.lut),
                                      ptr(outs[0]) if Tp > 0 else None, ptr(outs[1]) if Tf > 0 else None, N, T, Tp, Hin, Win, C, top, left,
                                      Hc, Wc, Hout, Wout, plan.ksx if hpass else 0, plan.ksy if vpass else 0, stream()),
          "vptr_clip_ingest_gather")
    return outs[0], outs[1]
