"""Per-tensor statistics of the optimizer's slabs as one call of two launches (csrc/tensor_stats.hip, include/vptr_hip_diag.h)."""

import torch

from .. import _lib
from .._lib import check, lib, ptr, stream


def tensor_stats(p, g, m, v, seg_off, item_first, S, scale_dev, state, ctl, table, ws, grid_cap=0):
    """p, g (and m, v with state, or all three None): fp32 device slabs; seg_off int64 [S + 1], item_first int32 [S + 1]: the plan of
    `vptr_amd.diagnostics.plan` on the device; scale_dev: a one-element fp32 device view or None; ctl fp32 [16], table fp32 [S + 1, 8],
    ws: the partial records.  Writes table and ctl in stream order; no host sync.  The library checks pointers and alignment; the
    shapes and dtypes that it cannot see are checked here."""
    _lib.require_cuda(p, g, m, v, seg_off, item_first, scale_dev, state, ctl, table, ws)
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("scale_dev", scale_dev), ("state", state), ("ctl", ctl), ("table", table)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("tensor_stats: %s must be a contiguous float32 tensor" % name)
    if seg_off.dtype != torch.int64 or item_first.dtype != torch.int32 or seg_off.numel() != S + 1 or item_first.numel() != S + 1:
        raise RuntimeError("tensor_stats: seg_off must be int64 and item_first int32, both of S + 1 = %d entries" % (S + 1))
    if table.numel() != (S + 1) * 8 or ctl.numel() != 16:
        raise RuntimeError("tensor_stats: table must hold (S + 1) * 8 = %d words and ctl 16" % ((S + 1) * 8))
    check(lib.vptr_tensor_stats(ptr(p), ptr(g), ptr(m), ptr(v), ptr(seg_off), ptr(item_first), int(S), ptr(scale_dev), ptr(state), ptr(ctl),
                                ptr(table), ptr(ws), ws.numel() * ws.element_size(), int(grid_cap), stream()), "vptr_tensor_stats")
