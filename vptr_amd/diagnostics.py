"""Per-tensor gradient, weight and update statistics of a `train.FlatAdamW` on the device (csrc/tensor_stats.hip,
include/vptr_hip_diag.h): `FlatAdamW(..., tensor_stats=TensorStats(every=1, moments=True, on_skip=True), names=None)` and the same argument
on `NARTrainer` / `FARTrainer`.

The optimizer's tensors are contiguous segments of its four slabs.  One call -- two launches, fixed order, capturable -- right behind the
update kernel leaves a `[S + 1, 8]` fp32 table on the device: per tensor (and, in row S, for the whole slab) the gradient and weight norms
and maxima, the rms of the Adam direction and the non-finite counts.  A control record decides on the device whether a call computes
(`every`: the last call of every k; `on_skip`: also every step the non-finite skip refused), so a captured step samples every n-th replay
without being captured again, and `set_every` / `set_on_skip` are stream-ordered one-word writes that reach the next replay.

This module holds what needs no device: the configuration, the plan (segment and item tables) with its validation, and the word indices.
`TensorStatsState` is the object an optimizer exposes as `opt.tensor_stats`.
"""
import numpy as np
import torch

CHUNK = 4096                 # VPTR_TS_CHUNK: elements per work item
MAX_TENSORS = 65535          # VPTR_TS_MAX_TENSORS
ROW_WORDS = 8
COLUMNS = ("grad_norm", "weight_norm", "grad_maxabs", "weight_maxabs", "dir_rms", "grad_nonfinite", "weight_nonfinite", "numel")
GRAD_NORM, WEIGHT_NORM, GRAD_MAXABS, WEIGHT_MAXABS, DIR_RMS, GRAD_NONFINITE, WEIGHT_NONFINITE, NUMEL = range(8)
CTL_WORDS = 16
C_EVERY, C_ON_SKIP = 0, 1                 # the host's words of the control record
C_PHASE, C_COMPUTED, C_AGE = 8, 9, 10     # the device's
AGE_MAX = 1 << 24
MAX_EVERY = 1 << 24          # EVERY and PHASE travel as fp32 words: whole numbers are exact below 2^24
PART_BYTES = 40              # VPTR_TS_PART_BYTES: one partial record per item


def check_every(every):
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or not 1 <= every < MAX_EVERY:
        raise ValueError("tensor statistics: every must be a whole number in [1, 2^24), got %r" % (every,))
    return int(every)


def _check_flag(name, flag):
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError("tensor statistics: %s must be True or False, got %r" % (name, flag))
    return bool(flag)


class TensorStats:
    """The configuration: every (compute in the last call of every `every`), moments (also read m and v: `dir_rms`, and with it
    `update_ratio`), on_skip (also compute in a step the non-finite skip refused; it reads the optimizer's state record, which travels
    with the moments, so it needs moments=True; None: on where it can be)."""

    def __init__(self, every=1, moments=True, on_skip=None):
        self.every, self.moments = check_every(every), _check_flag("moments", moments)
        self.on_skip = self.moments if on_skip is None else _check_flag("on_skip", on_skip)
        if self.on_skip and not self.moments:
            raise ValueError("tensor statistics: on_skip=True needs moments=True (the skip decision is read from the state record, which the call "
                             "receives together with the moments)")

    def __repr__(self):
        return "TensorStats(every=%d, moments=%r, on_skip=%r)" % (self.every, self.moments, self.on_skip)


def plan(sizes):
    """sizes: the element count of every tensor in slab order -> (seg_off int64 [S + 1], item_first int32 [S + 1]) as CPU tensors.
    ValueError: no tensor, more than 65535, a size that is not a whole number >= 1, or more than 2^31 - 1 items."""
    sizes = list(sizes)
    if not 1 <= len(sizes) <= MAX_TENSORS:
        raise ValueError("tensor statistics: %d tensors, must be 1 .. %d" % (len(sizes), MAX_TENSORS))
    for i, n in enumerate(sizes):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("tensor statistics: tensor %d has %r elements; every tensor needs a whole number >= 1" % (i, n))
    seg_off = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    items = np.concatenate([[0], np.cumsum((np.asarray(sizes, dtype=np.int64) + CHUNK - 1) // CHUNK)])
    if items[-1] >= 1 << 31:
        raise ValueError("tensor statistics: %d work items do not fit an int32 item index" % int(items[-1]))
    seg_off, item_first = torch.from_numpy(seg_off.astype(np.int64)), torch.from_numpy(items.astype(np.int32))
    validate_plan(seg_off, item_first)
    return seg_off, item_first


def validate_plan(seg_off, item_first):
    """what the kernels rely on and cannot check (both tables are device memory there)"""
    so, it = seg_off.tolist(), item_first.tolist()
    if seg_off.dtype != torch.int64 or item_first.dtype != torch.int32 or len(so) != len(it) or not 2 <= len(so) <= MAX_TENSORS + 1:
        raise ValueError("tensor statistics: the plan needs an int64 seg_off and an int32 item_first of S + 1 entries, S in 1 .. %d" % MAX_TENSORS)
    if so[0] != 0 or it[0] != 0 or any(b <= a for a, b in zip(so, so[1:])):
        raise ValueError("tensor statistics: seg_off must start at 0 and increase strictly")
    if any(it[i + 1] - it[i] != -(-(so[i + 1] - so[i]) // CHUNK) for i in range(len(so) - 1)):
        raise ValueError("tensor statistics: item_first is not the prefix sum of ceil(n_i / %d)" % CHUNK)


def items_of(seg_off, item_first):
    """the plan spelled out: [(tensor, first element, one past the last element)] per item, in item order"""
    so, it = seg_off.tolist(), item_first.tolist()
    out = []
    for i in range(len(so) - 1):
        for c in range(it[i + 1] - it[i]):
            out.append((i, so[i] + c * CHUNK, min(so[i] + (c + 1) * CHUNK, so[i + 1])))
    return out


def check_names(names, S):
    """names None -> "param_<i>"; ValueError for another length, a non-string or a duplicate"""
    if names is None:
        return ["param_%d" % i for i in range(S)]
    names = list(names)
    if len(names) != S:
        raise ValueError("tensor statistics: %d names for %d tensors" % (len(names), S))
    if any(not isinstance(n, str) for n in names):
        raise ValueError("tensor statistics: names must be strings")
    if len(set(names)) != S:
        seen, dup = set(), None
        for n in names:
            if n in seen:
                dup = n
                break
            seen.add(n)
        raise ValueError("tensor statistics: the name %r appears twice" % dup)
    return names


def column(col):
    if isinstance(col, str):
        if col not in COLUMNS:
            raise ValueError("tensor statistics: no column %r (one of %s)" % (col, ", ".join(COLUMNS)))
        return COLUMNS.index(col)
    if isinstance(col, bool) or not isinstance(col, (int, np.integer)) or not 0 <= col < ROW_WORDS:
        raise ValueError("tensor statistics: column %r is not one of 0 .. %d" % (col, ROW_WORDS - 1))
    return int(col)


class TensorStatsState:
    """`opt.tensor_stats`: the plan, the table, the control record and the workspace of one optimizer on its device, and the call.

    table: the [S + 1, 8] device tensor (row S: the whole slab; columns: `COLUMNS`).  It holds the last COMPUTED call -- `age()` tells
    how many calls ago that was, `computed()` whether the last call was one.  Nothing here enters a state_dict."""

    ROW_ALL = "<all>"

    def __init__(self, device, sizes, names, config):
        from .optim import Record
        if not isinstance(config, TensorStats):
            raise ValueError("tensor_stats must be a vptr_amd.diagnostics.TensorStats, got %r" % (config,))
        seg_off, item_first = plan(sizes)
        self.S = len(seg_off) - 1
        self.names = check_names(names, self.S)
        self.sizes = [int(n) for n in sizes]
        self.total = sum(self.sizes)
        self._index = {n: i for i, n in enumerate(self.names)}
        self.config, self.moments = config, config.moments
        self.items = int(item_first[-1])
        self.seg_off, self.item_first = seg_off.to(device), item_first.to(device)
        self.table = torch.zeros((self.S + 1, ROW_WORDS), device=device, dtype=torch.float32)
        self.ctl = torch.zeros(CTL_WORDS, device=device, dtype=torch.float32)
        self.ws = torch.empty(self.items * PART_BYTES // 8, device=device, dtype=torch.float64)
        if self.table.data_ptr() % 64:
            raise RuntimeError("tensor statistics: the allocator returned a table that is not 64-byte aligned")
        self._put = Record(self.ctl, "tensor-statistics control record").put
        self.every, self.on_skip = None, None
        self.set_every(config.every)
        self.set_on_skip(config.on_skip)
        self.lr_dev, self.lr_index = None, None      # set by the optimizer: the device words holding each tensor's rate (`report`)

    # -- the control record -------------------------------------------------------------------------------------------------------------
    def set_every(self, k):
        """compute in the last call of every k from now on: a stream-ordered one-word write, it reaches the next replay.  The phase
        the device has reached stays; a k at or below it makes the next call due."""
        self._put(C_EVERY, float(check_every(k)))
        self.every = int(k)

    def set_on_skip(self, flag):
        flag = _check_flag("on_skip", flag)
        if flag and not self.moments:
            raise ValueError("tensor statistics: on_skip needs moments=True")
        self._put(C_ON_SKIP, 1.0 if flag else 0.0)
        self.on_skip = flag

    def age(self):
        """calls since the table was last computed (0-dim fp32 device view; 0: the last call computed it)"""
        return self.ctl[C_AGE]

    def computed(self):
        """1 if the last call computed the table, else 0 (0-dim fp32 device view)"""
        return self.ctl[C_COMPUTED]

    # -- the table ------------------------------------------------------------------------------------------------------------------------
    def row(self, name_or_index):
        if isinstance(name_or_index, str):
            if name_or_index == self.ROW_ALL:
                return self.S
            if name_or_index not in self._index:
                raise ValueError("tensor statistics: no tensor named %r" % name_or_index)
            return self._index[name_or_index]
        i = name_or_index
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not -1 <= i <= self.S:
            raise ValueError("tensor statistics: row %r is not one of 0 .. %d (%d or -1: the whole slab)" % (i, self.S, self.S))
        return self.S if i == -1 else int(i)

    def view(self, name_or_index, col="grad_norm"):
        """0-dim fp32 device view of one table word, e.g. a term of `meters.DeviceLossMeters`; the row by name, by index, or "<all>" / -1
        for the whole slab"""
        return self.table[self.row(name_or_index), column(col)]

    def launch(self, p, g, m, v, scale_dev, state, grid_cap=0):
        """the call (two kernel nodes); m, v and state are passed on only with moments"""
        from .ops.diag import tensor_stats
        mom = self.moments
        if any(t.numel() < self.total for t in ((p, g, m, v) if mom else (p, g))):
            raise RuntimeError("tensor statistics: a slab is shorter than the %d elements of the plan" % self.total)
        tensor_stats(p, g, m if mom else None, v if mom else None, self.seg_off, self.item_first, self.S, scale_dev, state if mom else None,
                     self.ctl, self.table, self.ws, grid_cap)

    def _read(self):
        """table (and the rates) in ONE device-to-host copy"""
        parts = [self.table.reshape(-1)]
        if self.lr_dev is not None:
            parts.append(self.lr_dev.reshape(-1))
        host = torch.cat(parts).cpu().double()
        n = (self.S + 1) * ROW_WORDS
        return host[:n].view(self.S + 1, ROW_WORDS), host[n:]

    def report(self, top=None, sort="grad_norm"):
        """one host sync -> a list of dicts, one per tensor (name, index, the eight columns, update_ratio), sorted by `sort` descending
        (NaN first: it is what one looks for); top: only that many.  update_ratio = lr_g * dir_rms * sqrt(numel) / weight_norm, the norm
        of the last update without the decay over the norm of the weights (None without moments or before a rate exists)."""
        if sort != "update_ratio":
            column(sort)
        tab, lrs = self._read()
        out = []
        for i, name in enumerate(self.names):
            d = {"name": name, "index": i}
            d.update({c: float(tab[i, k]) for k, c in enumerate(COLUMNS)})
            ratio = None
            if self.moments and self.lr_index is not None and d["weight_norm"] > 0.0:
                ratio = float(lrs[self.lr_index[i]]) * d["dir_rms"] * d["numel"] ** 0.5 / d["weight_norm"]
            d["update_ratio"] = ratio
            out.append(d)

        def key(d):
            x = d[sort]
            return (0, 0.0) if x is None else ((2, 0.0) if x != x else (1, x))
        out.sort(key=key, reverse=True)
        return out if top is None else out[:int(top)]

    def culprits(self):
        """the names of the tensors whose gradient or weights held a NaN or an Inf when the table was last computed (one host sync)"""
        tab, _ = self._read()
        return [n for i, n in enumerate(self.names) if tab[i, GRAD_NONFINITE] != 0 or tab[i, WEIGHT_NONFINITE] != 0]
