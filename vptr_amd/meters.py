"""Epoch loss meters: the reference's `AverageMeters` / `BatchAverageMeter` / `gather_AverageMeters`
(utils/train_summary.py:41-91, 237-260) as host classes for scripts that keep their `.item()` loop, and `DeviceLossMeters`, which
keeps the same records on the device: `update()` is one `vptr_meters_add` launch (csrc/meters.hip) on the 0-dim tensors a trainer's
`step` / `eval_step` returns, and `compute()` is the one host sync of an epoch.

This module imports without the HIP library; the library is loaded when the first `DeviceLossMeters` with the default backend is built.
"""
import ctypes
import math

import torch

MAX_TERMS = 16
ROW = 8                                   # doubles per term: sum, sumsq, count, nonfinite, last, 3 reserved
SUM, SUMSQ, COUNT, NONFINITE, LAST = 0, 1, 2, 3, 4


# ---- host classes --------------------------------------------------------------------------------------------------------------
class BatchAverageMeter(object):
    """value / running average of one loss term (utils/train_summary.py:237-260)"""

    def __init__(self, name, fmt=":f"):
        self.name = name
        self.fmt = fmt
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def __str__(self):
        return ("{name} {val" + self.fmt + "} ({avg" + self.fmt + "})").format(**self.__dict__)


def _epoch_update(avg_of, loss_dict, epoch, train_flag):
    """AverageMeters.epoch_update (utils/train_summary.py:52-71): append each term's average to the train or val history; entries of
    `loss_dict` that are no histories ('epochs') are skipped, a history with no meter gets 0"""
    for k, v in loss_dict.items():
        hist = getattr(v, "train" if train_flag else "val", None)
        if hist is None:
            continue
        try:
            hist.append(avg_of(k))
        except KeyError:
            hist.append(0)
    loss_dict["epochs"] = epoch
    return loss_dict


class AverageMeters(object):
    """one BatchAverageMeter per loss name (utils/train_summary.py:41-71)"""

    def __init__(self, loss_name_list):
        self.loss_name_list = loss_name_list
        self.meters = {name: BatchAverageMeter(name, ":.10e") for name in loss_name_list}

    def iter_update(self, iter_loss_dict):
        for k, v in iter_loss_dict.items():
            self.meters[k].update(v)

    def epoch_update(self, loss_dict, epoch, train_flag=True):
        return _epoch_update(lambda k: self.meters[k].avg, loss_dict, epoch, train_flag)


def gather_AverageMeters(aveMeter_list):
    """the mean over ranks of each term's average (utils/train_summary.py:73-91); only `.avg` of the result is meaningful"""
    names = aveMeter_list[0].loss_name_list
    out = AverageMeters(names)
    for name in names:
        total = 0
        for am in aveMeter_list:
            total += am.meters[name].avg
        out.meters[name].avg = total / len(aveMeter_list)
    return out


# ---- device meter --------------------------------------------------------------------------------------------------------------
class _HipAdd:
    """default backend of DeviceLossMeters: vptr_meters_add.  The host array of source pointers is rebuilt only when a term's address
    changes, so a loop over graph replays (static output tensors) pays one ctypes call per update."""

    def __init__(self):
        from ._lib import check, lib, stream
        self._check, self._fn, self._stream = check, lib.vptr_meters_add, stream
        self._key, self._arr = None, None

    def __call__(self, terms, state, weight):
        key = tuple(0 if t is None else t.data_ptr() for t in terms)
        if key != self._key:
            self._arr = (ctypes.c_void_p * len(key))(*[p or None for p in key])
            self._key = key
        self._check(self._fn(self._arr, len(key), ctypes.c_void_p(state.data_ptr()), float(weight), self._stream()), "vptr_meters_add")


class DeviceLossMeters:
    """Per-term running records ([K, 8] fp64: sum, sum of squares, count, non-finite count, last value) of up to 16 loss terms.

    names: the loss names (a `loss_name_list`); `ignore`: keys a step returns that are deliberately not metered ('grad_norm' and what a
    step with optimizer controls adds, 'lr' / 'skipped' ...; any of them is metered when it is listed in `names`).
    add: backend `add(terms, state, weight)` with `terms` the K tensors in row order (None = absent); default: the HIP kernel."""

    def __init__(self, names, device, ignore=("grad_norm", "lr", "skipped", "lr_G", "lr_D", "skipped_G", "skipped_D", "applied"), add=None):
        self.names = list(names)
        if not 1 <= len(self.names) <= MAX_TERMS or len(set(self.names)) != len(self.names):
            raise ValueError("DeviceLossMeters: 1 .. %d distinct names, got %r" % (MAX_TERMS, self.names))
        self.ignore = frozenset(ignore) - set(self.names)
        self.device = torch.device(device)
        self.state = torch.zeros((len(self.names), ROW), dtype=torch.float64, device=self.device)
        self._row = {n: i for i, n in enumerate(self.names)}
        self._add = add if add is not None else _HipAdd()

    def update(self, terms, n=1):
        """fold one step's terms in (weight n, BatchAverageMeter.update(val, n)): one launch, no allocation, no sync.  Names missing
        from `terms` keep their records; a key that is neither a name nor ignored raises."""
        row = [None] * len(self.names)
        for k, t in terms.items():
            i = self._row.get(k)
            if i is None:
                if k in self.ignore:
                    continue
                raise KeyError("DeviceLossMeters: no meter named %r (names: %r)" % (k, self.names))
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != self.state.device:
                raise TypeError("DeviceLossMeters: term %r must be a one-element float32 tensor on %s" % (k, self.state.device))
            row[i] = t
        if not (math.isfinite(n) and n > 0):
            raise ValueError("DeviceLossMeters: n %r must be finite and positive" % (n,))
        self._add(row, self.state, n)

    def reset(self):
        """zero the records (stream-ordered).  Not for use inside a graph capture: a memset node is not replay-safe on this runtime."""
        if self.state.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DeviceLossMeters.reset() inside a graph capture")
        self.state.zero_()

    # -- the one host read of an epoch -------------------------------------------------------------------------------------------
    @staticmethod
    def _summary(sum_, sumsq, count, last, nonfinite):
        if count > 0:
            avg = sum_ / count
            var = sumsq / count - avg * avg
            std = math.sqrt(var) if var > 0 else (var if var != var else 0.0)
        else:
            avg, std = 0, 0.0          # BatchAverageMeter before its first update
        return {"avg": avg, "sum": sum_, "count": count, "std": std, "last": last, "nonfinite": int(nonfinite)}

    def compute(self, group=None, across="ranks_mean"):
        """-> {name: {avg, sum, count, std, last, nonfinite}} (std: population, count-weighted).  With a process group the ranks' records
        are all-gathered first: across="ranks_mean" averages the ranks' averages (gather_AverageMeters' rule: sum / count / std / last
        are then this rank's own, nonfinite is the total), across="samples" pools sums over pooled counts."""
        if across not in ("ranks_mean", "samples"):
            raise ValueError("DeviceLossMeters.compute: across must be 'ranks_mean' or 'samples'")
        states = [self.state]
        if group is not None and torch.distributed.get_world_size(group) > 1:
            states = [torch.empty_like(self.state) for _ in range(torch.distributed.get_world_size(group))]
            torch.distributed.all_gather(states, self.state, group=group)
        own = self.state.cpu().tolist()
        ranks = [own] if len(states) == 1 else [s.cpu().tolist() for s in states]
        out = {}
        for i, name in enumerate(self.names):
            if across == "samples" and len(ranks) > 1:
                rec = self._summary(sum(r[i][SUM] for r in ranks), sum(r[i][SUMSQ] for r in ranks), sum(r[i][COUNT] for r in ranks),
                                    own[i][LAST], sum(r[i][NONFINITE] for r in ranks))
            else:
                rec = self._summary(own[i][SUM], own[i][SUMSQ], own[i][COUNT], own[i][LAST], sum(r[i][NONFINITE] for r in ranks))
                if len(ranks) > 1:
                    total = 0
                    for r in ranks:
                        total += self._summary(r[i][SUM], r[i][SUMSQ], r[i][COUNT], r[i][LAST], 0)["avg"]
                    rec["avg"] = total / len(ranks)
            out[name] = rec
        return out

    def epoch_update(self, loss_dict, epoch, train_flag=True, group=None, across="ranks_mean"):
        """AverageMeters.epoch_update on the device records (one `compute()`): the result goes straight into checkpoint.save_ckpt"""
        res = self.compute(group, across)
        return _epoch_update(lambda k: res[k]["avg"], loss_dict, epoch, train_flag)
