"""Device-resident optimizer controls: learning-rate schedules and the non-finite skip of `train.FlatAdamW` (csrc/optim.hip,
include/vptr_hip_optim.h), its accumulation window and EMA (include/vptr_hip_accum.h) and its parameter groups (include/vptr_hip_groups.h).

`vptr_adamw` takes its hyper-parameters by value, so a captured step (`NARTrainer.capture`) freezes them into the graph.  With controls the
hyper-parameters live in a 64-byte device record (`hyper`); `vptr_optim_prepare` -- one single-lane launch behind the gradient's sum of
squares -- decides whether the step is usable, advances the step counter, evaluates the schedule and leaves the launch-uniform scalars of
the update in a second record (`state`), which `vptr_adamw_ctl` reads.  Everything the host changes is a stream-ordered write of a `hyper`
word, so it takes effect on the next step whether that step is eager or a graph replay.

`LRSchedule` is the host mirror of the schedule the kernel evaluates: `base_lr * schedule.factor(k)` is the rate of the update that follows
k applied updates, which is what `torch.optim.lr_scheduler.LambdaLR(opt, schedule.factor)` gives with `scheduler.step()` after each
`optimizer.step()`.
"""
import math

import numpy as np
import torch

from ._lib import check, lib, ptr, stream

# word indices of the two records (include/vptr_hip_optim.h)
H_BASE_LR, H_BETA1, H_BETA2, H_EPS, H_WEIGHT_DECAY, H_MAX_NORM, H_GRAD_SCALE, H_SKIP_NONFINITE = range(8)
H_SCHED_KIND, H_WARMUP_STEPS, H_TOTAL_STEPS, H_MIN_RATIO = range(8, 12)
S_LR_NOW, S_GRAD_NORM, S_SKIP_NOW, S_SKIPPED_TOTAL, S_SKIPPED_IN_A_ROW, S_COEF, S_STEP_SIZE, S_INV_SQRT_BC2, S_DECAY, S_OB1, S_OB2 = range(11)
S_BETA1, S_BETA2, S_EPS = 11, 12, 13
# word indices of the third record, `window` (include/vptr_hip_accum.h): words 0 .. 7 are the host's, 8 .. 15 the device's
W_ACCUM_STEPS, W_EMA_DECAY, W_EMA_WARMUP = range(3)
W_MICRO, W_APPLY_NOW, W_EMA_OMD, W_EMA_UPDATES = range(8, 12)
# the group tables (include/vptr_hip_groups.h): ghyper[G][4] = {lr_scale, weight_decay, -, -}, gstate[G][4] = {step_size, decay, lr, -}
MAX_GROUPS, G_WORDS = 16, 4
G_LR_SCALE, G_WEIGHT_DECAY = 0, 1
GS_STEP_SIZE, GS_DECAY, GS_LR = 0, 1, 2
SCALE_KEY = "vptr_lr_scale"   # the key `FlatAdamW.state_dict` adds to every group of a grouped optimizer
SKIP_HOLD = 2.0            # state[S_SKIP_NOW] while a window is open (0 apply, 1 skipped)
WORDS = 16
MAX_STEPS = 1 << 24        # W and S travel as fp32 words, and the step counter is an fp32 too: whole numbers are exact below 2^24

KINDS = ("constant", "linear", "cosine")
STATE_KEY = "vptr_controls"   # the key `FlatAdamW.state_dict` adds to param_groups[0]


def _f32(x):
    return float(np.float32(x))


class LRSchedule:
    """Warm-up + decay as a factor on the base rate.  With k the number of updates already applied, W = warmup_steps, S = total_steps,
    r = min_ratio:

        k < W:   factor = (k + 1) / W                               (linear warm-up that ends at 1, never starts at 0)
        else     t = min(1, (k - W) / max(1, S - W))
                 constant: 1;   linear: 1 - (1 - r) t;   cosine: r + (1 - r) (1 + cos(pi t)) / 2

    so the factor stays at r from k = S on.  `total_steps` may be omitted for the constant kind only.  `min_ratio` is held as the fp32
    value the device record stores, so `factor` is the exact mirror of what the kernel evaluates (in fp64, like here)."""

    def __init__(self, kind="constant", warmup_steps=0, total_steps=None, min_ratio=0.0):
        if kind not in KINDS:
            raise ValueError("LRSchedule: kind must be one of %r, got %r" % (KINDS, kind))
        for name, val in (("warmup_steps", warmup_steps), ("total_steps", total_steps)):
            if val is None and name == "total_steps":
                continue
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or not 0 <= val < MAX_STEPS:
                raise ValueError("LRSchedule: %s must be a whole number in [0, 2^24), got %r" % (name, val))
        if total_steps is None:
            if kind != "constant":
                raise ValueError("LRSchedule: kind %r needs total_steps" % kind)
            total_steps = warmup_steps
        if total_steps < warmup_steps:
            raise ValueError("LRSchedule: total_steps %d is below warmup_steps %d" % (total_steps, warmup_steps))
        if isinstance(min_ratio, bool) or not isinstance(min_ratio, (int, float, np.floating)) or not (math.isfinite(min_ratio) and 0.0 <= min_ratio <= 1.0):
            raise ValueError("LRSchedule: min_ratio must be a number in [0, 1], got %r" % (min_ratio,))
        self.kind, self.warmup_steps, self.total_steps, self.min_ratio = kind, int(warmup_steps), int(total_steps), _f32(min_ratio)

    def factor(self, k):
        """the factor of the update that follows k applied updates (Python floats)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError("LRSchedule.factor: k must be a whole number >= 0, got %r" % (k,))
        W, S, r = self.warmup_steps, self.total_steps, self.min_ratio
        if k < W:
            return (k + 1.0) / W
        if self.kind == "constant":
            return 1.0
        t = min(1.0, (k - W) / max(1.0, float(S - W)))
        if self.kind == "linear":
            return 1.0 - (1.0 - r) * t
        return r + (1.0 - r) * (1.0 + math.cos(math.pi * t)) / 2.0

    def words(self):
        """(sched_kind, W, S, r) as the `hyper` record holds them"""
        return float(KINDS.index(self.kind)), float(self.warmup_steps), float(self.total_steps), self.min_ratio

    def to_dict(self):
        return {"kind": self.kind, "warmup_steps": self.warmup_steps, "total_steps": self.total_steps, "min_ratio": self.min_ratio}

    @classmethod
    def from_dict(cls, d):
        return cls(d["kind"], d["warmup_steps"], d["total_steps"], d["min_ratio"])

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "LRSchedule(kind=%r, warmup_steps=%d, total_steps=%d, min_ratio=%r)" % (self.kind, self.warmup_steps, self.total_steps, self.min_ratio)


def _finite(name, x, lo=None, lo_open=False, hi=None, hi_open=False):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)) or not math.isfinite(x):
        raise ValueError("optimizer controls: %s must be a finite number, got %r" % (name, x))
    if lo is not None and (x <= lo if lo_open else x < lo) or hi is not None and (x >= hi if hi_open else x > hi):
        raise ValueError("optimizer controls: %s = %r is out of range" % (name, x))
    return float(x)


class Record:
    """A device record the host writes: the device view `dev`, the host's mirror of what it last wrote into each word, and `put` -- one
    fill kernel per CHANGED word (stream-ordered, no memset node, no host buffer whose lifetime a graph would have to care about).  The
    kernels need the record 64-byte aligned; a device-written record that follows it in the same buffer at a multiple of 64 bytes is
    aligned with it."""

    def __init__(self, dev, what="record"):
        if dev.data_ptr() % 64:
            raise RuntimeError("optimizer controls: the allocator returned a %s that is not 64-byte aligned" % what)
        self.dev, self.host = dev, [None] * dev.numel()

    def put(self, idx, value):
        value = _f32(value)
        if self.host[idx] != value:
            self.dev[idx:idx + 1].fill_(value)
            self.host[idx] = value


class OptimControls:
    """The device records of one optimizer and the launches on them.  `hyper` is written by the host only (a `Record`); `state` is
    written by the device only, apart from the zeroing here and `load_counters`.

    accum_steps / ema_decay (either one not None) add the third record, `window` (include/vptr_hip_accum.h): gradient accumulation over
    `accum_steps` micro-steps and the EMA of the parameters.  Its words 0 .. 7 are the host's (written through a `Record` as well),
    words 8 .. 15 the device's, apart from the zeroing here, `reset_window` and `load_window`.  `micro_host` mirrors the window position:
    it is deterministic, because neither a hold nor a skipped close moves a window boundary."""

    window = None      # the third record; None: no accumulation window
    micro_host = 0

    def __init__(self, device, lr, betas, eps, weight_decay, max_grad_norm, schedule=None, skip_nonfinite=False, accum_steps=None, ema_decay=None,
                 ema_warmup=True):
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise TypeError("optimizer controls: schedule must be an LRSchedule, got %r" % (schedule,))
        windowed = accum_steps is not None or ema_decay is not None
        buf = torch.zeros((3 if windowed else 2) * WORDS, device=device, dtype=torch.float32)
        self.hyper, self.state = buf[:WORDS], buf[WORDS:2 * WORDS]
        self._put = Record(self.hyper).put
        self.schedule = schedule if schedule is not None else LRSchedule()
        self.skip_nonfinite = bool(skip_nonfinite)
        self.write(lr, betas, eps, weight_decay, max_grad_norm, 1.0)
        if windowed:
            self.window = buf[2 * WORDS:]
            self._wput = Record(self.window).put
            self.accum_steps, self.ema_decay, self.ema_warmup = 1, None, True
            self.set_accum_steps(1 if accum_steps is None else accum_steps)
            self.set_ema_decay(ema_decay, ema_warmup)

    # -- hyper ------------------------------------------------------------------------------------------------------------------
    def write(self, lr, betas, eps, weight_decay, max_grad_norm, grad_scale):
        """validate and write every word"""
        self.set_lr(lr)
        self._put(H_BETA1, _finite("beta1", betas[0], 0.0, False, 1.0, True))
        self._put(H_BETA2, _finite("beta2", betas[1], 0.0, False, 1.0, True))
        self._put(H_EPS, _finite("eps", eps, 0.0))
        self.set_weight_decay(weight_decay)
        self.set_max_grad_norm(max_grad_norm)
        self.set_grad_scale(grad_scale)
        self._put(H_SKIP_NONFINITE, 1.0 if self.skip_nonfinite else 0.0)
        self.set_schedule(self.schedule)

    def set_lr(self, lr):
        self._put(H_BASE_LR, _finite("lr", lr, 0.0))

    def set_weight_decay(self, weight_decay):
        self._put(H_WEIGHT_DECAY, _finite("weight_decay", weight_decay, 0.0))

    def set_max_grad_norm(self, max_grad_norm):
        """None (or a value <= 0): no clipping"""
        self._put(H_MAX_NORM, 0.0 if max_grad_norm is None else max(0.0, _finite("max_grad_norm", max_grad_norm)))

    def set_grad_scale(self, grad_scale):
        self._put(H_GRAD_SCALE, _finite("grad_scale", grad_scale, 0.0, True))

    def set_schedule(self, schedule):
        if schedule is None:
            schedule = LRSchedule()
        if not isinstance(schedule, LRSchedule):
            raise TypeError("optimizer controls: schedule must be an LRSchedule, got %r" % (schedule,))
        self.schedule = schedule
        for idx, w in zip((H_SCHED_KIND, H_WARMUP_STEPS, H_TOTAL_STEPS, H_MIN_RATIO), schedule.words()):
            self._put(idx, w)

    # -- state ------------------------------------------------------------------------------------------------------------------
    def word(self, idx):
        """0-dim fp32 view of a `state` word"""
        return self.state[idx]

    def counters(self):
        """(skipped_total, skipped_in_a_row) read back (one sync)"""
        t, r = self.state[S_SKIPPED_TOTAL:S_SKIPPED_IN_A_ROW + 1].tolist()
        return t, r

    def load_counters(self, total, in_a_row):
        self.state[S_SKIPPED_TOTAL:S_SKIPPED_TOTAL + 1].fill_(float(total))
        self.state[S_SKIPPED_IN_A_ROW:S_SKIPPED_IN_A_ROW + 1].fill_(float(in_a_row))

    # -- window ------------------------------------------------------------------------------------------------------------------
    def _need_window(self, what):
        if self.window is None:
            raise RuntimeError("optimizer controls: %s needs the accumulation window (accum_steps= or ema_decay=)" % what)

    def set_accum_steps(self, k):
        """micro-steps per window; only between windows (the host's mirror of the window position must be 0: see `reset_window`)"""
        self._need_window("set_accum_steps")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k < MAX_STEPS:
            raise ValueError("optimizer controls: accum_steps must be a whole number in [1, 2^24), got %r" % (k,))
        if self.micro_host != 0:
            raise RuntimeError("optimizer controls: accum_steps cannot change inside a window (%d of %d micro-steps are held); finish the "
                               "window or reset_window() first" % (self.micro_host, self.accum_steps))
        self._wput(W_ACCUM_STEPS, float(k))
        self.accum_steps = int(k)

    def set_ema_decay(self, ema_decay, ema_warmup=None):
        """d in [0, 1) (None: the record holds 0, no EMA slab is kept); ema_warmup: d_now = min(d, (1 + u) / (10 + u)) after u updates"""
        self._need_window("set_ema_decay")
        if ema_warmup is not None:
            if not isinstance(ema_warmup, (bool, np.bool_)):
                raise ValueError("optimizer controls: ema_warmup must be True or False, got %r" % (ema_warmup,))
            self.ema_warmup = bool(ema_warmup)
        d = 0.0 if ema_decay is None else _finite("ema_decay", ema_decay, 0.0, False, 1.0, True)
        if _f32(d) >= 1.0:
            raise ValueError("optimizer controls: ema_decay = %r rounds to 1 in fp32" % (ema_decay,))
        self._wput(W_EMA_DECAY, d)
        self._wput(W_EMA_WARMUP, 1.0 if self.ema_warmup else 0.0)
        self.ema_decay = None if ema_decay is None else _f32(d)

    def reset_window(self):
        """drop the open window: a stream-ordered write of MICRO = 0, so the next `begin` zero-fills the gradient slab"""
        self._need_window("reset_window")
        self.window[W_MICRO:W_MICRO + 1].fill_(0.0)
        self.micro_host = 0

    def advance_mirror(self):
        """one micro-step passed (called for every windowed `prepare` that is executed: eager here, per replay by the owner of a graph);
        -> whether that micro-step closed its window"""
        self.micro_host = (self.micro_host + 1) if self.micro_host + 1 < self.accum_steps else 0
        return self.micro_host == 0

    def closes_next(self):
        """whether the next micro-step closes its window (host mirror)"""
        return self.micro_host + 1 >= self.accum_steps

    def wword(self, idx):
        """0-dim fp32 view of a `window` word"""
        self._need_window("wword")
        return self.window[idx]

    def window_counters(self):
        """(micro, ema_updates) read back (one sync)"""
        return float(self.window[W_MICRO]), float(self.window[W_EMA_UPDATES])

    def load_window(self, ema_updates):
        """the device half of the record as a checkpoint load leaves it: window position 0, the EMA update count as saved"""
        self.window[W_MICRO:W_EMA_UPDATES].fill_(0.0)
        self.window[W_EMA_UPDATES:W_EMA_UPDATES + 1].fill_(float(ema_updates))
        self.micro_host = 0

    # -- launches ---------------------------------------------------------------------------------------------------------------
    def begin(self, grad):
        """zero the gradient slab if a window starts, else leave the partial sum (one kernel node)"""
        check(lib.vptr_accum_begin(ptr(grad), grad.numel(), ptr(self.window), stream()), "vptr_accum_begin")

    def prepare(self, step_dev, sumsq_dev):
        """the single-lane launch behind the sum of squares; with a window its accumulating form, which also moves the host's mirror"""
        if self.window is None:
            check(lib.vptr_optim_prepare(ptr(self.hyper), ptr(self.state), ptr(step_dev), ptr(sumsq_dev), stream()), "vptr_optim_prepare")
            return
        check(lib.vptr_optim_prepare_accum(ptr(self.hyper), ptr(self.state), ptr(self.window), ptr(step_dev), ptr(sumsq_dev), stream()),
              "vptr_optim_prepare_accum")
        if not torch.cuda.is_current_stream_capturing():
            self.advance_mirror()

    def update(self, p, g, m, v, n, ema=None, groups=None):
        """the clip + AdamW launch on the scalars `prepare` left; ema: the EMA slab (needs the window), groups: a `GroupTable`"""
        if groups is not None:
            check(lib.vptr_adamw_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), ptr(groups.gid), n, ptr(self.state),
                                        ptr(self.window) if ema is not None else None, ptr(groups.gstate), groups.ngroups, stream()), "vptr_adamw_groups")
        elif ema is not None:
            check(lib.vptr_adamw_ctl_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), n, ptr(self.state), ptr(self.window), stream()), "vptr_adamw_ctl_ema")
        else:
            check(lib.vptr_adamw_ctl(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(self.state), stream()), "vptr_adamw_ctl")


# ---- parameter groups (include/vptr_hip_groups.h, csrc/optim.hip) -------------------------------------------------------------------
def resolve_param_groups(params, param_groups):
    """`FlatAdamW(param_groups=...)` against the optimizer's parameter list -> (group index of every parameter, [(lr_scale, weight_decay
    or None)] per group).  Each entry is a dict {"params": [...], "lr_scale": 1.0, "weight_decay": None}; None inherits the optimizer's
    weight decay.  Parameters no entry lists form group 0 with the defaults (lr_scale 1, inherited decay) and the listed groups follow
    as 1, 2, ...; when every parameter is listed there is no such group and entry i is group i.  ValueError: a parameter in two groups,
    a parameter that is not the optimizer's, an unknown key, more than 16 groups, a non-finite or negative value."""
    if not isinstance(param_groups, (list, tuple)):
        raise ValueError("param_groups must be a list of dicts, got %r" % type(param_groups).__name__)
    index = {id(p): i for i, p in enumerate(params)}
    group_of, specs = [None] * len(params), []
    for j, grp in enumerate(param_groups):
        if not isinstance(grp, dict) or "params" not in grp or set(grp) - {"params", "lr_scale", "weight_decay"}:
            raise ValueError("param_groups[%d] must be a dict with 'params' and optionally 'lr_scale', 'weight_decay', got %r"
                             % (j, sorted(grp) if isinstance(grp, dict) else grp))
        scale = _finite("param_groups[%d]['lr_scale']" % j, grp.get("lr_scale", 1.0), 0.0)
        wd = grp.get("weight_decay")
        if wd is not None:
            wd = _finite("param_groups[%d]['weight_decay']" % j, wd, 0.0)
        for p in grp["params"]:
            i = index.get(id(p))
            if i is None:
                raise ValueError("param_groups[%d] lists a parameter of shape %s that is not one of the optimizer's (trainable) parameters"
                                 % (j, tuple(getattr(p, "shape", ()))))
            if group_of[i] is not None:
                raise ValueError("parameter %d (shape %s) is in param_groups[%d] and param_groups[%d]" % (i, tuple(p.shape), group_of[i], j))
            group_of[i] = j
        specs.append((scale, wd))
    if any(g is None for g in group_of) or not specs:
        group_of, specs = [0 if g is None else g + 1 for g in group_of], [(1.0, None)] + specs
    if len(specs) > MAX_GROUPS:
        raise ValueError("%d parameter groups (the unlisted parameters' group included); at most %d" % (len(specs), MAX_GROUPS))
    return group_of, specs


def group_map(layout, group_of, numel):
    """the byte map of a slab of `numel` elements: layout[i] = (offset, numel, ...) of parameter i, group_of[i] its group; the elements no
    parameter owns (the pad at the slab's end) belong to group 0"""
    gid = torch.zeros(numel, dtype=torch.uint8)
    for (off, n, *_), g in zip(layout, group_of):
        gid[off:off + n] = g
    return gid


_NORMS = (torch.nn.LayerNorm, torch.nn.GroupNorm, torch.nn.modules.batchnorm._NormBase)


def no_decay_names(module):
    """names (as `module.named_parameters()` gives them) of the trainable parameters `no_decay_groups` exempts from weight decay"""
    out = []
    for mod_name, mod in module.named_modules():
        for name, p in mod.named_parameters(recurse=False):
            if p.requires_grad and (isinstance(mod, _NORMS) or name == "bias" or name.endswith("_bias") or name.endswith("bias_table")
                                    or name.startswith("pos_") or name.endswith("_pos")):
                out.append(mod_name + "." + name if mod_name else name)
    return out


def no_decay_groups(module, weight_decay=0.0):
    """The usual AdamW split as a `param_groups` list of one entry: {"params": [...], "weight_decay": weight_decay (0)}; every other
    trainable parameter stays unlisted, i.e. in group 0 with the optimizer's own weight decay.  The rule, on each module's DIRECT
    parameters:
      * every parameter of a normalisation layer (nn.LayerNorm -- the (C, H, W) affines of the conv-FFNs that the slab stores
        channel-last included --, nn.GroupNorm, the BatchNorm / InstanceNorm family): weight and bias;
      * every parameter named `bias` (or `*_bias`): nn.Linear, nn.Conv2d, nn.MultiheadAttention's in_proj_bias, ...;
      * bias and position TABLES: a parameter whose name ends in `bias_table` (the relative-position bias tables of the local
        attention) or starts with `pos_` / ends in `_pos` (learned absolute position tables).
    Everything else (weight matrices, convolution kernels, the learned frame queries) is decayed.  A parameter shared by two modules is
    listed once."""
    names = set(no_decay_names(module))
    seen, params = set(), []
    for name, p in module.named_parameters():
        if name in names and id(p) not in seen:
            seen.add(id(p))
            params.append(p)
    return [{"params": params, "weight_decay": weight_decay}]


class GroupTable:
    """The group map and the two group tables of one optimizer (include/vptr_hip_groups.h) and the launch that fills `gstate`; the update
    on them is `OptimControls.update(groups=)`.  `ghyper` is written by the host only (a `Record`); `gstate` by the device only."""

    def __init__(self, device, gid, specs, default_weight_decay):
        """gid: uint8 CPU tensor, one group index per slab element; specs: [(lr_scale, weight_decay or None)]"""
        self.ngroups = len(specs)
        if not 1 <= self.ngroups <= MAX_GROUPS:
            raise ValueError("optimizer controls: %d parameter groups, must be 1 .. %d" % (self.ngroups, MAX_GROUPS))
        if gid.dtype != torch.uint8 or int(gid.max()) >= self.ngroups:
            raise ValueError("optimizer controls: the group map must be uint8 with every entry below %d" % self.ngroups)
        self.gid = gid.to(device).contiguous()
        buf = torch.zeros(2 * MAX_GROUPS * G_WORDS, device=device, dtype=torch.float32)
        self.ghyper, self.gstate = buf[:MAX_GROUPS * G_WORDS], buf[MAX_GROUPS * G_WORDS:]
        self._put = Record(self.ghyper, "group table").put
        self.lr_scale, self.weight_decay = [1.0] * self.ngroups, [None] * self.ngroups     # weight_decay None: inherits the default
        self._default = _finite("weight_decay", default_weight_decay, 0.0)
        for g, (scale, wd) in enumerate(specs):
            self.set(g, scale, wd, inherit=wd is None)

    def _group(self, g):
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= g < self.ngroups:
            raise ValueError("optimizer controls: group %r is not one of 0 .. %d" % (g, self.ngroups - 1))
        return int(g)

    def set(self, g, lr_scale=None, weight_decay=None, inherit=False):
        """stream-ordered writes of group g's record words (None: leave as it is; inherit: follow the optimizer's weight decay again)"""
        g = self._group(g)
        if lr_scale is not None:
            self.lr_scale[g] = _finite("lr_scale", lr_scale, 0.0)
            self._put(g * G_WORDS + G_LR_SCALE, self.lr_scale[g])
        if inherit or weight_decay is not None:
            self.weight_decay[g] = None if inherit else _finite("weight_decay", weight_decay, 0.0)
            self._put(g * G_WORDS + G_WEIGHT_DECAY, self.decay_of(g))

    def decay_of(self, g):
        return self._default if self.weight_decay[g] is None else self.weight_decay[g]

    def set_default_weight_decay(self, weight_decay):
        """the optimizer's own weight decay changed: the groups that inherit it follow"""
        self._default = _finite("weight_decay", weight_decay, 0.0)
        for g in range(self.ngroups):
            if self.weight_decay[g] is None:
                self._put(g * G_WORDS + G_WEIGHT_DECAY, self._default)

    def lr(self, g):
        """0-dim fp32 device view: the rate group g used in the last applied step (0 before the first)"""
        return self.gstate[self._group(g) * G_WORDS + GS_LR]

    def scalars(self, state):
        """lane g: group g's step size and decay from the scalars a prepare launch just left in `state`"""
        check(lib.vptr_optim_group_scalars(ptr(state), ptr(self.ghyper), ptr(self.gstate), self.ngroups, stream()), "vptr_optim_group_scalars")
