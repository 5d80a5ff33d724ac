"""Training-step recipes of VPTR on the MI355X path.

`NARTrainer.step` reproduces `single_iter` of the reference's stage-2 NAR trainer (train_NAR.py:49-107 and its
data-parallel twin train_NAR_mp.py:132-189): two no-grad encoder passes, transformer + decoder forward,
MSE + GDL + lam_pc * BiPatchNCE, backward, clip_grad_norm_(max_norm) over the transformer parameters, AdamW.

MI355X-first differences in *how* (not *what*):
  * parameters / gradients / Adam moments of the transformer live in three flat fp32 slabs, so that global-norm
    clipping + AdamW are two HIP launches (vptr_sumsq, vptr_adamw) and the data-parallel gradient exchange is a
    handful of large RCCL all-reduces over xGMI instead of 664 small tensors;
  * losses are returned as device tensors (the reference's 8 `.item()` syncs per step are left to the caller);
  * the weight (and bias) gradients of every nn.Linear of a backward pass run as ONE grouped MFMA launch at its end
    (ops.defer_wgrad / vptr_gemm_grouped);
  * `capture()` turns the whole step into one hipGraph (single GPU; bench.py's default launch mode).

`FARTrainer` is the same for `single_iter` of train_FAR.py:48-101, `AETrainer` for the stage-1 auto-encoder + PatchGAN step of
train_AutoEncoder.py:44-78; both NAR and FAR trainers take the optional adversarial branch (`disc=`, `lam_gan=`).

Every trainer also has the `train_flag=False` branch of its `single_iter` as `eval_step` (eval mode, no_grad, nothing a step owns is
written; `capture_eval` makes it a hipGraph of its own), `step` / `eval_step` feed a `meters.DeviceLossMeters` without a host read, and
`run_epoch` is the reference's loop over a loader (train_NAR.py:231-247).

How the two stage-2 trainers are put together (`FARTrainer` subclasses `NARTrainer`):
  * the iteration is sequenced once, `_forward(past, future, train)`: encoder, [train: zero the gradients, BatchNorm-buffer broadcast,]
    transformer, decoder, discriminator terms (`_disc_update` / `_eval_disc`), recipe loss terms, generator's adversarial term.  A recipe
    contributes `_encode` (what is encoded and fed to the transformer) and `_loss_terms`; `_step_impl` adds backward + exchange + optimizer
    (`_finish`), `_eval_forward` is the same pass under `_eval_impl`'s eval mode;
  * `capture`, `capture_front` and `capture_eval` are ONE procedure, `_capture` (warm-up on a side stream, pinned staging for the table
    uploads, capture, node census, instantiate), parameterised by the warm-up pass, the captured body, whether the weight-gradient tuning is
    waited for and settled, and whether a process group's watchdog thread runs beside the capture; `_replay` is the one replay prologue.
"""
import contextlib
import os
import time

import torch
import torch.nn.functional as F

from . import ops
from ._lib import check, lib, ptr, stream
from .diagnostics import TensorStats, TensorStatsState
from .model.criterion import GDL, GANLoss, L1Loss, MSELoss, temporal_weight_func
from .optim import (GS_LR, H_GRAD_SCALE, G_WORDS, S_GRAD_NORM, S_LR_NOW, S_SKIPPED_IN_A_ROW, S_SKIPPED_TOTAL, SCALE_KEY, STATE_KEY, W_APPLY_NOW, W_MICRO, GroupTable, LRSchedule, OptimControls,
                    group_map, resolve_param_groups)


_HIP_NODE_TYPES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait_event", 7: "event_record",
                   10: "mem_alloc", 11: "mem_free"}


def graph_node_census(g):
    """{node type: count} of a torch.cuda.CUDAGraph captured with keep_graph=True (hipGraphGetNodes / hipGraphNodeGetType on the
    runtime torch itself loaded)"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    graph = ctypes.c_void_p(int(g.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    if n.value and hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    out = {}
    for i in range(n.value):
        t = ctypes.c_int(-1)
        if hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        name = _HIP_NODE_TYPES.get(t.value, "type%d" % t.value)
        out[name] = out.get(name, 0) + 1
    return out


def _copy_into(dst, src):
    """fill a captured graph's static input; a no-op when the caller wrote into that very tensor (`static_inputs`)"""
    if src is not dst:
        dst.copy_(src)


DP_CHUNKS = 4  # grouped weight-gradient launches per step when gradients are exchanged between ranks


class ReconLoss:
    """Configuration of a trainer's reconstruction loss (`recon=`): which point-wise criterion joins the total, the exponent of the
    gradient-difference loss and the per-frame weights of either -- `MSELoss(temporal_weight)`, `L1Loss(temporal_weight)` and
    `GDL(alpha, temporal_weight)` of model/criterion.py on the kernels of csrc/recon_loss.hip (`ops.recon_losses`).

    point: "mse", "l1" or "mse+l1" (what the total contains; both values are always reported, the one outside the total gets no
        gradient).  gdl_alpha: finite, >= 1 (the criterion class accepts less; its gradient is NaN at every tie).
    temporal_weight: None, "exp" (`temporal_weight_func(T)` for the T the trainer's loss sees) or a 1-D tensor / sequence of T values.
    gdl_temporal_weight: the same choices for the GDL; "same" (the default) reuses `temporal_weight`.
    No `norm_dim`: the normalised variants stay with the torch classes."""
    POINTS = ("mse", "l1", "mse+l1")
    SAME = "same"

    def __init__(self, point="mse", gdl_alpha=1.0, temporal_weight=None, gdl_temporal_weight=SAME):
        if point not in self.POINTS:
            raise ValueError("ReconLoss: point must be one of %s (got %r)" % (self.POINTS, point))
        if isinstance(gdl_alpha, bool) or not isinstance(gdl_alpha, (int, float)) or not 1.0 <= float(gdl_alpha) < float("inf"):
            raise ValueError("ReconLoss: gdl_alpha must be a finite number >= 1 (got %r)" % (gdl_alpha,))
        self.point, self.gdl_alpha = point, float(gdl_alpha)
        self.temporal_weight = self._spec(temporal_weight, "temporal_weight")
        self.gdl_temporal_weight = self.temporal_weight if isinstance(gdl_temporal_weight, str) and gdl_temporal_weight == self.SAME \
            else self._spec(gdl_temporal_weight, "gdl_temporal_weight")

    @staticmethod
    def _spec(w, name):
        if w is None or (isinstance(w, str) and w == "exp"):
            return w
        if isinstance(w, str):
            raise ValueError("ReconLoss: %s must be None, \"exp\" or a vector (got %r)" % (name, w))
        w = torch.as_tensor(w).detach().to("cpu", torch.float32)
        if w.dim() != 1 or w.numel() < 1 or not bool(torch.isfinite(w).all()):
            raise ValueError("ReconLoss: %s must be a finite 1-D vector (got shape %s)" % (name, tuple(w.shape)))
        return w.clone()

    @property
    def has_weights(self):
        return self.temporal_weight is not None or self.gdl_temporal_weight is not None

    @staticmethod
    def resolve(w, T, name="temporal_weight"):
        """the fp32 CPU vector of length T a weight specification stands for (None stays None); ValueError for another length"""
        if w is None:
            return None
        if isinstance(w, str):
            if T < 2:
                raise ValueError("ReconLoss: %s \"exp\" needs at least two time indices (got T = %d)" % (name, T))
            return temporal_weight_func(T).float()
        w = ReconLoss._spec(w, name)
        if w.numel() != T:
            raise ValueError("ReconLoss: %s has %d entries, the loss sees %d time indices" % (name, w.numel(), T))
        return w

    def total(self, l_mse, l_l1):
        """the point-wise part of the total"""
        return l_mse if self.point == "mse" else (l_l1 if self.point == "l1" else l_mse + l_l1)

    @classmethod
    def from_criteria(cls, point_criterion, gdl_criterion=None):
        """point_criterion: an `MSELoss`, an `L1Loss` or a pair of both (their temporal weights must then agree); gdl_criterion: a `GDL`
        (None: alpha 1, no weights).  ValueError when a `norm_dim` is set."""
        crits = list(point_criterion) if isinstance(point_criterion, (list, tuple)) else [point_criterion]
        kinds = []
        for c in crits:
            if not isinstance(c, (MSELoss, L1Loss)):
                raise ValueError("ReconLoss.from_criteria: %r is neither an MSELoss nor an L1Loss of vptr_amd.model.criterion" % (c,))
            if c.norm_dim is not None:
                raise ValueError("ReconLoss.from_criteria: norm_dim = %r is not available on the kernels" % (c.norm_dim,))
            kinds.append("mse" if isinstance(c, MSELoss) else "l1")
        if sorted(kinds) not in (["mse"], ["l1"], ["l1", "mse"]):
            raise ValueError("ReconLoss.from_criteria: expected one MSELoss, one L1Loss or one of each (got %s)" % kinds)
        w = crits[0].temporal_weight
        for c in crits[1:]:
            same = (w is None and c.temporal_weight is None) or (w is not None and c.temporal_weight is not None
                                                                 and torch.equal(torch.as_tensor(w).cpu(), torch.as_tensor(c.temporal_weight).cpu()))
            if not same:
                raise ValueError("ReconLoss.from_criteria: the MSELoss and the L1Loss carry different temporal weights; the kernels apply one")
        if gdl_criterion is not None and not isinstance(gdl_criterion, GDL):
            raise ValueError("ReconLoss.from_criteria: %r is no GDL of vptr_amd.model.criterion" % (gdl_criterion,))
        alpha = 1.0 if gdl_criterion is None else gdl_criterion.alpha
        wg = None if gdl_criterion is None else gdl_criterion.temporal_weight
        return cls("+".join(k for k in ("mse", "l1") if k in kinds), alpha, w, wg)

    def __repr__(self):
        def show(w):
            return w if w is None or isinstance(w, str) else "tensor[%d]" % w.numel()
        return "ReconLoss(point=%r, gdl_alpha=%g, temporal_weight=%s, gdl_temporal_weight=%s)" % (
            self.point, self.gdl_alpha, show(self.temporal_weight), show(self.gdl_temporal_weight))


class _ReconMixin:
    """what the trainers share of `recon=`: the device weight buffers (owned here, read by address by every launch, also from inside a
    captured graph) and the loss call"""
    recon = None
    _recon_w = None          # (w_point, w_gdl) device fp32 [T] or None each, built at the first step; _recon_T: their length

    def _init_recon(self, recon):
        if recon is not None and not isinstance(recon, ReconLoss):
            raise ValueError("recon must be a vptr_amd.train.ReconLoss or None (got %r)" % (recon,))
        self.recon, self._recon_w = recon, None

    def _recon_weights(self, T, device):
        if self._recon_w is None:
            r = self.recon
            wp, wg = ReconLoss.resolve(r.temporal_weight, T), ReconLoss.resolve(r.gdl_temporal_weight, T, "gdl_temporal_weight")
            self._recon_w = tuple(None if w is None else w.to(device) for w in (wp, wg))
            self._recon_T = T
        elif self._recon_T != T:
            raise ValueError("ReconLoss: the temporal weights were built for %d time indices, this step's loss sees %d" % (self._recon_T, T))
        return self._recon_w

    def _recon_losses(self, pred, target):
        """-> (l_mse, l_l1, l_gdl, the point-wise part of the total)"""
        wp, wg = self._recon_weights(pred.shape[1], pred.device) if self.recon.has_weights else (None, None)
        l_mse, l_l1, l_gdl = ops.recon_losses(pred, target, wp, wg, self.recon.gdl_alpha)
        return l_mse, l_l1, l_gdl, self.recon.total(l_mse, l_l1)

    def set_temporal_weight(self, w, gdl=None):
        """rewrite the temporal weights in place: w for the point-wise term, gdl for the GDL (None: w as well).  The copies are ordinary
        stream-ordered copies into the buffers the launches read by address, so a captured step uses the new values from its next replay
        on and its graph is untouched.  Only weights the trainer was constructed with can be rewritten (a launch without them holds NULL)."""
        if self.recon is None or not self.recon.has_weights:
            raise ValueError("set_temporal_weight: this trainer was constructed without temporal weights (recon=ReconLoss(temporal_weight=...))")
        gdl = w if gdl is None else gdl
        if self._recon_w is None:            # nothing launched yet: the configuration is all there is to change
            r = self.recon
            self.recon = ReconLoss(r.point, r.gdl_alpha, None if r.temporal_weight is None else w, None if r.gdl_temporal_weight is None else gdl)
            return
        if gdl is not w and self._recon_w[1] is None:
            raise ValueError("set_temporal_weight: this trainer's GDL was constructed without temporal weights")
        for buf, new, name in ((self._recon_w[0], w, "temporal_weight"), (self._recon_w[1], gdl, "gdl_temporal_weight")):
            if buf is not None:
                buf.copy_(ReconLoss.resolve(new, self._recon_T, name), non_blocking=False)


class _GanMixin:
    """How the trainers evaluate the adversarial loss: the torch `GANLoss` module (`gan_loss="torch"`, the default) or the fixed-order
    kernels of csrc/gan_loss.hip (`gan_loss="fused"`).  `self.gan`, the criterion module with labels 1 / 0, is built by the trainer in
    both settings; the fused calls take the same `gan_mode` and the same labels."""
    gan_fused = False

    def _init_gan_loss(self, gan_loss, gan_mode):
        if gan_loss not in ("torch", "fused"):
            raise ValueError("gan_loss must be 'torch' or 'fused', got %r" % (gan_loss,))
        if gan_loss == "fused" and gan_mode not in ops.GAN_MODES:
            raise ValueError("gan_loss='fused': gan_mode must be one of %s, got %r" % (sorted(ops.GAN_MODES), gan_mode))
        self.gan_loss, self.gan_mode, self.gan_fused = gan_loss, gan_mode, gan_loss == "fused"

    def _gan_pair(self, fake_logits, real_logits):
        """fused cal_lossD -> (l_fake, l_real, 0.5 * lam_gan * (l_fake + l_real)) in one forward call"""
        return ops.gan_loss_pair(fake_logits, real_logits, 0.5 * self.lam_gan, mode=self.gan_mode, real_label=1.0, fake_label=0.0)

    def _gan_term(self, logits):
        """the generator's adversarial term: the logits of generated frames against the real label"""
        if self.gan_fused:
            return ops.gan_loss(logits, True, mode=self.gan_mode, real_label=1.0, fake_label=0.0)
        return self.gan(logits, True)


class FlatAdamW:
    """torch.optim.AdamW semantics (lr, betas, eps, decoupled weight decay, bias correction) on one flat slab, with
    clip_grad_norm_ folded in.  Every parameter must receive a gradient each step (true for the VPTR transformers).

    schedule (an `optim.LRSchedule`) / skip_nonfinite: either one switches the device-resident controls on (optim.py, csrc/optim.hip).
    The hyper-parameters then live in a device record that `set_lr` / `set_weight_decay` / `set_max_grad_norm` / `set_schedule` (and an
    assignment to `.lr`) rewrite with stream-ordered writes, so they also reach the next replay of a captured step; the rate follows the
    schedule on the device; with skip_nonfinite a step whose gradient norm is NaN or Inf leaves the parameters, both moments and the step
    count bit for bit as they were and is counted (`skipped()`, `skipped_in_a_row()`).  With a constant schedule the trajectory is
    bit-identical to the uncontrolled optimizer's.  Without controls nothing changes: the same three launches, the same state_dict.

    accum_steps (a whole number k >= 1) / ema_decay (0 <= d < 1): either one switches the controls on as well and adds their `window`
    record (include/vptr_hip_accum.h, csrc/optim.hip).  Every `zero_grad()` + backward + `step()` is then one MICRO-step: `zero_grad`
    zeroes the gradient slab only when a window of k micro-steps starts, `step` issues the same launches every time, and the update
    happens in the call that closes the window, on the sum of the window's gradients times grad_scale / k; the calls before it (holds)
    leave parameters, moments, step count and schedule position bit for bit as they are.  `applied()` tells which kind a call was.
    With ema_decay an EMA of the parameters (`ema`, laid out like `flat`, seeded with the parameters) is updated inside the update
    kernel: ema += (1 - d_now) (p_new - ema), d_now = min(d, (1 + u) / (10 + u)) after u updates with ema_warmup, else d.  The default
    accum_steps=None is k = 1 without the window record.

    param_groups (a list of {"params": [...], "lr_scale": 1.0, "weight_decay": None}): switches the controls on as well and adds the
    group map and group tables (include/vptr_hip_groups.h, csrc/optim.hip): torch.optim.AdamW with several param_groups under one
    LambdaLR and one clip_grad_norm_ over all parameters.  Group g steps with base_lr * lr_scale_g * schedule factor and its own
    weight decay (None inherits the optimizer's and follows `set_weight_decay`); the clip norm, betas and eps stay global.  Parameters
    that no entry lists form group 0 with the defaults, the listed groups follow (optim.resolve_param_groups).  lr_scale 0 leaves a
    group's parameters bit for bit while its moments still move, as torch does with lr = 0; its gradient still counts in the clip norm.
    `set_group` rewrites a group between steps or replays, `group_lr(g)` is the rate it last used.  `step` then issues sumsq ->
    prepare -> group scalars -> grouped update -> plane refresh: one kernel node more than the controlled step.

    tensor_stats (a `diagnostics.TensorStats`), names (one string per trainable parameter in slab order; None: "param_<i>"): switches the
    controls on as well and adds per-tensor statistics on the device (diagnostics.py, csrc/tensor_stats.hip): `step` issues one call of
    two launches right behind the update -- so it sees the new p, m and v and this step's gradient, scaled by the record's grad_scale --
    and ahead of the plane refresh.  `opt.tensor_stats` (a `diagnostics.TensorStatsState`) holds the `[S + 1, 8]` table, `view`s of its
    words for `DeviceLossMeters`, `set_every` / `set_on_skip`, `report()` and `culprits()`.  Nothing of it enters `state_dict()`."""

    ctl = None   # optim.OptimControls when the controls are on
    ema = None   # the EMA slab (ema_decay=)
    groups = None   # optim.GroupTable (param_groups=)
    tensor_stats = None   # diagnostics.TensorStatsState (tensor_stats=)
    _windowed = False

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, channel_last=(), schedule=None,
                 skip_nonfinite=False, accum_steps=None, ema_decay=None, ema_warmup=True, param_groups=None, tensor_stats=None, names=None):
        """channel_last: ids of [C, ...] parameters that the kernels consume channel-last (the (C,H,W) LayerNorm affines and
        the depthwise 3x3 weights of MlpDWBN): they are STORED channel-last in the slab and exposed as a permuted view of
        their usual shape, so no per-step transposes of the parameter or its gradient remain (AdamW is elementwise, the
        order inside the slab is irrelevant; state_dict / load_state_dict go through strided copies)."""
        self.params = [p for p in params if p.requires_grad]
        if param_groups is not None:   # validated before any parameter is rebound to the slab
            self._group_of, group_specs = resolve_param_groups(self.params, param_groups)
        if tensor_stats is not None:   # validated before any parameter is rebound to the slab, too
            if not isinstance(tensor_stats, TensorStats):
                raise ValueError("tensor_stats must be a vptr_amd.diagnostics.TensorStats, got %r" % (tensor_stats,))
            from .diagnostics import check_names, plan
            plan([p.numel() for p in self.params])
            names = check_names(names, len(self.params))
        elif names is not None:
            raise ValueError("names= belongs to tensor_stats=")
        channel_last = set(channel_last)
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        pad = (-total) % 4
        self.flat = torch.zeros(total + pad, device=dev, dtype=torch.float32)
        self.grad = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        off = 0
        self._layout = []  # per parameter: (offset, numel, None | (channel-last storage shape, permutation back to the logical shape))
        with torch.no_grad():
            for p in self.params:
                n = p.numel()
                if id(p) in channel_last and p.dim() >= 2:
                    perm = list(range(1, p.dim())) + [0]                  # storage order: trailing dims, then channels
                    inv = [p.dim() - 1] + list(range(p.dim() - 1))
                    shape_cl = [p.shape[i] for i in perm]
                    val = p.detach().clone()
                    p.data = self.flat[off:off + n].view(shape_cl).permute(inv)
                    p.data.copy_(val)
                    p.grad = self.grad[off:off + n].view(shape_cl).permute(inv)
                    self._layout.append((off, n, (shape_cl, inv)))
                else:
                    self._layout.append((off, n, None))
                    self.flat[off:off + n].copy_(p.detach().reshape(-1))
                    p.data = self.flat[off:off + n].view(p.shape)
                    p.grad = self.grad[off:off + n].view(p.shape)
                off += n
        self.total = total
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.step_dev = torch.zeros(1, device=dev, dtype=torch.float32)
        self.sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        self._windowed = accum_steps is not None or ema_decay is not None
        if schedule is not None or skip_nonfinite or self._windowed or param_groups is not None or tensor_stats is not None:
            self.ctl = OptimControls(dev, lr, betas, eps, weight_decay, max_grad_norm, schedule, skip_nonfinite, accum_steps, ema_decay, ema_warmup)
        if param_groups is not None:
            self.groups = GroupTable(dev, group_map(self._layout, self._group_of, total + pad), group_specs, weight_decay)
        if tensor_stats is not None:
            ts = self.tensor_stats = TensorStatsState(dev, [n for _, n, _ in self._layout], names, tensor_stats)
            self._ts_scale = self.ctl.hyper[H_GRAD_SCALE:H_GRAD_SCALE + 1]
            if self.groups is not None:   # where `report` finds each tensor's rate: the group table's words, or the one of the state record
                ts.lr_dev, ts.lr_index = self.groups.gstate.view(-1, G_WORDS)[:, GS_LR], list(self._group_of)
            else:
                ts.lr_dev, ts.lr_index = self.ctl.state[S_LR_NOW:S_LR_NOW + 1], [0] * len(self.params)
        if ema_decay is not None:
            self.ema = self.flat.clone()
        if self._windowed:
            self.grad._vptr_accumulates = True   # ops.flush_wgrads: one adder per destination and launch in deterministic mode
        ops.register_flat_slab(self.flat, self.grad)  # backward kernels accumulate weight gradients in place
        # P16 planes of every nn.Linear-shaped weight of the slab (forward operand and transposed input-gradient operand), rebuilt
        # by one launch after each step: the GEMMs then stage weights by DMA instead of splitting fp32 per tile (ops.WeightPlanes)
        self.planes = None
        lin = ops.linear_weights_of(self.params) if ops.config.use_p16 else []
        if lin:
            self.planes = ops.WeightPlanes(lin)
            ops.register_weight_planes(self.planes)

    # -- hyper-parameters: plain attributes without controls; with them every change also goes into the device record ------------
    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        if self.ctl is not None:
            self.ctl.set_lr(value)
        self._lr = value

    def _need_ctl(self, what):
        if self.ctl is None:
            raise RuntimeError("FlatAdamW.%s needs the device-resident controls (schedule= or skip_nonfinite=True); without them the "
                               "hyper-parameters of a captured step are frozen" % what)
        return self.ctl

    def set_lr(self, lr):
        """the base rate the schedule multiplies; effective from the next step, eager or replayed"""
        self._need_ctl("set_lr")
        self.lr = lr

    def set_weight_decay(self, weight_decay):
        self._need_ctl("set_weight_decay").set_weight_decay(weight_decay)
        if self.groups is not None:
            self.groups.set_default_weight_decay(weight_decay)
        self.weight_decay = weight_decay

    def set_max_grad_norm(self, max_grad_norm):
        """None: no clipping"""
        self._need_ctl("set_max_grad_norm").set_max_grad_norm(max_grad_norm)
        self.max_grad_norm = max_grad_norm

    def set_schedule(self, schedule):
        """replace the schedule; it is evaluated at the step count the optimizer has reached, not restarted"""
        self._need_ctl("set_schedule").set_schedule(schedule)

    @property
    def schedule(self):
        return self.ctl.schedule if self.ctl is not None else None

    def lr_now(self):
        """the rate of the last applied step (0-dim fp32 device view, 0 before the first step)"""
        return self._need_ctl("lr_now").word(S_LR_NOW)

    def skipped(self):
        """steps skipped for a non-finite gradient norm so far (0-dim fp32 device view)"""
        return self._need_ctl("skipped").word(S_SKIPPED_TOTAL)

    def skipped_in_a_row(self):
        """... since the last applied step (0-dim fp32 device view): a run that no longer recovers shows here"""
        return self._need_ctl("skipped_in_a_row").word(S_SKIPPED_IN_A_ROW)

    # -- parameter groups ----------------------------------------------------------------------------------------------------------
    def _need_groups(self, what):
        if self.groups is None:
            raise RuntimeError("FlatAdamW.%s needs param_groups=" % what)
        return self.groups

    def set_group(self, g, lr_scale=None, weight_decay=None):
        """rewrite group g's rate scale and / or weight decay (None: as it is): stream-ordered writes of its record words, effective from
        the next step, eager or replayed.  A weight decay given here no longer follows `set_weight_decay`."""
        self._need_groups("set_group").set(g, lr_scale, weight_decay)

    def group_lr(self, g):
        """the rate group g used in the last applied step (0-dim fp32 device view, 0 before the first step)"""
        return self._need_groups("group_lr").lr(g)

    def group_params(self, g):
        """indices into `params` of group g's parameters, in slab order"""
        self._need_groups("group_params")._group(g)
        return [i for i, gi in enumerate(self._group_of) if gi == g]

    def _order(self):
        """parameter indices in the order torch.optim numbers them: group after group, slab order inside a group"""
        if self.groups is None:
            return list(range(len(self.params)))
        return [i for g in range(self.groups.ngroups) for i in self.group_params(g)]

    # -- accumulation window and EMA -------------------------------------------------------------------------------------------
    def _need_window(self, what):
        if not self._windowed:
            raise RuntimeError("FlatAdamW.%s needs accum_steps= or ema_decay=" % what)
        return self.ctl

    @property
    def accum_steps(self):
        return self.ctl.accum_steps if self._windowed else 1

    def set_accum_steps(self, k):
        """micro-steps per window from the next window on; raises inside a window (`reset_window()` drops it)"""
        self._need_window("set_accum_steps").set_accum_steps(k)

    def set_ema_decay(self, ema_decay):
        if self.ema is None or ema_decay is None:
            raise RuntimeError("FlatAdamW.set_ema_decay: the EMA slab exists only when the optimizer was built with ema_decay=, and stays then")
        self.ctl.set_ema_decay(ema_decay)

    def reset_window(self):
        """drop the micro-steps held in the open window (stream-ordered, reaches the next replay too): the next `zero_grad` zero-fills.
        A capture ends with the window wherever its warm-up steps left it; call this to start the first replay on a window boundary."""
        self._need_window("reset_window").reset_window()

    def applied(self):
        """1 if the last `step` call closed a window with an update, 0 for a hold or a skipped close (0-dim fp32 device view)"""
        return self._need_window("applied").wword(W_APPLY_NOW)

    def micro(self):
        """micro-steps held in the open window (0-dim fp32 device view; 0 after a close)"""
        return self._need_window("micro").wword(W_MICRO)

    def ema_param(self, i):
        """the EMA of parameter i in its logical shape (a view of the EMA slab)"""
        if self.ema is None:
            raise RuntimeError("FlatAdamW.ema_param needs ema_decay=")
        return self._logical(self.ema, i)

    def swap_ema(self):
        """exchange the parameter slab and the EMA slab in place (one launch) and rebuild the weight planes"""
        if self.ema is None:
            raise RuntimeError("FlatAdamW.swap_ema needs ema_decay=")
        check(lib.vptr_slab_swap(ptr(self.flat), ptr(self.ema), self.flat.numel(), stream()), "vptr_slab_swap")
        self._swapped = not self._swapped
        if self.planes is not None:
            self.planes.refresh()

    _swapped = False   # the parameter slab currently holds the EMA (inside NARTrainer.ema_weights)

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError("FlatAdamW.%s: the parameter slab holds the EMA weights (inside ema_weights()); leave the context first" % what)

    # -- torch.optim.AdamW-compatible state (checkpoints of the reference carry `optimizer_T.state_dict()`) ------------------
    def _logical(self, slab, i):
        """view of parameter i's range of `slab` (m, v, ...) in the parameter's LOGICAL shape: channel-last stored parameters
        come back through the same permuted view their .data uses, so state crosses the torch.optim format unscrambled"""
        off, n, cl = self._layout[i]
        if cl is None:
            return slab[off:off + n].view(self.params[i].shape)
        return slab[off:off + n].view(cl[0]).permute(cl[1])

    def state_dict(self):
        self._not_swapped("state_dict")
        state = {}
        step = self.step_dev.detach().clone().reshape(())
        for k, i in enumerate(self._order()):   # k: the id torch.optim gives the parameter (== i without groups)
            state[k] = {"step": step.clone(), "exp_avg": self._logical(self.m, i).contiguous().clone(),
                        "exp_avg_sq": self._logical(self.v, i).contiguous().clone()}
            if self.ema is not None:   # an unknown key of a parameter's state travels through torch.optim.AdamW.load_state_dict as well
                state[k]["ema"] = self._logical(self.ema, i).contiguous().clone()
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self.params)))}
        if self.ctl is not None:   # torch.optim.AdamW.load_state_dict carries an unknown key of a group along untouched
            total, in_a_row = self.ctl.counters()
            group[STATE_KEY] = {"schedule": self.ctl.schedule.to_dict(), "skip_nonfinite": self.ctl.skip_nonfinite,
                                "skipped_total": total, "skipped_in_a_row": in_a_row}
            if self._windowed:
                micro, ema_updates = self.ctl.window_counters()
                group[STATE_KEY].update(accum_steps=self.ctl.accum_steps, micro=micro, ema_decay=self.ctl.ema_decay, ema_warmup=self.ctl.ema_warmup,
                                        ema_updates=ema_updates)
        if self.groups is None:
            return {"state": state, "param_groups": [group]}
        out, first = [], 0
        for g in range(self.groups.ngroups):   # one entry per group; group 0 carries the controls
            cnt = len(self.group_params(g))
            entry = dict(group if g == 0 else {k: v for k, v in group.items() if k != STATE_KEY})
            entry.update(lr=self.lr * self.groups.lr_scale[g], weight_decay=self.groups.decay_of(g), params=list(range(first, first + cnt)))
            entry[SCALE_KEY] = self.groups.lr_scale[g]
            out.append(entry)
            first += cnt
        return {"state": state, "param_groups": out}

    def load_state_dict(self, sd):
        self._not_swapped("load_state_dict")
        groups = sd["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(self.params):
            raise ValueError("FlatAdamW.load_state_dict: %d parameters in the checkpoint, %d here" % (len(ids), len(self.params)))
        g0 = groups[0]
        order = list(range(len(self.params)))      # which parameter the k-th saved id belongs to
        if self.groups is None:
            if any(g["lr"] != g0["lr"] or g["weight_decay"] != g0["weight_decay"] for g in groups):
                raise ValueError("FlatAdamW.load_state_dict: the checkpoint's %d param_groups differ in lr or weight_decay; build the optimizer "
                                 "with the same param_groups=" % len(groups))
            lr, weight_decay = g0["lr"], g0["weight_decay"]
        elif len(groups) == 1:
            # an ungrouped checkpoint: base rate and default decay from it, this optimizer's own grouping, scales and group decays stay
            lr, weight_decay = g0["lr"], g0["weight_decay"]
        else:
            lr, weight_decay, scales, decays = self._read_groups(groups)
            order = self._order()
        self.lr, self.betas, self.eps = lr, tuple(g0["betas"]), g0["eps"]
        if self.ctl is None:
            self.weight_decay = weight_decay
        else:
            self.set_weight_decay(weight_decay)
        if self.groups is not None and len(groups) > 1:
            for g, (sc, wd) in enumerate(zip(scales, decays)):
                self.groups.set(g, sc, wd, inherit=wd is None)
        step = None
        with torch.no_grad():
            for pid, i in zip(ids, order):
                p = self.params[i]
                st = sd["state"].get(pid)
                if st is None:  # parameter never stepped
                    self._logical(self.m, i).zero_()
                    self._logical(self.v, i).zero_()
                else:
                    if tuple(st["exp_avg"].shape) != tuple(p.shape):
                        raise ValueError("FlatAdamW.load_state_dict: parameter %d has shape %s, its state %s"
                                         % (i, tuple(p.shape), tuple(st["exp_avg"].shape)))
                    self._logical(self.m, i).copy_(st["exp_avg"])
                    self._logical(self.v, i).copy_(st["exp_avg_sq"])
                    s_i = float(st["step"])
                    if step is not None and s_i != step:
                        raise ValueError("FlatAdamW.load_state_dict: per-parameter step counts differ (%g vs %g)" % (s_i, step))
                    step = s_i
            self.step_dev.fill_(0.0 if step is None else step)
        if self.ctl is not None:
            # a checkpoint of a controlled optimizer brings its schedule, skip flag and counters; one without the key (torch.optim.AdamW,
            # an uncontrolled FlatAdamW) leaves this optimizer's own controls in place
            saved = g0.get(STATE_KEY)
            if saved is not None:
                self.ctl.skip_nonfinite = bool(saved["skip_nonfinite"])
                self.ctl.schedule = LRSchedule.from_dict(saved["schedule"])
                self.ctl.load_counters(saved["skipped_total"], saved["skipped_in_a_row"])
            self.ctl.write(self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm, self._last_scale)
            if self._windowed:
                self._load_window(sd, ids, saved or {})
        ops.invalidate_weight_planes()   # a checkpoint load usually rewrites the parameters too (possibly through .data)

    def _read_groups(self, groups):
        """a dict with several param_groups against this optimizer's grouping -> (base lr, default weight decay, scale per group, weight
        decay per group or None for a group that keeps inheriting).  The scale is the `vptr_lr_scale` key, or lr_g / base without it
        (a torch.optim.AdamW dict), where base is what makes group 0's rate agree with the scale group 0 has here."""
        T = self.groups
        if len(groups) != T.ngroups or any(len(g["params"]) != len(self.group_params(j)) for j, g in enumerate(groups)):
            raise ValueError("FlatAdamW.load_state_dict: the checkpoint has param_groups of sizes %r, this optimizer %r"
                             % ([len(g["params"]) for g in groups], [len(self.group_params(j)) for j in range(T.ngroups)]))
        s0 = groups[0].get(SCALE_KEY, T.lr_scale[0])
        base = groups[0]["lr"] / s0 if s0 > 0 else self.lr
        scales = [g[SCALE_KEY] if SCALE_KEY in g else (g["lr"] / base if base > 0 else T.lr_scale[j]) for j, g in enumerate(groups)]
        inheriting = [j for j in range(T.ngroups) if T.weight_decay[j] is None]
        default = groups[inheriting[0]]["weight_decay"] if inheriting else self.weight_decay
        decays = [None if (j in inheriting and g["weight_decay"] == default) else g["weight_decay"] for j, g in enumerate(groups)]
        return base, default, scales, decays

    def _load_window(self, sd, ids, saved):
        """Loading always ends on a window boundary: a partial window's gradients are not part of a checkpoint, so resume is bit-exact
        at window boundaries only.  The EMA comes from the checkpoint; a dict without it (torch.optim.AdamW, an optimizer without
        ema_decay) seeds it again from the parameters as they are now -- load the model before the optimizer."""
        self.ctl.load_window(0.0)
        if "accum_steps" in saved:
            self.ctl.set_accum_steps(int(saved["accum_steps"]))
            if self.ema is not None and saved.get("ema_decay") is not None:
                self.ctl.set_ema_decay(saved["ema_decay"], bool(saved["ema_warmup"]))
        if saved.get("micro"):
            import warnings
            warnings.warn("FlatAdamW.load_state_dict: the checkpoint was saved inside an accumulation window; the %d micro-batch(es) it held "
                          "are dropped and the next step starts a window" % int(saved["micro"]))
        if self.ema is None:
            return
        with torch.no_grad():
            if all(sd["state"].get(pid) is not None and "ema" in sd["state"][pid] for pid in ids):
                order = self._order() if (self.groups is not None and len(sd["param_groups"]) > 1) else range(len(ids))
                for i, pid in zip(order, ids):
                    self._logical(self.ema, i).copy_(sd["state"][pid]["ema"])
                self.ctl.load_window(saved.get("ema_updates", 0.0))
            else:
                self.ema.copy_(self.flat)

    def close(self):
        """drop this optimizer's process-wide registrations (gradient-slab lookup, weight planes); also runs when it is collected"""
        if getattr(self, "flat", None) is not None:
            ops.unregister_flat_slab(self.flat)
        self.planes = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: interpreter shutdown
            pass

    def zero_grad(self):
        p0 = self.params[0]
        if p0.grad is None or p0.grad.data_ptr() != self.grad.data_ptr():
            raise RuntimeError("FlatAdamW: a parameter lost its flat gradient view (do not use set_to_none=True)")
        ops.discard_wgrads()  # leftovers of a backward pass that raised must not leak into this step
        if self._windowed:
            self.ctl.begin(self.grad)   # zero-fills when a window starts, keeps the partial sum otherwise: one kernel node either way
        else:
            self.grad.zero_()

    def grad_norm(self):
        """global L2 norm of the (scaled) gradients of the last step (device tensor), as clip_grad_norm_ returns"""
        if self.ctl is not None:
            return self.ctl.word(S_GRAD_NORM)
        return self.sumsq.sqrt() * self._last_scale

    _last_scale = 1.0
    _sumsq_ws = None

    def step(self, grad_scale=1.0):
        """grad_scale multiplies every gradient before clipping (e.g. 1 / accumulation steps; with accum_steps=k the 1 / k is applied
        here, on top of grad_scale).  With accum_steps / ema_decay every call issues sumsq -> prepare -> update -> plane refresh; a hold
        behaves as a skipped step does: the update kernel returns at once and the planes are rebuilt from unchanged weights."""
        self._not_swapped("step")
        n = self.flat.numel()
        self._last_scale = float(grad_scale)
        if ops.config.deterministic:   # fixed-order two-pass sum (no atomics): the clip coefficient is reproducible bit for bit
            if self._sumsq_ws is None:
                self._sumsq_ws = torch.empty(1024, device=self.flat.device, dtype=torch.float32)
            check(lib.vptr_sumsq_ws(ptr(self.grad), n, ptr(self.sumsq), ptr(self._sumsq_ws), self._sumsq_ws.numel(), stream()), "vptr_sumsq_ws")
        else:
            self.sumsq.zero_()
            check(lib.vptr_sumsq(ptr(self.grad), n, ptr(self.sumsq), stream()), "vptr_sumsq")
        if self.ctl is not None:
            # sumsq -> prepare (skip decision, step count, schedule, update scalars: one lane) -> the update reading them -> plane refresh.
            # A skipped step still refreshes the planes: they are rebuilt from unchanged weights.
            self.ctl.set_grad_scale(grad_scale / self.accum_steps)
            self.ctl.prepare(self.step_dev, self.sumsq)
            if self.groups is not None:
                self.groups.scalars(self.ctl.state)
        else:
            self.step_dev.add_(1.0)
        prof = ops.profiling.opt
        if prof is not None:   # bench.py's HBM roofline pass: HIP events on the launch stream around the optimizer's streaming kernels
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        if self.ctl is not None:
            self.ctl.update(self.flat, self.grad, self.m, self.v, n, self.ema, self.groups)
        else:
            check(lib.vptr_adamw(ptr(self.flat), ptr(self.grad), ptr(self.m), ptr(self.v), n, self.lr, self.betas[0], self.betas[1],
                                 self.eps, self.weight_decay, ptr(self.step_dev),
                                 ptr(self.sumsq) if self.max_grad_norm is not None else None,
                                 float(self.max_grad_norm or 0.0), float(grad_scale), stream()), "vptr_adamw")
        if prof is not None:
            ev[1].record()
        if self.tensor_stats is not None:   # behind the update (the new p, m, v; this step's gradient), ahead of the plane refresh
            self.tensor_stats.launch(self.flat, self.grad, self.m, self.v, self._ts_scale, self.ctl.state)
        if self.planes is not None:
            self.planes.refresh()
        if prof is not None:
            ev[2].record()
            prof.append((n, self.planes.wp.numel() if self.planes is not None else 0, ev))


def _channel_last_ids(transformer):
    """parameters of the conv-FFNs that the HIP kernels read channel-last: LayerNorm((C,H,W)) affines and depthwise 3x3 weights"""
    from .model.vidhrformer import MlpDWBN
    ids = []
    for m in transformer.modules():
        if isinstance(m, MlpDWBN):
            ids.append(id(m.dw3x3.weight))
            if m.layer_norm:
                for norm in (m.norm1, m.norm2, m.norm3):
                    ids += [id(norm.weight), id(norm.bias)]
    return ids


class NARTrainer(_ReconMixin, _GanMixin):
    """One stage-2 NAR training step; see module docstring.  `enc`/`dec` are frozen (eval), `transformer` trains."""

    def __init__(self, enc, dec, transformer, batch_size, lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, process_group=None,
                 bucket_mb=64, dec_weight_grads=True, disc=None, lam_gan=None, gan_mode="vanilla", schedule=None, skip_nonfinite=False,
                 accum_steps=None, ema_decay=None, ema_warmup=True, recon=None, gan_loss="torch", param_groups=None, tensor_stats=None):
        """tensor_stats: a `diagnostics.TensorStats` -- per-tensor gradient, weight and update statistics of the transformer's `FlatAdamW`
        on the device, named as `transformer.named_parameters()` names them (`trainer.opt.tensor_stats`: table, `view`, `set_every`,
        `report`, `culprits`).  It switches the device-resident controls on; a captured step gains two kernel nodes.  Data parallel: the
        call runs behind the exchange, every rank computes the same table and no collective is added.  The discriminator's optimizer
        (`disc=`) has none.

        param_groups: the parameter groups of the transformer's `FlatAdamW` (per-group lr_scale and weight_decay): a list of
        {"params": [...], "lr_scale": 1.0, "weight_decay": None}, or a callable that takes the transformer and returns one, e.g.
        `optim.no_decay_groups`.  It switches the device-resident controls on; `trainer.opt.set_group(g, ...)` between steps or replays
        changes the next update, `trainer.opt.group_lr(g)` can go into `DeviceLossMeters`.  The discriminator's optimizer (`disc=`) stays
        ungrouped.

        recon: a `ReconLoss` -- the frame loss then runs on `ops.recon_losses` (L1, a GDL exponent, temporal weights of length Tf), the
        returned terms gain "T_L1", and `set_temporal_weight` rewrites the weights between steps or replays.  None: `ops.mse_gdl` as ever.

        gan_loss: "torch" (the `GANLoss` module: ATen expand, BCE, mean and their autograd) or "fused" (`ops.gan_loss_pair` for the
        discriminator update with coef = 0.5 * lam_gan, `ops.gan_loss` for the generator term: csrc/gan_loss.hip, fixed-order kernels in
        the `gan_mode` given).  The returned keys are the same; without a discriminator the setting is only validated.

        accum_steps / ema_decay / ema_warmup: gradient accumulation and EMA weights of `FlatAdamW`.  Every `step()` call is then one
        micro-step and also returns "applied" (1 when the call closed a window with an update); `trainer.opt.reset_window()` drops an
        open window, e.g. after `capture`, which ends wherever its warm-up steps left the window.  Data parallel: the calls that hold
        flush their weight gradients without any all-reduce, the closing call exchanges the summed slab as before.  `ema_weights()`,
        `eval_step(..., weights="ema")`, `predict(..., weights="ema")` and `ema_state_dict()` use the EMA.  Not with the adversarial
        branch (`disc=`): its discriminator steps inside the forward pass.

        schedule / skip_nonfinite: the device-resident optimizer controls of `FlatAdamW` (optim.py), given to the transformer's optimizer
        and, with the adversarial branch, to the discriminator's alike.  `step` then also returns "lr" and "skipped" (and "skipped_D"), and
        `capture`, `capture_front`, `verify_graph` work as before: `trainer.opt.set_lr(...)` between replays changes the next update.  A
        skipped step leaves parameters, moments and step count untouched; it still refreshes the weight planes (from unchanged weights),
        still advances the dropout seed, and BatchNorm running statistics of the forward pass it belongs to have been updated already."""
        self._init_stage2(enc, dec, transformer, lr, max_grad_norm, process_group, bucket_mb, dec_weight_grads, disc, lam_gan, gan_mode,
                          schedule, skip_nonfinite, accum_steps, ema_decay, ema_warmup, gan_loss, param_groups, tensor_stats)
        self._init_recon(recon)
        # loss_name_list MSE / GDL(alpha=1) / BiPatchNCE(N, Tf, 8, 8, temperature 1.0) of train_NAR.py:176-179 run as the fused kernels of
        # csrc/losses.hip (ops.mse_gdl, ops.nce_loss): plain kernel launches only, so the step can live in a hipGraph
        self.nce_temperature = 1.0
        self.lam_pc = lam_pc
        if self.world > 1:
            from .parallel import BufferSync
            self._bufsync = BufferSync(self.T, 0, process_group)   # DDP's per-forward broadcast of rank 0's BatchNorm statistics

    def _init_stage2(self, enc, dec, transformer, lr, max_grad_norm, process_group, bucket_mb, dec_weight_grads, disc, lam_gan, gan_mode,
                     schedule, skip_nonfinite, accum_steps=None, ema_decay=None, ema_warmup=True, gan_loss="torch", param_groups=None, tensor_stats=None):
        """what both stage-2 recipes construct: frozen auto-encoder, optional adversarial branch, the transformer's flat-slab optimizer"""
        if disc is not None and (ema_decay is not None or (accum_steps is not None and accum_steps != 1)):
            raise ValueError("accum_steps > 1 / ema_decay are not available with the adversarial branch (disc=): the discriminator's "
                             "update runs inside every forward pass and has no accumulation window")
        self.enc, self.dec, self.T = enc.eval(), dec.eval(), transformer
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.bucket_elems = bucket_mb * (1 << 20) // 4
        self._init_gan(disc, lam_gan, lr, gan_mode, schedule, skip_nonfinite, gan_loss)
        # Stage 2 optimises the transformer only (train_NAR.py:205).  The reference nevertheless leaves the decoder's
        # parameters trainable (train_NAR.py:190-191, train_FAR.py:181-182), so its backward computes decoder weight gradients nobody
        # consumes; that work is reproduced by default (dec_weight_grads=True) so that the measured step does everything the reference's does.
        for p in enc.parameters():
            p.requires_grad_(False)  # the encoder runs under no_grad (:54-56)
        for p in dec.parameters():
            p.requires_grad_(bool(dec_weight_grads))
        self.dec_weight_grads = bool(dec_weight_grads)
        for mod in list(self.enc.modules()) + list(self.dec.modules()):
            mod._vptr_frozen = True  # never stepped here: packed conv weights / eval-BN folds are cached (ops.frozen_weights)
        self.opt = FlatAdamW(self.T.parameters(), lr=lr, max_grad_norm=max_grad_norm, channel_last=_channel_last_ids(self.T),
                             schedule=schedule, skip_nonfinite=skip_nonfinite, accum_steps=accum_steps,
                             ema_decay=ema_decay, ema_warmup=ema_warmup,
                             param_groups=param_groups(self.T) if callable(param_groups) else param_groups, tensor_stats=tensor_stats,
                             names=None if tensor_stats is None else [n for n, p in self.T.named_parameters() if p.requires_grad])
        self._bufsync = None
        self._graph = None

    _front = None          # data-parallel front graph (capture_front)
    _front_items = ()

    # -- optional adversarial branch (train_NAR.py:22-30,37-41,66-79; train_FAR.py:22-45,66-80): off in the reference scripts ----
    def _init_gan(self, disc, lam_gan, lr, gan_mode, schedule=None, skip_nonfinite=False, gan_loss="torch"):
        self.disc, self.lam_gan = disc, lam_gan
        self._init_gan_loss(gan_loss, gan_mode)
        if disc is None:
            return
        if lam_gan is None:
            raise ValueError("a discriminator needs lam_gan (train_NAR.py:67)")
        for p in disc.parameters():
            p.requires_grad_(True)
        self.opt_D = FlatAdamW(list(disc.parameters()), lr=lr, betas=(0.5, 0.999), weight_decay=0.0, schedule=schedule,
                               skip_nonfinite=skip_nonfinite)  # Adam, :204
        self.gan = GANLoss(gan_mode, target_real_label=1.0, target_fake_label=0.0).to(self.opt_D.flat.device)

    def _disc_update(self, fake, real):
        """cal_lossD + optimizer_D.step(), then freeze the discriminator for the generator pass"""
        if not self.disc.training:
            self.disc.train()
        for p in self.disc.parameters():
            p.requires_grad_(True)
        self.opt_D.zero_grad()
        if self.gan_fused:
            l_fake, l_real, loss_D = self._gan_pair(self.disc(fake.detach().flatten(0, 1)), self.disc(real.flatten(0, 1)))
        else:
            l_fake = self.gan(self.disc(fake.detach().flatten(0, 1)), False)
            l_real = self.gan(self.disc(real.flatten(0, 1)), True)
            loss_D = (l_fake + l_real) * 0.5 * self.lam_gan
        loss_D.backward()
        if self.pg is not None and self.world > 1:   # the reference's DDP-wrapped discriminator averages its gradients too
            ops.flush_wgrads()
            from .parallel import allreduce_mean_
            allreduce_mean_(self.opt_D.grad, self.pg, self.bucket_elems)
        self.opt_D.step()
        for p in self.disc.parameters():
            p.requires_grad_(False)
        out = {"Dtotal": loss_D.detach(), "Dfake": l_fake.detach(), "Dreal": l_real.detach()}
        if self.opt_D.ctl is not None:
            out["skipped_D"] = self.opt_D.skipped()
        return out

    # -- data-parallel gradient exchange: a few large RCCL all-reduces on the flat gradient slab ---------------------
    _grad_scale = 1.0   # factor the next optimizer step applies to the gradient slab (1 / world after a summed exchange)

    comm_stats = None   # set to a dict by bench.py: per-step exchange accounting (bytes, calls, device-side exposed time, host wait time)

    def _comm_begin(self):
        st = self.comm_stats
        if st is None:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()      # on the launch stream, behind the last kernel that produces gradients
        return (e0, time.perf_counter())

    def _comm_end(self, tok, nbytes, calls):
        """e0 -> e1 on the launch stream brackets nothing but the wait for the collectives: the time the stream idles there is the
        communication the step could not hide behind compute (0 when every all-reduce finished under the weight-gradient chunks)"""
        if tok is None:
            return
        st = self.comm_stats
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        st.setdefault("events", []).append((tok[0], e1))
        st["wait_host_s"] = st.get("wait_host_s", 0.0) + time.perf_counter() - tok[1]
        st["bytes"] = st.get("bytes", 0) + int(nbytes)
        st["calls"] = st.get("calls", 0) + int(calls)
        st["steps"] = st.get("steps", 0) + 1

    def _exchanges(self):
        """whether the step's gradients cross the process group.  VPTR_DP_FORCE_EXCHANGE=1: take the exchange path on a one-rank group
        too (a one-GPU box can then drive c10d's RCCL backend -- its own stream, async Work objects, event ordering against the
        weight-gradient launches -- through the same code the 8-GPU job runs: tests/test_22_rccl_gpu.py, bench.py --force-exchange)"""
        return self.pg is not None and (self.world > 1 or os.environ.get("VPTR_DP_FORCE_EXCHANGE") == "1")

    @staticmethod
    def _overlaps():
        """whether the all-reduces are issued between the weight-gradient chunks (VPTR_DP_OVERLAP=0: one plain exchange after them)"""
        return os.environ.get("VPTR_DP_OVERLAP", "1") != "0"

    def _holds_next(self):
        """whether the next optimizer call leaves its accumulation window open (the host's mirror of the window position: it is
        deterministic, because neither a hold nor a skipped close moves a window boundary)"""
        return self.opt._windowed and not self.opt.ctl.closes_next()

    def _allreduce_grads(self):
        if not self._exchanges():
            return
        from .parallel import allreduce_sum_
        tok = self._comm_begin()
        allreduce_sum_(self.opt.grad, self.pg, self.bucket_elems)
        self._comm_end(tok, self.opt.grad.numel() * 4, -(-self.opt.grad.numel() // self.bucket_elems))
        self._grad_scale = 1.0 / self.world

    def _backward_and_exchange(self, loss):
        """loss.backward(), the grouped weight-gradient GEMMs and the data-parallel gradient exchange.  With more than one
        rank the weight gradients are flushed in DP_CHUNKS grouped launches ordered by slab address; as soon as a chunk has
        been enqueued, the slab range below the next chunk's first destination is final and its all-reduce is issued
        asynchronously (RCCL runs it on its own stream), overlapping the next chunk's GEMM."""
        self._grad_scale = 1.0
        if self._exchanges() and self._holds_next():
            # a micro-step that leaves its window open: the slab is a partial sum no other rank needs yet.  The weight gradients are
            # flushed in one grouped launch and nothing crosses the process group; the closing call exchanges the window's sum
            loss.backward()
            ops.flush_wgrads()
            self._grad_scale = 1.0 / self.world
            return
        if not (self._exchanges() and self._overlaps()):
            loss.backward()
            ops.flush_wgrads()  # no-op: the grouped weight-gradient launch already ran at the end of backward
            self._allreduce_grads()
            return
        with ops.hold_wgrads():
            loss.backward()
        self._exchange_held_wgrads()

    def _exchange_held_wgrads(self):
        """the recorded weight gradients as DP_CHUNKS grouped launches with the slab ranges they complete sent out in between (see
        `_backward_and_exchange`); also the eager tail of a front-graph step (`capture_front`)"""
        grad = self.opt.grad
        base, n = grad.data_ptr(), grad.numel()
        works, sent = [], [0]
        # bench.py's tuning table (comm_stats["timeline"] = True): HIP events on the launch stream at the start of the exchange, behind every
        # weight-gradient chunk (= the moment its all-reduces may start: c10d orders them behind this point of the stream) and behind every
        # Work.wait() (= the moment that all-reduce had finished, or the stream reached the wait -- whichever is later)
        tl = None
        if self.comm_stats is not None and self.comm_stats.get("timeline"):
            tl = {"t0": torch.cuda.Event(enable_timing=True), "chunk_end": [], "sent_bytes": [], "ar_done": [], "ar_bytes": []}
            tl["t0"].record()

        def send_upto(next_ptr):
            hi = n if next_ptr is None else max(sent[0], min(n, (next_ptr - base) // 4))
            off = sent[0]
            if tl is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                tl["chunk_end"].append(e)
                tl["sent_bytes"].append((hi - off) * 4)
            while off < hi:  # sub-ranges of at most bucket_elems, like the non-overlapped path
                end = min(hi, off + self.bucket_elems)
                works.append(torch.distributed.all_reduce(grad[off:end], op=torch.distributed.ReduceOp.SUM, group=self.pg,
                                                          async_op=True))
                if tl is not None:
                    tl["ar_bytes"].append((end - off) * 4)
                off = end
            sent[0] = hi

        ops.flush_wgrads(chunks=DP_CHUNKS, on_chunk=send_upto)
        if sent[0] < n:
            send_upto(None)
        tok = self._comm_begin()
        for w in works:
            w.wait()
            if tl is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                tl["ar_done"].append(e)
        if tl is not None:
            self.comm_stats["last_timeline"] = tl     # of the most recent step; bench.py resolves the events after its final synchronize
        self._comm_end(tok, n * 4, len(works))
        self._grad_scale = 1.0 / self.world   # the mean over ranks is folded into the optimizer kernel (FlatAdamW.step(grad_scale)): no extra pass over the slab

    def losses(self, pred_frames, future, pred_feats, future_feats):
        """cal_lossT (train_NAR.py:32-47, 81-91): MSE + GDL on the frames, lam_pc * BiPatchNCE on the L2-normalised NCE projections"""
        nce = self._nce_operands(pred_feats, future_feats)
        l_mse, l_gdl = ops.mse_gdl(pred_frames, future)
        l_pc = ops.nce_loss(*nce, self.nce_temperature)
        return l_gdl + l_mse + self.lam_pc * l_pc, l_gdl, l_mse, l_pc

    def _nce_operands(self, pred_feats, future_feats):
        """-> the (g, p, frames, L) of ops.nce_loss: the NCE projections of the future and the predicted features, token-major"""
        a = self.T.NCE_projector(pred_feats.permute(0, 1, 3, 4, 2))      # (N, T, h, w, C): token-major memory
        b = self.T.NCE_projector(future_feats.permute(0, 1, 3, 4, 2))
        N, T, h, w, C = a.shape
        return b.reshape(-1, C), a.reshape(-1, C), N * T, h * w

    # -- the stage-2 iteration, sequenced once for train and eval; a recipe contributes `_encode` and `_loss_terms` ----------------------
    def _encode(self, past, future):
        """-> (what the transformer is fed, what `_loss_terms` needs of the encoder besides)"""
        # train_NAR.py:54-56 encodes past and future in two calls; the encoder is per-frame (eval-mode BN), so one call on
        # the concatenated clip gives the same features with twice the rows per conv GEMM (480 instead of 240 tiles)
        if past.shape[0] == future.shape[0] and past.shape[2:] == future.shape[2:]:
            feats = self.enc(torch.cat([past, future], dim=1))
            return feats[:, :past.shape[1]], feats[:, past.shape[1]:]
        return self.enc(past), self.enc(future)

    def _loss_terms(self, pred_frames, pred_feats, past, future, future_feats):
        """-> (the recipe's part of the loss, its terms by name)"""
        if self.recon is None:
            loss, l_gdl, l_mse, l_pc = self.losses(pred_frames, future, pred_feats, future_feats)
            return loss, {"T_GDL": l_gdl, "T_MSE": l_mse, "T_bpc": l_pc}
        nce = self._nce_operands(pred_feats, future_feats)               # the launch order of `losses`: projections, frame loss, NCE
        l_mse, l_l1, l_gdl, l_point = self._recon_losses(pred_frames, future)
        l_pc = ops.nce_loss(*nce, self.nce_temperature)
        return l_gdl + l_point + self.lam_pc * l_pc, {"T_GDL": l_gdl, "T_MSE": l_mse, "T_bpc": l_pc, "T_L1": l_l1}

    def _forward(self, past, future, train, front=False):
        """-> (loss, terms): encoder, transformer, decoder, discriminator terms, recipe loss terms, generator's adversarial term"""
        with torch.no_grad():
            feats, aux = self._encode(past, future)
        if train:
            if not self.T.training:   # nn.Module.train() walks ~500 sub-modules: ~5 ms of host time per step
                self.T.train()
            self.opt.zero_grad()
            if self.dec_weight_grads:
                self.dec.zero_grad(set_to_none=True)  # train_NAR.py:61
            if self._bufsync and not front:      # a collective: the front-graph step issues it eagerly before the replay
                self._bufsync.sync()
        pred_feats = self.T(feats)
        pred_frames = self.dec(pred_feats)
        extra = {}
        if self.disc is not None:                # cal_lossD(VPTR_Disc, pred_frames, future_frames): train_NAR.py:73,96, train_FAR.py:72,93
            extra = self._disc_update(pred_frames, future) if train else self._eval_disc(pred_frames, future)
        loss, terms = self._loss_terms(pred_frames, pred_feats, past, future, aux)
        if self.disc is not None:
            extra["T_gan"] = self._gan_term(self.disc(pred_frames.flatten(0, 1)))
            loss = loss + self.lam_gan * extra["T_gan"]
        return loss, dict({"T_total": loss}, **terms, **extra)

    def _step_impl(self, past, future, front=False):
        loss, terms = self._forward(past, future, True, front)
        return self._finish(loss, {k: v.detach() for k, v in terms.items()}, front)

    def step(self, past, future, meters=None):
        """one train step (a replay when `capture` / `capture_front` ran); meters: a `meters.DeviceLossMeters` that receives the returned
        terms in one launch issued behind the step -- outside any captured graph, so the meter can be swapped per epoch"""
        self.opt._not_swapped("step (NARTrainer.step)")
        out = self._step(past, future)
        if meters is not None:
            meters.update(out)
        return out

    def _replay(self, g, static_past, static_future, past, future, bufsync=False):
        """fill a captured graph's static inputs and replay it.  Replays are stream-ordered like any other launch;
        tests/test_20_graph_gpu.py compares them with eager steps (the round-1 corruption was a captured table upload reading a
        recycled pinned buffer: ops._to_device_async)"""
        if self.opt.planes is not None and self.opt.planes.stale():
            self.opt.planes.refresh()   # parameters were changed from outside (load_state_dict) since the last replay
        _copy_into(static_past, past)
        _copy_into(static_future, future)
        if bufsync and self._bufsync:
            self._bufsync.sync()
        g.replay()

    def _step(self, past, future):
        if self._front is not None:
            # data-parallel step: forward + backward replayed as one hipGraph, then the part that talks to other ranks runs eagerly --
            # DP_CHUNKS grouped weight-gradient launches on the recorded operands (static addresses in the graph's pool), the all-reduces
            # between them, the optimizer (3 launches)
            self._replay(self._front, self._static_past, self._static_future, past, future, bufsync=True)
            ops.requeue_wgrads(self._front_items)
            self._grad_scale = 1.0
            if self._exchanges() and self._holds_next():   # an open window: flush, no all-reduce (see `_backward_and_exchange`)
                ops.flush_wgrads()
                self._grad_scale = 1.0 / self.world
            elif self._overlaps():
                self._exchange_held_wgrads()
            else:
                ops.flush_wgrads()
                self._allreduce_grads()
            self.opt.step(grad_scale=self._grad_scale)
            self._static_out["grad_norm"] = self.opt.grad_norm()
            if self.opt.ctl is not None:
                self._static_out["lr"], self._static_out["skipped"] = self.opt.lr_now(), self.opt.skipped()
            if self.opt._windowed:
                self._static_out["applied"] = self.opt.applied()
            return self._static_out
        if self._graph is not None:
            self._replay(self._graph, self._static_past, self._static_future, past, future)
            if self.opt._windowed:
                self.opt.ctl.advance_mirror()   # the replay ran one captured prepare launch
            return self._static_out
        return self._step_impl(past, future)

    def _module_scratch(self):
        """The frozen auto-encoder keeps shape-keyed scratch on its modules (plane, head and Winograd buffers) and replaces it when a
        forward of another shape runs; a captured graph reads and writes the buffers of its capture by address, so it holds on to them --
        otherwise an eager pass at another batch size (the fall-back of `eval_step`, `predict`) would hand their memory to the next
        allocation and the following replay would write into it."""
        return [getattr(m, a) for mod in (self.enc, self.dec) for m in mod.modules() for a in ("_plane_bufs", "_head_bufs", "_wino_bufs")
                if getattr(m, a, None) is not None]

    @staticmethod
    def _warm_up_for_capture(warmup, step, any_rank=None, tune=True):
        """eager steps in front of a capture: `warmup` - 1 of them, then as many more as the tile-row tuning of the grouped weight-gradient
        launches still wants (ops.wgrad_tune_open: each setting is timed ops._TUNE_SAMPLES times, the first, cold sample not counted), then
        the geometry is FIXED (ops.wgrad_tune_settle) and one last step issues exactly the launches -- and table uploads, counted in
        ops._upload_stats -- the capture will issue.  Whether a timing has been booked depends on how far this host runs ahead of its
        GPU, so with several ranks (`any_rank`: True if the flag holds on any rank) every rank takes the same number of extra steps: each
        of them issues the step's all-reduces, and a rank that stopped early would pair its next collective with another rank's step.
        tune=False (a validation pass, which launches no weight gradients): the tuning is neither waited for nor settled -- settling
        would fix the geometry for a later train capture."""
        for _ in range(max(warmup, 1) - 1):
            step()
        if tune:
            extra = 0
            while extra < 2 * ops._TUNE_SAMPLES and (any_rank(ops.wgrad_tune_open()) if any_rank else ops.wgrad_tune_open()):
                step()
                extra += 1
            ops.wgrad_tune_settle()
        ops._upload_stats.update(count=0, max_bytes=0)
        step()

    def _capture(self, past, future, warmup, eager, body, what, census, tune=True, any_rank=None, beside_collectives=False):
        """The capture procedure of `capture`, `capture_front` and `capture_eval` -> (graph, what `body` returned, static past, static
        future, scratch to keep alive).  `past`/`future` give the static shapes; `eager(past, future)` is one warm-up pass on a side
        stream, `body(past, future)` what is captured; `census` names the attribute that receives the node census and `what` the
        captured thing in the error text; `tune`, `any_rank`: see `_warm_up_for_capture`.

        The captured graph is inspected before it is instantiated: it must consist of kernel, memcpy and empty nodes only.  A MEMSET
        node (hipMemsetAsync under capture -- ATen's multi-block reductions zero their semaphores that way) writes garbage from
        the second replay on with this HIP runtime (tools/memset_node_probe.py), which is what corrupted the round-2 graph
        (F.normalize's backward in the BiPatchNCE branch); the step's own losses are plain kernels now (csrc/losses.hip) and
        any memset node that sneaks back in raises here instead of silently training on garbage."""
        past, future = past.clone(), future.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._warm_up_for_capture(warmup, lambda: eager(past, future), any_rank, tune)
        torch.cuda.current_stream().wait_stream(s)
        # the captured pass uploads as many host-built tables as the last warm-up pass did (grouped launches: 2 per group, more with
        # the GAN branch or non-P16 groups); each gets a pinned buffer of its own that lives as long as the graph
        ops.reserve_graph_staging(count=ops._upload_stats["count"] + 4, nbytes=max(1 << 16, 2 * ops._upload_stats["max_bytes"]))
        if tune:
            ops.wgrad_tune_settle()
        if beside_collectives:
            # c10d's RCCL watchdog thread polls the events of earlier collectives (hipEventQuery): under the default GLOBAL capture mode
            # that call, made while THIS thread captures, aborts the process ("operation not permitted when stream is capturing").  Drain
            # the device first (no work left to poll) and capture in thread-local mode (other threads' calls stay legal).
            torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, capture_error_mode="thread_local" if beside_collectives else "global"):
            out = body(past, future)
        nodes = graph_node_census(g)
        setattr(self, census, nodes)
        bad = {k: v for k, v in nodes.items() if k not in ("kernel", "memcpy", "empty")}
        if bad:
            g.reset()
            raise RuntimeError("captured %s holds node types that are not replay-safe on this HIP runtime: %s (all nodes: %s)" % (what, bad, nodes))
        g.instantiate()
        return g, out, past, future, self._module_scratch()

    def capture(self, past, future, warmup=3):
        """Capture the whole step (forward, losses, backward, clip, AdamW) into one hipGraph.  `past`/`future` give the
        static shapes; real data is copied into the captured input buffers by `step`.

        The procedure, and the node census it refuses a graph on, is `_capture`'s."""
        if self.pg is not None and self.world > 1:
            raise RuntimeError("graph capture of the data-parallel step is not enabled (RCCL calls stay eager)")
        g, self._static_out, self._static_past, self._static_future, self._graph_scratch = self._capture(
            past, future, warmup, self._step_impl, self._step_impl, "step", "graph_nodes")
        self._graph = g
        return g

    def capture_front(self, past, future, warmup=3):
        """Data-parallel twin of `capture`: everything of the step that involves no other rank -- encoder, forward, losses, backward
        with the weight gradients only RECORDED (ops.hold_wgrads), the LayerNorm parameter-gradient reductions -- becomes one hipGraph;
        `step` replays it and then runs the exchange eagerly (grouped weight-gradient chunks, RCCL all-reduces, optimizer): ~1000
        launches per step leave the host's critical path, no collective is ever captured.  The recorded weight-gradient operands live
        in the graph's private pool, so their addresses are the same at every replay."""
        if self.disc is not None:
            raise RuntimeError("capture_front: the adversarial branch all-reduces inside the step; run it eagerly")
        if self.pg is None:
            raise RuntimeError("capture_front is the data-parallel capture; use capture() without a process group")
        g, (self._static_out, self._front_items), self._static_past, self._static_future, self._graph_scratch = self._capture(
            past, future, warmup, self._step_impl, lambda p, f: (self._front_impl(p, f), ops.take_wgrads()),
            "step", "graph_nodes", any_rank=self._any_rank, beside_collectives=True)
        self._front = g
        return g

    def _any_rank(self, flag):
        """`flag` or-reduced over the process group (MAX all-reduce of one element on the launch stream)"""
        if self.pg is None or self.world == 1:
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0], device=self.opt.flat.device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=self.pg)
        return t.item() > 0.5

    def _front_impl(self, past, future):
        """`_step_impl` up to the end of the backward pass: weight gradients recorded but not launched, no collective, no optimizer"""
        return self._step_impl(past, future, front=True)

    def _finish(self, loss, terms, front):
        """backward + exchange + optimizer (the whole step), or -- front=True, under capture_front -- backward only, with the weight
        gradients held for the eager tail"""
        if front:
            with ops.hold_wgrads():
                loss.backward()
            ops.flush_partial_reduces()
            return terms
        self._backward_and_exchange(loss)
        self.opt.step(grad_scale=self._grad_scale)
        terms["grad_norm"] = self.opt.grad_norm()
        if self.opt.ctl is not None:
            terms["lr"], terms["skipped"] = self.opt.lr_now(), self.opt.skipped()
        if self.opt._windowed:
            terms["applied"] = self.opt.applied()
        return terms

    # -- EMA weights ------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """Run what is inside on the EMA weights: the parameter slab and the EMA slab are exchanged in place (one launch) and the weight
        planes rebuilt, and exchanged back on exit, also when the body raises.  A captured eval graph reads the slab by address, so
        `eval_step` replays work unchanged.  `step()` and the optimizer's `state_dict()` raise inside."""
        self.opt.swap_ema()
        try:
            yield self
        finally:
            self.opt.swap_ema()

    def ema_state_dict(self):
        """the transformer's `state_dict()` with the EMA in place of every trained parameter; buffers are copied as they are (BatchNorm
        running statistics are not averaged)"""
        if self.opt.ema is None:
            raise RuntimeError("ema_state_dict needs ema_decay=")
        index = {id(p): i for i, p in enumerate(self.opt.params)}
        sd = {k: v.detach().clone() for k, v in self.T.state_dict().items()}
        with torch.no_grad():
            for name, p in self.T.named_parameters():
                if id(p) in index and name in sd:
                    sd[name] = self.opt.ema_param(index[id(p)]).contiguous().clone()
        return sd

    def _weights(self, weights):
        if weights not in ("raw", "ema"):
            raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
        return self.ema_weights() if weights == "ema" else contextlib.nullcontext()

    # -- validation pass: the train_flag=False branch of single_iter (train_NAR.py:88-100, train_FAR.py:85-94) ------------------------
    _eval_graph = None

    def _eval_disc(self, fake, real):
        """cal_lossD, forward only (eval-mode discriminator): both clips flattened to frames, whatever their lengths"""
        if self.gan_fused:
            l_fake, l_real, l_D = self._gan_pair(self.disc(fake.flatten(0, 1)), self.disc(real.flatten(0, 1)))
            return {"Dtotal": l_D, "Dfake": l_fake, "Dreal": l_real}
        l_fake = self.gan(self.disc(fake.flatten(0, 1)), False)
        l_real = self.gan(self.disc(real.flatten(0, 1)), True)
        return {"Dtotal": (l_fake + l_real) * 0.5 * self.lam_gan, "Dfake": l_fake, "Dreal": l_real}

    def _eval_forward(self, past, future):
        return self._forward(past, future, False)[1]

    @torch.no_grad()
    def _eval_impl(self, past, future):
        """Forward and losses with the transformer (and discriminator) in eval mode.  Nothing a train step owns is written: no optimizer
        state, no gradient, no BatchNorm statistic (eval mode), no collective; the dropout master seed, which every transformer forward
        advances, is put back, and so is the seed scope a pending backward would read."""
        if self.T.training:
            self.T.eval()
        if self.disc is not None and self.disc.training:
            self.disc.eval()
        dev = past.device
        key, seed = ops._dev_key(dev), ops._master_seed(dev)
        scope, saved = ops._seed_scope.get(key), seed.clone()
        try:
            return self._eval_forward(past, future)
        finally:
            seed.copy_(saved)
            if scope is None:
                ops._seed_scope.pop(key, None)
            else:
                ops._seed_scope[key] = scope

    def eval_step(self, past, future, meters=None, weights="raw"):
        """One validation iteration: the terms of `step` minus grad_norm, as 0-dim device tensors.  After `capture_eval` a batch of the
        captured shapes is a replay of the eval graph; any other batch runs eagerly.  The next `step` puts the modules back into train
        mode.  meters: as in `step`.  weights="ema": this one call inside `ema_weights()`; the returned terms are then copies (a
        replay's static outputs would be overwritten by the next one)."""
        if weights != "raw":
            with self._weights(weights):
                out = {k: v.clone() for k, v in self.eval_step(past, future).items()}
            if meters is not None:
                meters.update(out)
            return out
        g = self._eval_graph
        if g is not None and past.shape == self._eval_past.shape and future.shape == self._eval_future.shape:
            self._replay(g, self._eval_past, self._eval_future, past, future)
            out = self._eval_out
        else:
            out = self._eval_impl(past, future)
        if meters is not None:
            meters.update(out)
        return out

    def capture_eval(self, past, future, warmup=2):
        """`capture` for the validation pass (the same procedure, `_capture`).  An eval pass launches no weight gradients, so their
        tile-row tuning is neither waited for nor settled.  The eval graph has static inputs and outputs of its own, so it coexists with
        a train graph; it holds no collective, so it is allowed under a multi-rank group."""
        g, self._eval_out, self._eval_past, self._eval_future, self._eval_scratch = self._capture(
            past, future, warmup, self._eval_impl, self._eval_impl, "validation pass", "eval_graph_nodes", tune=False)
        self._eval_graph = g
        return g

    def has_graph(self, train=True):
        """whether `step` (train) / `eval_step` replays a captured graph"""
        return (self._graph is not None or self._front is not None) if train else self._eval_graph is not None

    def static_inputs(self, train=True):
        """the (past, future) buffers the train (`capture` / `capture_front`) or eval (`capture_eval`) graph reads.  `step` / `eval_step`
        skip their copy when handed exactly these tensors: write a batch there once -- `ClipIngest(...)(raw, out=trainer.static_inputs())`"""
        if not self.has_graph(train):
            raise RuntimeError("static_inputs: capture() / capture_front() first" if train else "static_inputs(train=False): capture_eval() first")
        return (self._static_past, self._static_future) if train else (self._eval_past, self._eval_future)

    # -- replay == eager, checked on the live model (bench.py runs this before it times a graph) -------------------------------------
    @staticmethod
    def _slab_state(opt, module):
        """copies of what a step writes of one optimizer and the module it steps: slabs, step count, controls record, module buffers"""
        s = {"flat": opt.flat.clone(), "m": opt.m.clone(), "v": opt.v.clone(), "step": opt.step_dev.clone(),
             "buffers": [b.detach().clone() for b in module.buffers()]}
        if opt.ctl is not None:   # the controls' device-written record: last rate, skip counters, the update scalars
            s["ctl"] = opt.ctl.state.clone()
        if opt._windowed:         # inside a window the gradient slab is state too; the window record and the host's mirror of its position
            s["grad"], s["window"], s["micro_host"] = opt.grad.clone(), opt.ctl.window.clone(), opt.ctl.micro_host
        if opt.ema is not None:
            s["ema"] = opt.ema.clone()
        return s

    @staticmethod
    def _load_slab_state(opt, module, s):
        opt.flat.copy_(s["flat"]); opt.m.copy_(s["m"]); opt.v.copy_(s["v"]); opt.step_dev.copy_(s["step"])
        for b, v in zip(module.buffers(), s["buffers"]):
            b.copy_(v)
        if "ctl" in s:
            opt.ctl.state.copy_(s["ctl"])
        if "window" in s:
            opt.grad.copy_(s["grad"]); opt.ctl.window[8:].copy_(s["window"][8:])   # the device's half; the host's words follow the setters
            opt.ctl.micro_host = s["micro_host"]
        if "ema" in s:
            opt.ema.copy_(s["ema"])

    def _snapshot(self):
        snap = self._slab_state(self.opt, self.T)
        snap["seed"] = ops._master_seed(self.opt.flat.device).clone()
        if self.disc is not None:   # the adversarial branch steps a second slab and the discriminator's BatchNorm statistics
            snap["D"] = self._slab_state(self.opt_D, self.disc)
        return snap

    def _restore(self, snap):
        dev = self.opt.flat.device
        with torch.no_grad():
            self._load_slab_state(self.opt, self.T, snap)
            ops._master_seed(dev).copy_(snap["seed"])
            if self.disc is not None:
                self._load_slab_state(self.opt_D, self.disc, snap["D"])
                if self.opt_D.planes is not None:
                    self.opt_D.planes.refresh()
        ops._seed_scope.pop(ops._dev_key(dev), None)
        if self.opt.planes is not None:
            self.opt.planes.refresh()

    @staticmethod
    def _term_diff(a, b):
        return abs(a - b) / (abs(a) + 1e-6) if (b == b and abs(b) < 1e30) else float("inf")

    def verify_graph(self, past, future, steps=3, rtol=2e-3, traj_rtol=5e-2, param_rtol=3e-4):
        """Replay == eager, checked on the live model; the state is restored afterwards.  -> (ok, report)

        Two comparisons, because a train step is a noise amplifier (the order of fp32 atomics perturbs a
        gradient by ~1e-7, the first AdamW updates are ~lr * sign(g), and a random-filled model turns the resulting sign flips into
        1e-4 ... 1e-3 differences of the NEXT step's gradient norm):
          * lock-step (bound `rtol` per term, `param_rtol` on the post-step parameters): replay i and eager step i both start from
            the SAME state -- the state the previous replay left (parameters, Adam moments, step count, BatchNorm statistics, dropout
            seed; the discriminator's too on the GAN branch).  Differences are those of ONE forward / backward / update from identical
            inputs with identical masks, nothing accumulates, and replay i is still the i-th consecutive replay of the graph (the
            round-2 corruption began at the second replay).
          * trajectory (`traj_rtol`, loose, plus finiteness): `steps` back-to-back replays with no host read in between vs `steps`
            eager steps from the same initial state."""
        if not self.has_graph():
            raise RuntimeError("verify_graph: capture() / capture_front() first")
        snap0 = self._snapshot()
        kind = "_graph" if self._graph is not None else "_front"
        g = getattr(self, kind)
        worst, where, prel = 0.0, None, 0.0
        lock = []
        try:
            for i in range(steps):
                pre = self._snapshot()
                setattr(self, kind, g)
                rg = {k: float(v) for k, v in self.step(past, future).items()}
                post_g = self._snapshot()
                self._restore(pre)
                setattr(self, kind, None)
                re_ = {k: float(v) for k, v in self.step(past, future).items()}
                pe, pg = self.opt.flat.double(), post_g["flat"].double()
                prel = max(prel, float((pe - pg).norm() / pe.norm()))
                for k in re_:
                    d = self._term_diff(re_[k], rg[k])
                    if d > worst:
                        worst, where = d, (i, k, re_[k], rg[k])
                lock.append((re_, rg))
                self._restore(post_g)          # the chain follows the graph: replay i + 1 sees what replay i left
            runs = {}
            for mode in ("eager", "graph"):
                self._restore(snap0)
                setattr(self, kind, g if mode == "graph" else None)
                outs = [self.step(past, future) for _ in range(steps)]           # no host read between the steps
                torch.cuda.synchronize()
                runs[mode] = [{k: float(v) for k, v in o.items()} for o in (outs if mode == "eager" else outs[-1:])]
            tworst, twhere = 0.0, None
            for k, a in runs["eager"][-1].items():
                d = self._term_diff(a, runs["graph"][-1][k])
                if d > tworst:
                    tworst, twhere = d, (steps - 1, k, a, runs["graph"][-1][k])
        finally:
            setattr(self, kind, g)
            self._restore(snap0)
        ok = worst <= rtol and prel <= param_rtol and tworst <= traj_rtol
        return ok, {"steps": steps, "worst_term_rel_diff": worst, "worst_term": where, "param_rel_l2": prel,
                    "trajectory_worst_rel_diff": tworst, "trajectory_worst": twhere,
                    "eager_last": runs["eager"][-1], "graph_last": runs["graph"][-1]}

    @torch.no_grad()
    def predict(self, past, weights="raw"):
        """Inference: Enc -> NAR -> Dec (Test_VPTR.ipynb cell 5, one NAR round).  weights="ema": inside `ema_weights()`."""
        self.T.eval()
        with self._weights(weights):
            return self.dec(self.T(self.enc(past)))


class FARTrainer(NARTrainer):
    """One FAR training step without the GAN branch (`single_iter` of train_FAR.py:48-101 with VPTR_Disc = None, the
    script's default :186-192): Enc(cat(past, future[:, :-1])) under no_grad, VPTRFormerFAR (causal temporal attention as a
    kernel flag), Dec, MSE + GDL against cat(past[:, 1:], future), backward, clip_grad_norm_(max_norm), AdamW.  Shares the
    flat-slab optimizer, grouped weight gradients and data-parallel exchange with `NARTrainer`."""

    def __init__(self, enc, dec, transformer, lr=1e-4, max_grad_norm=1.0, process_group=None, bucket_mb=64, dec_weight_grads=True,
                 disc=None, lam_gan=None, gan_mode="vanilla", schedule=None, skip_nonfinite=False, accum_steps=None, ema_decay=None,
                 ema_warmup=True, recon=None, gan_loss="torch", param_groups=None, tensor_stats=None):
        """schedule / skip_nonfinite / accum_steps / ema_decay / ema_warmup / recon / gan_loss / param_groups / tensor_stats: as in `NARTrainer`; the temporal
        weights of a `ReconLoss` have Tp - 1 + Tf entries here, one per frame of cat(past[:, 1:], future)"""
        # no BufferSync: the FAR transformer has no BatchNorm (LayerNorm conv-FFNs), nothing to broadcast per forward
        self._init_stage2(enc, dec, transformer, lr, max_grad_norm, process_group, bucket_mb, dec_weight_grads, disc, lam_gan, gan_mode,
                          schedule, skip_nonfinite, accum_steps, ema_decay, ema_warmup, gan_loss, param_groups, tensor_stats)
        self._init_recon(recon)

    def _encode(self, past, future):
        return self.enc(torch.cat([past, future[:, :-1]], dim=1)), None    # train_FAR.py:53-55

    def _loss_terms(self, pred_frames, pred_feats, past, future, aux):
        real = torch.cat([past[:, 1:], future], dim=1)                       # :80
        if self.recon is None:
            l_mse, l_gdl = ops.mse_gdl(pred_frames, real)                    # cal_lossT :32-46
            return l_gdl + l_mse, {"T_GDL": l_gdl, "T_MSE": l_mse}
        l_mse, l_l1, l_gdl, l_point = self._recon_losses(pred_frames, real)
        return l_gdl + l_point, {"T_GDL": l_gdl, "T_MSE": l_mse, "T_L1": l_l1}

    @torch.no_grad()
    def predict(self, past, num_pred, kv_cache=False, weights="raw", graph=False, mode="train"):
        """Autoregressive test-phase rollout (train_FAR.py:103-125): see vptr_amd.inference.far_rollout (kv_cache: its KV-cached path;
        mode: its 'train' / 'RIP' / 'RIL').  weights="ema": inside `ema_weights()`.
        graph=True (with kv_cache=True, else ValueError): the cached steps replay one captured hipGraph; the trainer keeps one
        `CachedDecoder` per (batch size, mode), captured at its first use.  The graph reads the parameter slab by address, so it follows
        `step()` and the EMA swap."""
        from .inference import CachedDecoder, far_rollout
        if graph and not kv_cache:
            raise ValueError("far_rollout: graph=True replays the KV-cached step; it needs kv_cache=True")
        with self._weights(weights):
            if graph:
                self.T.eval()
                key = (int(past.shape[0]), mode)
                decoders = self.__dict__.setdefault("_decoders", {})
                if key not in decoders:
                    decoders[key] = CachedDecoder(self.enc, self.dec, self.T, key[0], mode)
                graph = decoders[key]
            return far_rollout(self.enc, self.dec, self.T, past, num_pred, mode=mode, kv_cache=kv_cache, graph=graph)

    rollout = predict


class AETrainer(_ReconMixin, _GanMixin):
    """One stage-1 step (`single_iter` of train_AutoEncoder.py:44-78): rec = Dec(Enc(cat(past, future))) with train-mode
    BatchNorm; discriminator update on (rec.detach(), x): 0.5 * lam_gan * (BCE(D(fake), 0) + BCE(D(real), 1)), Adam; generator
    update: lam_gan * BCE(D(rec), 1) + MSE + GDL, Adam on Enc + Dec.  torch.optim.Adam(lr 2e-4, betas (0.5, 0.999)) is
    AdamW with weight_decay 0, so both optimizers are `FlatAdamW` slabs (no clipping in this stage)."""

    def __init__(self, enc, dec, disc, lr=2e-4, lam_gan=0.01, betas=(0.5, 0.999), gan_mode="vanilla", schedule=None, skip_nonfinite=False,
                 accum_steps=None, ema_decay=None, recon=None, gan_loss="torch", param_groups=None, tensor_stats=None):
        """recon: a `ReconLoss` with `point` and `gdl_alpha` only (the stage-1 loss has no time axis to weight: temporal weights raise
        ValueError); `step` and `eval_step` then also return "AE_L1".

        param_groups: not available here (ValueError): stage 1 is plain Adam without weight decay on both optimizers.
        tensor_stats: not available here either (ValueError): the statistics belong to the stage-2 trainers' transformer optimizer.

        gan_loss: "torch" or "fused", as in `NARTrainer`: the discriminator update's two losses and 0.5 * lam_gan * (their sum) in one
        `ops.gan_loss_pair`, the generator's term in one `ops.gan_loss`.

        schedule / skip_nonfinite: the device-resident optimizer controls of `FlatAdamW` (optim.py) for both optimizers; `step` then
        also returns "lr_G", "lr_D", "skipped_G", "skipped_D".  The two decisions are independent: a non-finite discriminator gradient
        skips the discriminator's update only.  A skipped step still advances the dropout seed and the BatchNorm running statistics of
        Enc, Dec and the discriminator, which the forward passes have written before the gradient exists: a non-finite INPUT therefore
        still reaches the running statistics (train-mode steps do not read them; an `eval_step` does)."""
        if ema_decay is not None or (accum_steps is not None and accum_steps != 1):
            raise ValueError("accum_steps > 1 / ema_decay are not available for the stage-1 step: its two optimizers alternate inside "
                             "one iteration and have no accumulation window")
        if param_groups is not None:
            raise ValueError("param_groups are not available for the stage-1 step (Adam without weight decay on Enc + Dec and on the "
                             "discriminator); they belong to the stage-2 trainers' transformer optimizer")
        if tensor_stats is not None:
            raise ValueError("tensor_stats are not available for the stage-1 step (two optimizers that alternate inside one iteration); "
                             "they belong to the stage-2 trainers' transformer optimizer")
        self._init_recon(recon)
        self._init_gan_loss(gan_loss, gan_mode)
        if recon is not None and recon.has_weights:
            raise ValueError("AETrainer: temporal weights are not available for the stage-1 loss (ReconLoss point and gdl_alpha only)")
        self.enc, self.dec, self.disc = enc, dec, disc
        for m in (enc, dec, disc):
            for p in m.parameters():
                p.requires_grad_(True)
        self.opt_G = FlatAdamW(list(enc.parameters()) + list(dec.parameters()), lr=lr, betas=betas, weight_decay=0.0, schedule=schedule,
                               skip_nonfinite=skip_nonfinite)
        self.opt_D = FlatAdamW(list(disc.parameters()), lr=lr, betas=betas, weight_decay=0.0, schedule=schedule, skip_nonfinite=skip_nonfinite)
        self.gan = GANLoss(gan_mode, target_real_label=1.0, target_fake_label=0.0).to(self.opt_G.flat.device)
        self.lam_gan = lam_gan

    def has_graph(self, train=True):
        """the stage-1 step is not captured"""
        return False

    def _ae_recon(self, rec, x):
        """-> (l_mse, l_gdl, the point-wise part of the total, further terms by name)"""
        if self.recon is None:
            l_mse, l_gdl = ops.mse_gdl(rec, x)
            return l_mse, l_gdl, l_mse, {}
        l_mse, l_l1, l_gdl, l_point = self._recon_losses(rec, x)
        return l_mse, l_gdl, l_point, {"AE_L1": l_l1}

    def step(self, past, future, meters=None):
        out = self._step(past, future)
        if meters is not None:
            meters.update(out)
        return out

    @torch.no_grad()
    def eval_step(self, past, future, meters=None):
        """the train_flag=False branch of single_iter (train_AutoEncoder.py:75-82): Enc, Dec and the discriminator in eval mode,
        cal_lossD and cal_lossG forward only; returns the keys of `step`.  Enc and Dec live in this trainer's optimizer slab, so
        their eval-mode forward keeps no packed weight or BatchNorm fold (ops.weights_cacheable): the pass reads the parameters and
        running statistics the last `step` left."""
        for m in (self.enc, self.dec, self.disc):
            if m.training:
                m.eval()
        x = torch.cat([past, future], dim=1)
        rec = self.dec(self.enc(x))
        if self.gan_fused:
            l_fake, l_real, l_D = self._gan_pair(self.disc(rec.flatten(0, 1)), self.disc(x.flatten(0, 1)))
        else:
            l_fake = self.gan(self.disc(rec.flatten(0, 1)), False)
            l_real = self.gan(self.disc(x.flatten(0, 1)), True)
            l_D = None
        l_gan = self._gan_term(self.disc(rec.flatten(0, 1)))
        l_mse, l_gdl, l_point, extra = self._ae_recon(rec, x)
        out = {"AEgan": l_gan, "AE_MSE": l_mse, "AE_GDL": l_gdl, "AE_total": self.lam_gan * l_gan + l_point + l_gdl,
               "Dtotal": (l_fake + l_real) * 0.5 * self.lam_gan if l_D is None else l_D, "Dfake": l_fake, "Dreal": l_real}
        out.update(extra)
        if meters is not None:
            meters.update(out)
        return out

    def _step(self, past, future):
        x = torch.cat([past, future], dim=1)
        if not self.enc.training:
            self.enc.train()
        if not self.dec.training:
            self.dec.train()
        self.opt_G.zero_grad()
        rec = self.dec(self.enc(x))
        # ---- discriminator (cal_lossD, :20-29)
        if not self.disc.training:
            self.disc.train()
        for p in self.disc.parameters():
            p.requires_grad_(True)
        self.opt_D.zero_grad()
        if self.gan_fused:
            l_fake, l_real, loss_D = self._gan_pair(self.disc(rec.detach().flatten(0, 1)), self.disc(x.flatten(0, 1)))
        else:
            l_fake = self.gan(self.disc(rec.detach().flatten(0, 1)), False)
            l_real = self.gan(self.disc(x.flatten(0, 1)), True)
            loss_D = (l_fake + l_real) * 0.5 * self.lam_gan
        loss_D.backward()
        self.opt_D.step()
        # ---- generator (cal_lossG, :31-42)
        for p in self.disc.parameters():
            p.requires_grad_(False)
        l_gan = self._gan_term(self.disc(rec.flatten(0, 1)))
        l_mse, l_gdl, l_point, extra = self._ae_recon(rec, x)
        loss_G = self.lam_gan * l_gan + l_point + l_gdl
        loss_G.backward()
        self.opt_G.step()
        out = {"AEgan": l_gan.detach(), "AE_MSE": l_mse.detach(), "AE_GDL": l_gdl.detach(), "AE_total": loss_G.detach(),
               "Dtotal": loss_D.detach(), "Dfake": l_fake.detach(), "Dreal": l_real.detach()}
        out.update({k: v.detach() for k, v in extra.items()})
        if self.opt_G.ctl is not None:
            out.update(lr_G=self.opt_G.lr_now(), lr_D=self.opt_D.lr_now(), skipped_G=self.opt_G.skipped(), skipped_D=self.opt_D.skipped())
        return out


def run_epoch(trainer, loader, train, meters, ingest=None):
    """One epoch of the reference's loop (train_NAR.py:231-247): `step` (train) or `eval_step` over `loader` with every returned term
    folded into `meters` on the device; nothing is read back, the caller's `meters.compute()` / `epoch_update()` is the epoch's one
    sync.  ingest: a `data.ClipIngest`; the loader then yields uint8 clip batches, written as fp32 straight into the graph's static
    inputs when the trainer has captured one for this mode and the batch fits it."""
    fn = trainer.step if train else trainer.eval_step
    static = None
    if ingest is not None and trainer.has_graph(train):
        static = trainer.static_inputs(train=train)
    for sample in loader:
        if ingest is None:
            past, future = sample
        elif static is not None and sample.shape[0] == static[0].shape[0]:
            past, future = ingest(sample, out=static)
        else:
            past, future = ingest(sample)
        fn(past, future, meters=meters)
    return meters


def script_style_nar_iter(enc, dec, transformer, optimizer, past, future, mse_loss, gdl_loss, bpnce, lam_pc=0.1, max_grad_norm=1.0):
    """One stage-2 iteration the way the reference's OWN script drives the `model` package (train_NAR.py:49-107 without the GAN
    branch): module calls, `zero_grad(set_to_none=True)`, the criterion classes + F.normalize, `loss.backward()`,
    `nn.utils.clip_grad_norm_`, a stock `torch.optim` optimizer -- no NARTrainer, no flat slab, no fused losses.  This is what
    "train_NAR.py drops in unchanged" executes on this package; tests/test_04_dropin_gpu.py pins it against the reference's step
    records and bench.py times it beside the NARTrainer step (`other_configs.drop_in_single_iter`)."""
    with torch.no_grad():
        past_feats = enc(past)
        future_feats = enc(future)
    transformer = transformer.train()
    transformer.zero_grad(set_to_none=True)
    dec.zero_grad(set_to_none=True)
    pred_feats = transformer(past_feats)
    pred_frames = dec(pred_feats)
    pf = transformer.NCE_projector(pred_feats.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
    gf = transformer.NCE_projector(future_feats.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
    l_mse = mse_loss(pred_frames, future)
    l_gdl = gdl_loss(future, pred_frames)
    l_pc = bpnce(F.normalize(gf, p=2.0, dim=2), F.normalize(pf, p=2.0, dim=2))
    loss = l_gdl + l_mse + lam_pc * l_pc
    loss.backward()
    gn = torch.nn.utils.clip_grad_norm_(transformer.parameters(), max_norm=max_grad_norm, norm_type=2)
    optimizer.step()
    return {"T_total": loss.detach(), "T_GDL": l_gdl.detach(), "T_MSE": l_mse.detach(), "T_bpc": l_pc.detach(), "grad_norm": gn.detach()}
