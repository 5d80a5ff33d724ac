"""Case runner of tests/test_09e_optim_ctl_gpu.py: the device-resident optimizer controls called through the C ABI
(include/vptr_hip_optim.h) -- vptr_optim_prepare (skip decision, step count, schedule, update scalars) and vptr_adamw_ctl (vptr_adamw with
its scalars read from the state record).

The runner talks to a BACKEND as tests/step_tail_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's
order without the trailing stream (tensors for pointers, None for NULL) and returns the return code; `last_error()` is the library's message.
`OptimEmu` below is an fp32 CPU emulation of the two entry points (and of vptr_adamw with the same element update, so that the bit-identity
cases mean something on the CPU) written from the header; tests/test_optim_ctl_cpu.py runs every case against it and against four named
mutations of it, each of which must fail the cases listed in `MUTATIONS`.

Every record and slab is a `Rec` / `Guard`: the payload inside a NaN-filled allocation with 16 guard floats (64 bytes, so a record stays
64-byte aligned) on both sides, which must come back bit for bit; the reserved words of `state` carry a bit pattern that must survive.

Bars.  lr_now: 2^-23 relative to base_lr * LRSchedule.factor(k) (one rounding of an fp64 product whose cos may differ from the host's in its
last bit).  Update scalars: 4 ulp (4 * 2^-23 relative) of an fp32 numpy evaluation of adamw_kernel's expressions; grad_norm 1 ulp.  The
bias corrections against fp64: through the update they produce, at test_09d's bar (step_tail_cases.adamw_bars: five times the distance an
fp32 evaluation of the same formulas keeps to fp64) -- the record stores lr / bc1 and rsqrt(bc2), not bc1 and bc2; their derived values are
printed.  The trajectory: adamw_bars' rule on the whole trajectory.  Everything else is bit for bit."""
import functools
import math

import numpy as np
import torch

from helpers import adamw_f32_emulation, f32, rel
from step_tail_cases import (ADAMW_BAR_FACTOR, ADAMW_BETAS, ADAMW_BIG, ADAMW_STEPS, HYPER, Guard, adamw_bars, adamw_inputs, bits, clip_coef_f32, record,
                             rn, same_bits, scalar, shifted)
from vptr_amd.optim import LRSchedule

F = np.float32
ULP = 2.0 ** -23
WORDS = 16
# word indices of include/vptr_hip_optim.h (tests/test_optim_ctl_cpu.py compares them with the header's #defines)
H = dict(BASE_LR=0, BETA1=1, BETA2=2, EPS=3, WEIGHT_DECAY=4, MAX_NORM=5, GRAD_SCALE=6, SKIP_NONFINITE=7, SCHED_KIND=8, WARMUP_STEPS=9, TOTAL_STEPS=10,
         MIN_RATIO=11)
S = dict(LR_NOW=0, GRAD_NORM=1, SKIP_NOW=2, SKIPPED_TOTAL=3, SKIPPED_IN_A_ROW=4, COEF=5, STEP_SIZE=6, INV_SQRT_BC2=7, DECAY=8, OB1=9, OB2=10, BETA1=11,
         BETA2=12, EPS=13)
SCALARS = ("COEF", "STEP_SIZE", "INV_SQRT_BC2", "DECAY", "OB1", "OB2", "BETA1", "BETA2", "EPS")
RESERVED = (14, 15)
RESERVED_BITS = (0x7FC12345, 0x0BADF00D)          # a NaN with a payload and an ordinary pattern
KINDS = ("constant", "linear", "cosine")
BASE_LR = 1e-3


def hyper_words(lr=BASE_LR, b1=HYPER["b1"], b2=HYPER["b2"], eps=HYPER["eps"], wd=HYPER["wd"], max_norm=None, grad_scale=1.0, skip=0, sched=None):
    """the 16 words the host writes (reserved words NaN: the kernel must not read them into anything)"""
    sched = sched or LRSchedule()
    w = torch.full((WORDS,), float("nan"))
    w[:12] = torch.tensor([lr, b1, b2, eps, wd, 0.0 if max_norm is None else max_norm, grad_scale, float(skip),
                           float(KINDS.index(sched.kind)), float(sched.warmup_steps), float(sched.total_steps), sched.min_ratio], dtype=torch.float64).float()
    return w


def fresh_state():
    w = torch.zeros(WORDS)
    w.view(torch.int32)[list(RESERVED)] = torch.tensor([b - (1 << 32) if b >> 31 else b for b in RESERVED_BITS], dtype=torch.int64).int()
    return w


class Rec(Guard):
    """a 16-word record inside its guards; the guards are compared bit for bit"""

    def __init__(self, dev, start, shift=0):
        super().__init__(WORDS, dev, start=start, shift=shift)
        assert shift or self.out.data_ptr() % 64 == 0
        self.guard_bits = bits(self.buf).clone()

    def words(self):
        """guards bit-identical; the payload on the CPU"""
        now = bits(self.buf)
        assert torch.equal(now[:self.lo], self.guard_bits[:self.lo]) and torch.equal(now[self.lo + self.n:], self.guard_bits[self.lo + self.n:]), "write outside a record"
        return self.out.cpu().clone()


def _ulps(got, want):
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return 0.0 if math.isnan(want) and math.isnan(got) else float("inf")
    if math.isinf(want) or want == 0.0:
        return 0.0 if got == want else float("inf")
    return abs(got - want) / (abs(want) * ULP)


# --------------------------------------------------------------------------------------------------- the expected record, from the header's text
def update_scalars_f32(lr, step, b1, b2, eps, wd, sumsq, max_norm, grad_scale):
    """adamw_kernel's launch-uniform expressions in numpy fp32 (optim.hip); max_norm <= 0: no clipping"""
    lr, k, b1, b2, eps, wd = (F(x) for x in (lr, step, b1, b2, eps, wd))
    coef = clip_coef_f32(sumsq if max_norm > 0 else None, max_norm, grad_scale)
    bc1, bc2 = -np.expm1(k * np.log1p(b1 - F(1))), -np.expm1(k * np.log1p(b2 - F(1)))
    return dict(COEF=coef, STEP_SIZE=lr / bc1, INV_SQRT_BC2=F(1) / np.sqrt(bc2), DECAY=F(1) - lr * wd, OB1=F(1) - b1, OB2=F(1) - b2, BETA1=b1, BETA2=b2, EPS=eps)


def expected_state(hyper, state, step, sumsq, sched):
    """(state words as {name: value}, new step) after one vptr_optim_prepare, from the header's semantics; lr through LRSchedule.factor"""
    h = {k: float(hyper[i]) for k, i in H.items()}
    old = {k: float(state[i]) for k, i in S.items()}
    ss = F(sumsq)
    with np.errstate(all="ignore"):
        out = dict(old, GRAD_NORM=float(np.sqrt(ss) * F(h["GRAD_SCALE"])))
        if h["SKIP_NONFINITE"] != 0 and not math.isfinite(float(ss)):
            out.update(SKIP_NOW=1.0, SKIPPED_TOTAL=old["SKIPPED_TOTAL"] + 1, SKIPPED_IN_A_ROW=old["SKIPPED_IN_A_ROW"] + 1)
            return out, step
        new = step + 1
        lr = f32(h["BASE_LR"] * sched.factor(int(new) - 1))
        out.update(SKIP_NOW=0.0, SKIPPED_IN_A_ROW=0.0, LR_NOW=lr)
        out.update({k: float(v) for k, v in update_scalars_f32(lr, new, h["BETA1"], h["BETA2"], h["EPS"], h["WEIGHT_DECAY"], float(ss), h["MAX_NORM"],
                                                               h["GRAD_SCALE"]).items()})
    return out, new


TOL = dict(LR_NOW=1.0, GRAD_NORM=1.0, SKIP_NOW=0.0, SKIPPED_TOTAL=0.0, SKIPPED_IN_A_ROW=0.0, COEF=4.0, STEP_SIZE=4.0, INV_SQRT_BC2=4.0, DECAY=4.0, OB1=0.0, OB2=0.0,
           BETA1=0.0, BETA2=0.0, EPS=0.0)        # in ulp; 0: exact (1 - b is exact for b in [0.5, 1], copies and counters are exact)


def check_state(tag, got, want, start):
    """every named word within its bar, the reserved words bit for bit as `start` has them"""
    worst = 0.0
    for name, i in S.items():
        u = _ulps(got[i], want[name])
        assert u <= TOL[name], "%s: state word %s = %r, expected %r (%.1f ulp, bar %g)" % (tag, name, float(got[i]), want[name], u, TOL[name])
        worst = max(worst, u)
    assert torch.equal(bits(got)[list(RESERVED)], bits(start)[list(RESERVED)]), "%s: a reserved state word changed" % tag
    return worst


def _prepare(be, hyper, state, step, sumsq):
    """one call on guarded records -> (return code, state words, step, the records)"""
    dev = be.dev
    hr, sr = Rec(dev, hyper), Rec(dev, state)
    st, ss = Guard(1, dev, start=torch.tensor([float(step)])), Guard(1, dev, start=torch.tensor([sumsq], dtype=torch.float32))
    rc = be.call("optim_prepare", hr.out, sr.out, st.out, ss.out)
    be.sync()
    assert same_bits(hr.words(), hyper) and same_bits(ss.out.cpu(), torch.tensor([sumsq], dtype=torch.float32)) and ss.guards_intact() and st.guards_intact(), \
        "optim_prepare wrote to hyper, sumsq_dev or a guard"
    return rc, sr.words(), float(st.out.cpu()), (hr, sr, st, ss)


# ------------------------------------------------------------------------------------------------------------ 1. vptr_optim_prepare
SCHED_MAIN = dict(warmup_steps=5, total_steps=30, min_ratio=0.1)
# W = 0 (no warm-up: k = 0 is already the decay's t = 0); S = W (max(1, S - W): no division by zero, the floor is reached one step after the
# warm-up); W = 1 (the warm-up is the single factor 1 / 1); all run past S, where the factor must stay at r
SCHED_EDGES = {"W0": dict(warmup_steps=0, total_steps=8, min_ratio=0.25), "S_eq_W": dict(warmup_steps=4, total_steps=4, min_ratio=0.5),
               "W1": dict(warmup_steps=1, total_steps=6, min_ratio=0.0)}


def _run_schedule(be, sched, steps, tag):
    hyper = hyper_words(sched=sched, max_norm=1.0)
    dev = be.dev
    hr, sr = Rec(dev, hyper), Rec(dev, fresh_state())
    st, ss = Guard(1, dev, start=torch.tensor([0.0])), Guard(1, dev, start=torch.tensor([4.0]))
    worst, lrs = 0.0, []
    for k in range(steps):
        assert be.call("optim_prepare", hr.out, sr.out, st.out, ss.out) == 0, tag
        be.sync()
        got = sr.words()
        assert float(st.out.cpu()) == k + 1, "%s: step %r after %d calls" % (tag, float(st.out.cpu()), k + 1)
        want = f32(BASE_LR) * sched.factor(k)
        u = abs(float(got[S["LR_NOW"]]) - want) / (want * ULP) if want else float(got[S["LR_NOW"]] != 0)
        assert u <= 1.0, "%s: lr_now %r at k = %d, host mirror %r (%.2f ulp)" % (tag, float(got[S["LR_NOW"]]), k, want, u)
        worst = max(worst, u)
        lrs.append(float(got[S["LR_NOW"]]))
    record(tag + " lr_now worst (ulp)", worst, 1.0)
    return lrs


def run_prepare_schedule(be, kind):
    """step and lr_now over k = 0 .. 40 with W = 5, S = 30, r = 0.1"""
    sched = LRSchedule(kind, **SCHED_MAIN)
    lrs = _run_schedule(be, sched, 41, "prepare schedule %s" % kind)
    assert lrs[0] == f32(f32(BASE_LR) * 0.2) and lrs[4] == f32(BASE_LR)                     # the warm-up starts at 1 / W and ends at 1
    if kind != "constant":
        floor = f32(f32(BASE_LR) * sched.min_ratio)
        assert all(abs(x - floor) <= floor * ULP for x in lrs[30:]) and lrs[29] > floor      # past S the rate stays at r * base


def run_prepare_schedule_edges(be, edge):
    for kind in KINDS:
        sched = LRSchedule(kind, **SCHED_EDGES[edge])
        lrs = _run_schedule(be, sched, sched.total_steps + 4, "prepare schedule %s %s" % (edge, kind))
        if kind != "constant":
            floor = f32(BASE_LR) * sched.min_ratio
            assert all(abs(x - floor) <= floor * ULP for x in lrs[sched.total_steps + 1:]), (edge, kind, lrs)
        if edge == "W1":
            assert lrs[0] == f32(BASE_LR)


def run_prepare_scalars(be, k, betas):
    """the update scalars of step k (4 ulp of the numpy fp32 evaluation), then the update they produce against fp64 at test_09d's bar"""
    hyper_d = dict(HYPER, b1=betas[0], b2=betas[1])
    hyper = hyper_words(b1=betas[0], b2=betas[1], lr=HYPER["lr"])
    start = fresh_state()
    rc, got, step, _ = _prepare(be, hyper, start, k - 1, 4.0)
    assert rc == 0 and step == k
    want, _ = expected_state(hyper, start, k - 1, 4.0, LRSchedule())
    tag = "prepare scalars step %d betas %g/%g" % (k, betas[0], betas[1])
    record(tag + " worst (ulp)", check_state(tag, got, want, start), 4.0)
    b1, b2 = f32(betas[0]), f32(betas[1])
    bc1, bc2 = float(got[S["LR_NOW"]]) / float(got[S["STEP_SIZE"]]), 1.0 / float(got[S["INV_SQRT_BC2"]]) ** 2
    print("%s: bc1, bc2 derived from the record against fp64 (not asserted): %.3e %.3e" % (tag, abs(bc1 / (1.0 - b1 ** k) - 1.0), abs(bc2 / (1.0 - b2 ** k) - 1.0)))
    # p0 = 0: the stored p is the update itself at full fp32 resolution (step_tail_cases.run_adamw_precision)
    p, g, m, v = adamw_inputs(4099, k, betas[0], betas[1])
    state = (torch.zeros_like(p), g, m, v)
    bars, _, ref = adamw_bars(state, k, hyper_d, None, None, 1.0)
    out = _ctl_step(be, state, hyper, k - 1, 4.0)
    for name, a, w, bar in zip("pmv", out, ref, bars):
        val = record("%s update %s" % (tag, name), rel(a, w), bar)
        assert val <= bar, (tag, name, val, bar)


# id -> (max_norm, grad_scale, sumsq): |g|^2 = 368.6 as step_tail_cases' clip cases have it
CLIP = {"off_zero": (0.0, 1.0), "off_negative": (-1.0, 1.0), "active": (1.9, 1.0), "inactive": (50.0, 1.0), "gs_active": (0.48, 0.25), "gs_inactive": (10.0, 0.25),
        "gs_off": (0.0, 0.25)}
CLIP_SUMSQ = 368.64


def run_prepare_clip(be, case):
    max_norm, gs = CLIP[case]
    hyper, start = hyper_words(max_norm=max_norm, grad_scale=gs), fresh_state()
    rc, got, step, _ = _prepare(be, hyper, start, 3, CLIP_SUMSQ)
    assert rc == 0 and step == 4
    want, _ = expected_state(hyper, start, 3, CLIP_SUMSQ, LRSchedule())
    norm = CLIP_SUMSQ ** 0.5 * gs
    if max_norm <= 0 or "inactive" in case:
        assert want["COEF"] == f32(gs), case                              # the reference itself: no clipping leaves grad_scale alone
    else:
        assert norm > 9.0 * max_norm and want["COEF"] < 0.12 * gs, case
    check_state("prepare clip %s" % case, got, want, start)
    assert abs(float(got[S["GRAD_NORM"]]) - norm) <= 2 * ULP * norm


# 3.5e38 is above FLT_MAX (3.4028e38): written into the fp32 word it IS +Inf -- the fp32 overflow of the sum, a skip like the other two.  3.4e38
# is the finite neighbour: its square root (1.8e19) and the clip coefficient (5e-20) are ordinary numbers, never a skip
NONFINITE = {"nan": float("nan"), "inf": float("inf"), "overflow_3.5e38": 3.5e38, "big_finite": 3.4e38}


def run_prepare_nonfinite(be, which, skip):
    """every state word and step_dev after a call with sumsq = NaN / +Inf / 3.5e38 (an overflow) / 3.4e38 (finite: never a skip), from the
    record a good step left"""
    hyper = hyper_words(max_norm=1.0, skip=skip, sched=LRSchedule("cosine", **SCHED_MAIN))
    sched = LRSchedule("cosine", **SCHED_MAIN)
    rc, prior, step, _ = _prepare(be, hyper, fresh_state(), 6, 4.0)
    assert rc == 0 and step == 7
    if which == "overflow_3.5e38":
        assert math.isinf(f32(NONFINITE[which]))
    rc, got, step2, _ = _prepare(be, hyper, prior, 7, NONFINITE[which])
    assert rc == 0
    want, wstep = expected_state(hyper, prior, 7, NONFINITE[which], sched)
    skipped = bool(skip) and which != "big_finite"
    assert wstep == (7 if skipped else 8) and step2 == wstep, (which, skip, step2)
    check_state("prepare %s skip %d" % (which, skip), got, want, prior)
    if skipped:
        for name in ("LR_NOW",) + SCALARS:                                 # not merely close: untouched
            assert bits(got)[S[name]] == bits(prior)[S[name]], (which, name)
        assert float(got[S["SKIP_NOW"]]) == 1.0 and float(got[S["SKIPPED_TOTAL"]]) == 1.0
    else:
        assert float(got[S["SKIP_NOW"]]) == 0.0 and float(got[S["SKIPPED_TOTAL"]]) == 0.0
        if which == "big_finite":
            assert math.isfinite(float(got[S["GRAD_NORM"]])) and 0.0 < float(got[S["COEF"]]) < 1e-18


def run_prepare_sequence(be):
    """good, bad, bad, good with skip_nonfinite = 1 on the same records: step 1 1 1 2, skipped_total 0 1 2 2, in a row 0 1 2 0"""
    dev, sched = be.dev, LRSchedule("linear", **SCHED_MAIN)
    hyper = hyper_words(max_norm=1.0, skip=1, sched=sched)
    hr, sr, st = Rec(dev, hyper), Rec(dev, fresh_state()), Guard(1, dev, start=torch.tensor([0.0]))
    seen, words, step = [], fresh_state(), 0.0
    for sumsq in (4.0, float("nan"), float("inf"), 9.0):
        ss = scalar(sumsq, dev)
        assert be.call("optim_prepare", hr.out, sr.out, st.out, ss) == 0
        be.sync()
        want, step = expected_state(hyper, words, step, sumsq, sched)
        got = sr.words()
        check_state("prepare sequence sumsq %r" % sumsq, got, want, words)
        assert float(st.out.cpu()) == step
        words = got
        seen.append((step, float(got[S["SKIP_NOW"]]), float(got[S["SKIPPED_TOTAL"]]), float(got[S["SKIPPED_IN_A_ROW"]]), float(got[S["LR_NOW"]])))
    lr1, lr2 = f32(f32(BASE_LR) * 0.2), f32(f32(BASE_LR) * 0.4)
    assert seen == [(1.0, 0.0, 0.0, 0.0, lr1), (1.0, 1.0, 1.0, 1.0, lr1), (1.0, 1.0, 2.0, 2.0, lr1), (2.0, 0.0, 2.0, 0.0, lr2)], seen


# ---------------------------------------------------------------------------------------------------------------- 2. vptr_adamw_ctl
CTL_LAUNCH = {"big": (ADAMW_BIG, None), "big_p": (ADAMW_BIG, "p"), "big_g": (ADAMW_BIG, "g"), "big_m": (ADAMW_BIG, "m"), "big_v": (ADAMW_BIG, "v"),
              "n1": (1, None), "n3": (3, None), "n4": (4, None), "n1027": (1027, None)}
CTL_SKIP_N = {"big": ADAMW_BIG, "n1": 1, "n3": 3, "n4": 4, "n1027": 1027}
CTL_CLIP = {"absent": None, "active": 1.0 / 3.0, "inactive": 3.0}            # max_norm as a multiple of the gradient norm
CTL_WD = (0.0, 0.01)


def _sumsq_of(g):
    return f32(float((g.double() ** 2).sum()))


def _slabs(be, state, shift=None):
    dev = be.dev
    p, g, m, v = state
    n = p.numel()
    pg, mg, vg = (Guard(n, dev, start=t, shift=1 if shift == s else 0) for s, t in (("p", p), ("m", m), ("v", v)))
    gd_ = shifted(g, dev) if shift == "g" else g.to(dev)
    return pg, gd_, mg, vg


def _slab_result(gs, finite=True):
    for x in gs:
        assert x.guards_intact(), "write outside a slab"
    return tuple(x.result() if finite else x.out.cpu().clone() for x in gs)


def _ctl_step(be, state, hyper, step, sumsq, shift=None, records=None, finite=True):
    """vptr_optim_prepare + vptr_adamw_ctl on guarded copies of `state` -> p, m, v (CPU).  records: (hyper Rec, state Rec, step Guard) to go on with"""
    dev = be.dev
    hr, sr, st = records or (Rec(dev, hyper), Rec(dev, fresh_state()), Guard(1, dev, start=torch.tensor([float(step)])))
    pg, gd_, mg, vg = _slabs(be, state, shift)
    assert be.call("optim_prepare", hr.out, sr.out, st.out, scalar(sumsq, dev)) == 0
    assert be.call("adamw_ctl", pg.out, gd_, mg.out, vg.out, state[0].numel(), sr.out) == 0
    be.sync()
    sr.words()
    assert same_bits(gd_.cpu(), state[1]), "adamw_ctl changed the gradient"
    return _slab_result((pg, mg, vg), finite)


def _adamw_step(be, state, hyper_d, k, sumsq, max_norm, grad_scale=1.0, shift=None, finite=True):
    """vptr_adamw on guarded copies of `state` -> p, m, v (CPU)"""
    dev = be.dev
    pg, gd_, mg, vg = _slabs(be, state, shift)
    rc = be.call("adamw", pg.out, gd_, mg.out, vg.out, state[0].numel(), hyper_d["lr"], hyper_d["b1"], hyper_d["b2"], hyper_d["eps"], hyper_d["wd"],
                 scalar(float(k), dev), None if max_norm is None else scalar(sumsq, dev), 1.0 if max_norm is None else max_norm, grad_scale)
    assert rc == 0
    be.sync()
    return _slab_result((pg, mg, vg), finite)


def _assert_same(tag, a, b):
    for name, x, y in zip("pmv", a, b):
        assert same_bits(x, y), "%s: %s differs from vptr_adamw's in %d of %d elements" % (tag, name, int((bits(x) != bits(y)).sum()), x.numel())


def run_ctl_same_bits_launch(be, case):
    """constant schedule, step 7, clip active, weight decay 0.01: p, m, v bit-identical to vptr_adamw's in every launch class"""
    n, shift = CTL_LAUNCH[case]
    state = adamw_inputs(n, 7, HYPER["b1"], HYPER["b2"])
    sumsq = _sumsq_of(state[1])
    max_norm = f32(sumsq ** 0.5 / 3.0)
    a = _adamw_step(be, state, HYPER, 7, sumsq, max_norm, shift=shift)
    b = _ctl_step(be, state, hyper_words(max_norm=max_norm), 6, sumsq, shift=shift)
    _assert_same("adamw_ctl %s" % case, b, a)
    assert not same_bits(b[0], state[0])


def run_ctl_same_bits_clip(be, clip, wd):
    state = adamw_inputs(4099, 4, HYPER["b1"], HYPER["b2"])
    sumsq = _sumsq_of(state[1])
    max_norm = None if CTL_CLIP[clip] is None else f32(sumsq ** 0.5 * CTL_CLIP[clip])
    for gs in (1.0, 0.25):
        a = _adamw_step(be, state, dict(HYPER, wd=wd), 4, sumsq, None if max_norm is None else max_norm * gs, grad_scale=gs)
        b = _ctl_step(be, state, hyper_words(wd=wd, max_norm=None if max_norm is None else max_norm * gs, grad_scale=gs), 3, sumsq)
        _assert_same("adamw_ctl clip %s wd %g grad_scale %g" % (clip, wd, gs), b, a)


def run_ctl_same_bits_stage1(be):
    """the settings of the stage-1 and discriminator optimizers (Adam: betas (0.5, 0.999), no decay, no clipping, lr 2e-4) at steps 1 .. 4"""
    hd = dict(HYPER, lr=2e-4, b1=0.5, b2=0.999, wd=0.0)
    for k in (1, 2, 3, 4):
        state = adamw_inputs(4099, k, 0.5, 0.999)
        a = _adamw_step(be, state, hd, k, 1.0, None)
        b = _ctl_step(be, state, hyper_words(lr=2e-4, b1=0.5, b2=0.999, wd=0.0), k - 1, 1.0)
        _assert_same("adamw_ctl stage-1 settings step %d" % k, b, a)


def _grad(n, i):
    return rn((n,), 7100 + i, 0.3)


def run_ctl_cosine_same_bits(be):
    """6 consecutive steps under a cosine schedule: each bit-identical to vptr_adamw given the read-back lr_now as its lr"""
    n, dev = 1027, be.dev
    sched = LRSchedule("cosine", warmup_steps=0, total_steps=6, min_ratio=0.1)     # t = 0, 1/6, ...: six different rates
    hyper = hyper_words(max_norm=1.0, sched=sched)
    recs = (Rec(dev, hyper), Rec(dev, fresh_state()), Guard(1, dev, start=torch.tensor([0.0])))
    p, _, m, v = adamw_inputs(n, 1, HYPER["b1"], HYPER["b2"])
    m, v = torch.zeros_like(m), torch.zeros_like(v)
    seen = []
    for i in range(6):
        g = _grad(n, i)
        sumsq = _sumsq_of(g)
        b = _ctl_step(be, (p, g, m, v), hyper, i, sumsq, records=recs)
        lr_now = float(recs[1].out.cpu()[S["LR_NOW"]])
        assert float(recs[2].out.cpu()) == i + 1
        a = _adamw_step(be, (p, g, m, v), dict(HYPER, lr=lr_now), i + 1, sumsq, 1.0)
        _assert_same("adamw_ctl cosine step %d" % (i + 1), b, a)
        seen.append(lr_now)
        p, m, v = b
    assert len(set(seen)) == 6, seen                                        # the rate moved at every step


@functools.lru_cache(maxsize=1)
def trajectory_reference():
    """12 steps at n = 1027, warm-up 3, cosine to S = 12, clip at 1.0 (active: |g| = 9.6): torch.optim.AdamW on fp64 parameters under
    LambdaLR(factor) with clip_grad_norm_, and the fp32 emulation of the same trajectory (helpers.adamw_f32_emulation step by step) -> the
    reference p, m, v and their bars (adamw_bars' rule: ADAMW_BAR_FACTOR x the emulation's rel-L2 distance)"""
    n, sched = 1027, LRSchedule("cosine", warmup_steps=3, total_steps=12, min_ratio=0.1)
    h = {k: f32(x) for k, x in HYPER.items()}
    p0 = adamw_inputs(n, 1, HYPER["b1"], HYPER["b2"])[0]
    par = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([par], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sched.factor)
    emu = (p0.clone(), torch.zeros(n), torch.zeros(n))
    for i in range(12):
        g = _grad(n, i)
        par.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([par], f32(1.0))
        opt.step()
        lam.step()
        emu = adamw_f32_emulation(emu[0], g, emu[1], emu[2], i + 1, f32(h["lr"] * sched.factor(i)), h["b1"], h["b2"], h["eps"], h["wd"],
                                  coef=clip_coef_f32(_sumsq_of(g), 1.0, 1.0))
    st = opt.state[par]
    want = (par.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    dist = [rel(e, w) for e, w in zip(emu, want)]
    return sched, p0, want, [ADAMW_BAR_FACTOR * d for d in dist], dist


def run_ctl_trajectory(be):
    sched, p0, want, bars, dist = trajectory_reference()
    n, dev = p0.numel(), be.dev
    hyper = hyper_words(max_norm=1.0, sched=sched)
    recs = (Rec(dev, hyper), Rec(dev, fresh_state()), Guard(1, dev, start=torch.tensor([0.0])))
    cur = (p0, torch.zeros(n), torch.zeros(n))
    for i in range(12):
        g = _grad(n, i)
        cur = _ctl_step(be, (cur[0], g, cur[1], cur[2]), hyper, i, _sumsq_of(g), records=recs)
    print("trajectory: fp32 emulation to fp64: p %.3e m %.3e v %.3e" % tuple(dist))
    vals = [record("trajectory %s" % name, rel(a, w), bar) for name, a, w, bar in zip("pmv", cur, want, bars)]
    assert all(x <= b for x, b in zip(vals, bars)), (vals, bars)


def run_ctl_skip(be, case):
    """a NaN at the last element of g, sumsq NaN.  skip_nonfinite = 1: p, m, v bit-unchanged, and the next good step is bit-identical to a run that
    never saw the bad gradient.  skip_nonfinite = 0: the (non-finite) result equals vptr_adamw's bit for bit"""
    n, dev = CTL_SKIP_N[case], be.dev
    p, g, m, v = adamw_inputs(n, 7, HYPER["b1"], HYPER["b2"])
    bad = g.clone()
    bad[-1] = float("nan")
    good_ss = _sumsq_of(g)
    max_norm = f32(good_ss ** 0.5 / 3.0)
    hyper = hyper_words(max_norm=max_norm, skip=1)
    recs = (Rec(dev, hyper), Rec(dev, fresh_state()), Guard(1, dev, start=torch.tensor([6.0])))
    pg, gd_, mg, vg = _slabs(be, (p, bad, m, v))
    assert be.call("optim_prepare", recs[0].out, recs[1].out, recs[2].out, scalar(float("nan"), dev)) == 0
    assert be.call("adamw_ctl", pg.out, gd_, mg.out, vg.out, n, recs[1].out) == 0
    be.sync()
    assert pg.untouched() and mg.untouched() and vg.untouched(), "adamw_ctl %s: a skipped step wrote to p, m or v" % case
    assert float(recs[2].out.cpu()) == 6.0 and float(recs[1].words()[S["SKIP_NOW"]]) == 1.0
    after = _ctl_step(be, (p, g, m, v), hyper, None, good_ss, records=recs)
    clean = _ctl_step(be, (p, g, m, v), hyper, 6, good_ss)
    _assert_same("adamw_ctl %s: the good step after a skip" % case, after, clean)
    assert float(recs[2].out.cpu()) == 7.0 and float(recs[1].words()[S["SKIPPED_TOTAL"]]) == 1.0
    # without the skip: today's behaviour (fminf(1, NaN) = 1: the clip coefficient stays finite, the NaN element poisons its own p, m, v)
    a = _adamw_step(be, (p, bad, m, v), HYPER, 7, float("nan"), max_norm, finite=False)
    b = _ctl_step(be, (p, bad, m, v), hyper_words(max_norm=max_norm, skip=0), 6, float("nan"), finite=False)
    _assert_same("adamw_ctl %s: NaN gradient without the skip" % case, b, a)
    assert bool(torch.isnan(b[0][-1])) and bool(torch.isnan(b[1][-1])) and bool(torch.isnan(b[2][-1]))


def run_rejects(be):
    """a NULL pointer, a record 4 bytes off a 64-byte boundary, n <= 0: non-zero return, a message, nothing written"""
    dev = be.dev
    hyper, state = hyper_words(max_norm=1.0), fresh_state()
    p, g, m, v = adamw_inputs(1027, 7, HYPER["b1"], HYPER["b2"])

    def prepare(drop=None, shift=None):
        hr, sr = Rec(dev, hyper, shift=1 if shift == "hyper" else 0), Rec(dev, state, shift=1 if shift == "state" else 0)
        st, ss = Guard(1, dev, start=torch.tensor([3.0])), Guard(1, dev, start=torch.tensor([4.0]))
        args = [hr.out, sr.out, st.out, ss.out]
        if drop is not None:
            args[drop] = None
        rc = be.call("optim_prepare", *args)
        msg = be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("optim_prepare"), (drop, shift, rc, msg)
        assert hr.untouched() and sr.untouched() and st.untouched() and ss.untouched(), (drop, shift)

    for drop in range(4):
        prepare(drop=drop)
    prepare(shift="hyper")
    prepare(shift="state")

    def ctl(drop=None, n=1027, shift=False):
        sr = Rec(dev, state, shift=1 if shift else 0)
        pg, gd_, mg, vg = _slabs(be, (p, g, m, v))
        args = [pg.out, gd_, mg.out, vg.out, n, sr.out]
        if drop is not None:
            args[drop] = None
        rc = be.call("adamw_ctl", *args)
        msg = be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("adamw_ctl"), (drop, n, shift, rc, msg)
        assert pg.untouched() and mg.untouched() and vg.untouched() and sr.untouched(), (drop, n, shift)

    for drop in (0, 1, 2, 3, 5):
        ctl(drop=drop)
    ctl(n=0)
    ctl(n=-1)
    ctl(shift=True)


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
def _fma(a, b, c):
    """fmaf on fp32 arrays / scalars: the product is exact in fp64, the sum is rounded there and once more to fp32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


# mutation -> the cases (functions of this module with their arguments) that must fail under it
MUTATIONS = {
    "k_off_by_one": [("run_prepare_schedule", ("linear",)), ("run_prepare_schedule", ("cosine",)), ("run_prepare_sequence", ()), ("run_ctl_trajectory", ())],
    "step_on_skip": [("run_prepare_nonfinite", ("nan", 1)), ("run_prepare_nonfinite", ("inf", 1)), ("run_prepare_sequence", ()), ("run_ctl_skip", ("n1027",))],
    "coef_without_grad_scale": [("run_prepare_clip", ("gs_active",)), ("run_prepare_clip", ("gs_inactive",)), ("run_prepare_clip", ("gs_off",)),
                                ("run_ctl_same_bits_clip", ("absent", 0.01))],
    "warmup_from_zero": [("run_prepare_schedule", ("constant",)), ("run_prepare_schedule", ("cosine",)), ("run_prepare_schedule_edges", ("W1",)),
                         ("run_ctl_trajectory", ())],
}


class OptimEmu:
    """fp32 CPU emulation of vptr_optim_prepare, vptr_adamw_ctl and vptr_adamw (numpy, one rounding per operation, explicit FMAs where the
    kernels have them), with the documented argument checks.  mutation: one of MUTATIONS, a deliberate arithmetic error."""
    dev = "cpu"

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mutation, self._err = mutation, ""

    def sync(self):
        pass

    def last_error(self):
        return self._err

    def call(self, name, *a):
        return getattr(self, name)(*a)

    def _fail(self, msg):
        self._err = msg
        return -1

    def optim_prepare(self, hyper, state, step_dev, sumsq_dev):
        if any(t is None for t in (hyper, state, step_dev, sumsq_dev)):
            return self._fail("optim_prepare: a pointer is NULL")
        if hyper.data_ptr() % 64 or state.data_ptr() % 64:
            return self._fail("optim_prepare: a record is not 64-byte aligned")
        h, s = hyper.numpy(), state.numpy()
        with np.errstate(all="ignore"):
            ss, gs = F(sumsq_dev.numpy()[0]), h[H["GRAD_SCALE"]]
            s[S["GRAD_NORM"]] = np.sqrt(ss) * gs
            if h[H["SKIP_NONFINITE"]] != 0 and not np.isfinite(ss):
                s[S["SKIP_NOW"]] = 1
                s[S["SKIPPED_TOTAL"]] += F(1)
                s[S["SKIPPED_IN_A_ROW"]] += F(1)
                if self.mutation == "step_on_skip":
                    step_dev += 1.0
                return 0
            s[S["SKIP_NOW"]] = 0
            s[S["SKIPPED_IN_A_ROW"]] = 0
            step = F(step_dev.numpy()[0]) + F(1)
            step_dev.fill_(float(step))
            k = float(step) - 1.0 + (1.0 if self.mutation == "k_off_by_one" else 0.0)
            W, S_, r, kind = float(h[H["WARMUP_STEPS"]]), float(h[H["TOTAL_STEPS"]]), float(h[H["MIN_RATIO"]]), int(h[H["SCHED_KIND"]])
            f = 1.0
            if k < W:
                f = (k if self.mutation == "warmup_from_zero" else k + 1.0) / W
            elif kind:
                t = min(1.0, (k - W) / max(1.0, S_ - W))
                f = 1.0 - (1.0 - r) * t if kind == 1 else r + (1.0 - r) * (1.0 + math.cos(math.pi * t)) / 2.0
            lr = F(float(h[H["BASE_LR"]]) * f)
            b1, b2, eps, wd, max_norm = h[H["BETA1"]], h[H["BETA2"]], h[H["EPS"]], h[H["WEIGHT_DECAY"]], h[H["MAX_NORM"]]
            coef = F(1) if self.mutation == "coef_without_grad_scale" else gs
            if max_norm > 0:
                coef = coef * min(F(1), max_norm / _fma(np.sqrt(ss), gs, F(1e-6)))
            bc1, bc2 = -np.expm1(step * np.log1p(b1 - F(1))), -np.expm1(step * np.log1p(b2 - F(1)))
            for name, val in (("LR_NOW", lr), ("COEF", coef), ("STEP_SIZE", lr / bc1), ("INV_SQRT_BC2", F(1) / np.sqrt(bc2)), ("DECAY", _fma(-lr, wd, F(1))),
                              ("OB1", F(1) - b1), ("OB2", F(1) - b2), ("BETA1", b1), ("BETA2", b2), ("EPS", eps)):
                s[S[name]] = F(val)
        return 0

    @staticmethod
    def _update(p, g, m, v, n, coef, step_size, inv_sqrt_bc2, decay, ob1, ob2, b1, b2, eps):
        with np.errstate(all="ignore"):
            pv, gv, mv, vv = (t.reshape(-1)[:n].numpy() for t in (p, g, m, v))
            gi = gv * F(coef)
            mi = _fma(b1, mv, F(ob1) * gi)
            vi = _fma(b2, vv, (F(ob2) * gi) * gi)
            denom = _fma(np.sqrt(vi), inv_sqrt_bc2, eps)
            pi = _fma(pv, decay, -(F(step_size) * mi / denom))
            pv[:], mv[:], vv[:] = pi, mi, vi

    def adamw_ctl(self, p, g, m, v, n, state):
        if n <= 0:
            return self._fail("adamw_ctl: n must be positive")
        if any(t is None for t in (p, g, m, v, state)):
            return self._fail("adamw_ctl: a pointer is NULL")
        if state.data_ptr() % 64:
            return self._fail("adamw_ctl: state is not 64-byte aligned")
        s = state.numpy()
        if s[S["SKIP_NOW"]] != 0:
            return 0
        self._update(p, g, m, v, n, *(s[S[k]] for k in SCALARS))
        return 0

    def adamw(self, p, g, m, v, n, lr, b1, b2, eps, wd, step_dev, sumsq_dev, max_norm, grad_scale):
        if n <= 0 or any(t is None for t in (p, g, m, v, step_dev)):
            return self._fail("adamw: bad arguments")
        with np.errstate(all="ignore"):
            lr, b1, b2, eps, wd, max_norm, gs, step = (F(x) for x in (lr, b1, b2, eps, wd, max_norm, grad_scale, float(step_dev)))
            coef = gs
            if sumsq_dev is not None:
                coef = coef * min(F(1), max_norm / _fma(np.sqrt(F(float(sumsq_dev))), gs, F(1e-6)))
            bc1, bc2 = -np.expm1(step * np.log1p(b1 - F(1))), -np.expm1(step * np.log1p(b2 - F(1)))
            self._update(p, g, m, v, n, coef, lr / bc1, F(1) / np.sqrt(bc2), _fma(-lr, wd, F(1)), F(1) - b1, F(1) - b2, b1, b2, eps)
        return 0
