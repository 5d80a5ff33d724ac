"""Case runner of tests/test_09g_accum_ema_gpu.py: gradient accumulation and EMA weights of the device-resident optimizer controls called
through the C ABI (include/vptr_hip_accum.h) -- vptr_accum_begin, vptr_optim_prepare_accum, vptr_adamw_ctl_ema, vptr_slab_swap.

The runner talks to a BACKEND as tests/optim_ctl_cases.py does (`call(name, *args)` without the trailing stream, `last_error()`, `sync()`).
`AccumEmu` is an fp32 CPU emulation of the four entry points written from the header, on top of optim_ctl_cases.OptimEmu;
tests/test_accum_cpu.py runs every case against it and against eight named mutations, each of which must fail the cases listed in `MUTATIONS`.

Records are placed as optim_ctl_cases places them (`Rec`: 64-byte aligned inside NaN guards that must come back bit for bit).  The reserved
words of `state` (14, 15) and of `window` (12 .. 15) carry bit patterns that must survive; the host's reserved words (hyper 12 .. 15, window
3 .. 7) are NaN, must survive too, and must not leak into anything.

Bars.  lr_now of a closed window: one fp32 ulp of base_lr * LRSchedule.factor(applied updates).  EMA_OMD: one fp32 ulp of the fp64 host
mirror 1 - d_now.  The EMA per element: 2^-23 (|ema_0| + |p_new|) around ema_0 + omd (p_new - ema_0) evaluated in fp64 on the RETURNED fp32
p_new -- two roundings, the difference and the fma, each at most half an ulp of a value no larger than |ema_0| + |p_new| (omd <= 1).  The
trajectory: optim_ctl_cases' bars (step_tail_cases.adamw_bars' rule), the EMA at the bar of the parameters it averages.  Everything else is
bit for bit."""
import functools
import math

import numpy as np
import torch

import optim_ctl_cases as C
from helpers import adamw_f32_emulation, f32, rel
from optim_ctl_cases import BASE_LR, H, S, ULP, WORDS, Guard, Rec, bits, fresh_state, hyper_words, same_bits
from step_tail_cases import ADAMW_BAR_FACTOR, ADAMW_BIG, HYPER, adamw_inputs, clip_coef_f32, record, rn, scalar, shifted
from vptr_amd.optim import LRSchedule

F = np.float32
# word indices of include/vptr_hip_accum.h (tests/test_accum_cpu.py compares them with the header's #defines)
W = dict(ACCUM_STEPS=0, EMA_DECAY=1, EMA_WARMUP=2, MICRO=8, APPLY_NOW=9, EMA_OMD=10, EMA_UPDATES=11)
W_HOST_RESERVED = (3, 4, 5, 6, 7)
W_RESERVED = (12, 13, 14, 15)
W_RESERVED_BITS = (0x7FC54321, 0x0BADF00D, 0x12345678, 0x7F800001)
SIZES = {"n1": 1, "n3": 3, "n4": 4, "n1027": 1027, "big": ADAMW_BIG}     # big: the second grid-stride trip plus a scalar tail
NAN = float("nan")


def window_words(k=1, d=0.0, warm=0, micro=0.0, apply_now=0.0, omd=0.0, updates=0.0):
    w = torch.full((WORDS,), NAN)
    w[0:3] = torch.tensor([float(k), d, float(warm)], dtype=torch.float64).float()
    w[8:12] = torch.tensor([micro, apply_now, omd, updates], dtype=torch.float64).float()
    w.view(torch.int32)[list(W_RESERVED)] = torch.tensor([b - (1 << 32) if b >> 31 else b for b in W_RESERVED_BITS], dtype=torch.int64).int()
    return w


def _frozen(tag, got, before, but=()):
    """every word of a record bit-identical to `before`, apart from the words named in `but`"""
    g, b = bits(got), bits(before)
    for i in range(WORDS):
        assert i in but or g[i] == b[i], "%s: word %d changed (%#x -> %#x)" % (tag, i, int(b[i]) & 0xFFFFFFFF, int(g[i]) & 0xFFFFFFFF)


def _window_reserved_intact(tag, got, start):
    idx = list(W_HOST_RESERVED) + list(W_RESERVED) + [W["ACCUM_STEPS"], W["EMA_DECAY"], W["EMA_WARMUP"]]
    assert torch.equal(bits(got)[idx], bits(start)[idx]), "%s: a host or reserved window word changed" % tag


def seeded(n, seed):
    """ordinary values with a NaN (payload kept), an Inf and a -0.0 among them"""
    t = rn((n,), seed, 1.0)
    t[0] = NAN
    if n > 2:
        t[n // 2] = float("inf")
        t[-1] = -0.0
    return t


# -------------------------------------------------------------------------------------------------------------- 1. vptr_accum_begin
BEGIN = [(s, sh, mi) for s in SIZES for sh in (0, 1) for mi in (0, 1, 2)]


def run_begin(be, size, shift, micro):
    n, dev = SIZES[size], be.dev
    start = window_words(k=3, micro=float(micro))
    wr, g = Rec(dev, start), Guard(n, dev, start=seeded(n, 8100 + n % 97), shift=shift)
    assert be.call("accum_begin", g.out, n, wr.out) == 0, be.last_error()
    be.sync()
    assert same_bits(wr.words(), start), "accum_begin wrote to the window record"
    if micro == 0:
        assert g.guards_intact() and same_bits(g.out.cpu(), torch.zeros(n)), "accum_begin %s: the slab is not +0 everywhere" % size
    else:
        assert g.untouched(), "accum_begin %s: an open window's partial sum was touched" % size


def run_begin_rejects(be):
    dev, start = be.dev, window_words(k=2)
    for drop, n, shift in ((0, 1027, 0), (2, 1027, 0), (None, 0, 0), (None, -3, 0), (None, 1027, 1)):
        wr, g = Rec(dev, start, shift=shift), Guard(1027, dev, start=seeded(1027, 8200))
        args = [g.out, n, wr.out]
        if drop is not None:
            args[drop] = None
        rc, msg = be.call("accum_begin", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("accum_begin"), (drop, n, shift, rc, msg)
        assert g.untouched() and wr.untouched(), (drop, n, shift)


# ------------------------------------------------------------------------------------------------------ 2. vptr_optim_prepare_accum
class Records:
    """hyper, state, window, step_dev on the backend's device"""

    def __init__(self, be, hyper, window, state=None, step=0.0):
        dev = be.dev
        self.be, self.hyper, self.window0 = be, hyper, window
        self.hr, self.sr, self.wr = Rec(dev, hyper), Rec(dev, fresh_state() if state is None else state), Rec(dev, window)
        self.st = Guard(1, dev, start=torch.tensor([float(step)]))

    def call(self, sumsq):
        ss = Guard(1, self.be.dev, start=torch.tensor([sumsq], dtype=torch.float32))
        rc = self.be.call("optim_prepare_accum", self.hr.out, self.sr.out, self.wr.out, self.st.out, ss.out)
        assert rc == 0, self.be.last_error()
        self.be.sync()
        assert same_bits(self.hr.words(), self.hyper) and ss.untouched() and self.st.guards_intact(), "optim_prepare_accum wrote to hyper, sumsq_dev or a guard"
        s, w = self.sr.words(), self.wr.words()
        _window_reserved_intact("optim_prepare_accum", w, self.window0)
        assert torch.equal(bits(s)[list(C.RESERVED)], bits(fresh_state())[list(C.RESERVED)]), "a reserved state word changed"
        return s, w, float(self.st.out.cpu())

    def host_write(self, idx, value):
        """a stream-ordered write of one host word, as OptimControls issues it"""
        self.wr.out[idx:idx + 1].fill_(value)
        self.window0 = self.window0.clone()
        self.window0[idx] = value


def run_prepare_k1(be):
    """k = 1, 12 calls, the 6th with a non-finite sum and the skip on: state and step_dev torch.equal to vptr_optim_prepare run beside it"""
    sched = LRSchedule("cosine", warmup_steps=2, total_steps=10, min_ratio=0.1)
    hyper = hyper_words(max_norm=1.0, skip=1, sched=sched)
    a = Records(be, hyper, window_words(k=1, d=0.999, warm=1))
    hr, sr, st = Rec(be.dev, hyper), Rec(be.dev, fresh_state()), Guard(1, be.dev, start=torch.tensor([0.0]))
    for i in range(12):
        sumsq = float("inf") if i == 5 else 1.0 + 0.37 * i
        s, w, step = a.call(sumsq)
        assert be.call("optim_prepare", hr.out, sr.out, st.out, scalar(sumsq, be.dev)) == 0
        be.sync()
        assert torch.equal(bits(s), bits(sr.words())), "call %d: state differs from vptr_optim_prepare's:\n%r\n%r" % (i, s, sr.words())
        assert torch.equal(bits(a.st.out.cpu()), bits(st.out.cpu())), i
        assert float(w[W["MICRO"]]) == 0.0 and float(w[W["APPLY_NOW"]]) == (0.0 if i == 5 else 1.0), (i, w)
    assert step == 11.0 and float(s[S["SKIPPED_TOTAL"]]) == 1.0 and float(w[W["EMA_UPDATES"]]) == 11.0


def run_prepare_k3(be):
    """k = 3, 10 calls under a cosine schedule with a 2-update warm-up: the MICRO / APPLY_NOW / SKIP_NOW sequences, holds bit-frozen, the rate
    of each closed window at the applied-update count"""
    sched = LRSchedule("cosine", warmup_steps=2, total_steps=6, min_ratio=0.1)
    a = Records(be, hyper_words(max_norm=1.0, sched=sched), window_words(k=3, d=0.9, warm=0))
    s0, w0, step0 = a.sr.out.cpu().clone(), a.wr.out.cpu().clone(), 0.0
    seq, lrs, worst = [], [], 0.0
    for i in range(10):
        s, w, step = a.call(2.0 + i)
        seq.append((float(w[W["MICRO"]]), float(w[W["APPLY_NOW"]]), float(s[S["SKIP_NOW"]])))
        if (i + 1) % 3:
            _frozen("hold %d state" % i, s, s0, but=(S["SKIP_NOW"],))
            _frozen("hold %d window" % i, w, w0, but=(W["MICRO"], W["APPLY_NOW"]))
            assert step == step0, "hold %d advanced step_dev to %r" % (i, step)
        else:
            applied = (i + 1) // 3 - 1                      # updates applied before this one
            assert step == applied + 1.0 and float(w[W["EMA_UPDATES"]]) == applied + 1.0, (i, step, w)
            want = f32(BASE_LR) * sched.factor(applied)
            u = abs(float(s[S["LR_NOW"]]) - want) / (want * ULP)
            assert u <= 1.0, "window %d: lr_now %r, host mirror %r (%.2f ulp)" % (applied, float(s[S["LR_NOW"]]), want, u)
            worst = max(worst, u)
            lrs.append(float(s[S["LR_NOW"]]))
            assert abs(float(s[S["GRAD_NORM"]]) - math.sqrt(2.0 + i)) <= 2 * ULP * math.sqrt(2.0 + i)       # of the closing call's sum
        s0, w0, step0 = s, w, step
    assert seq == [(1.0, 0.0, 2.0), (2.0, 0.0, 2.0), (0.0, 1.0, 0.0)] * 3 + [(1.0, 0.0, 2.0)], seq
    assert len(lrs) == 3 and lrs[0] == f32(f32(BASE_LR) * 0.5) and lrs[1] == f32(BASE_LR), lrs      # the warm-up counts windows, not calls
    record("prepare_accum k3 lr_now worst (ulp)", worst, 1.0)


def run_prepare_nonfinite_hold(be):
    """a NaN / Inf sum on a hold call with the skip on is ignored; the window then closes with an update"""
    a = Records(be, hyper_words(max_norm=1.0, skip=1), window_words(k=3))
    s0, w0 = a.sr.out.cpu().clone(), a.wr.out.cpu().clone()
    for i, bad in enumerate((NAN, float("inf"))):
        s, w, step = a.call(bad)
        _frozen("non-finite hold state", s, s0, but=(S["SKIP_NOW"],))
        assert float(s[S["SKIP_NOW"]]) == 2.0 and float(s[S["SKIPPED_TOTAL"]]) == 0.0 and float(w[W["MICRO"]]) == i + 1.0 and step == 0.0
    s, w, step = a.call(4.0)
    assert float(s[S["SKIP_NOW"]]) == 0.0 and float(w[W["APPLY_NOW"]]) == 1.0 and step == 1.0 and float(s[S["SKIPPED_TOTAL"]]) == 0.0


def run_prepare_nonfinite_close(be, skip):
    """one applied window, then a window whose closing call sees an Inf sum"""
    a = Records(be, hyper_words(max_norm=1.0, skip=skip), window_words(k=2, d=0.9, warm=1))
    a.call(1.0)
    s1, w1, step1 = a.call(4.0)
    assert step1 == 1.0 and float(w1[W["EMA_UPDATES"]]) == 1.0 and float(w1[W["EMA_OMD"]]) > 0.0
    a.call(3.0)
    s, w, step = a.call(float("inf"))
    assert float(w[W["MICRO"]]) == 0.0
    if skip:
        assert float(s[S["SKIP_NOW"]]) == 1.0 and float(s[S["SKIPPED_TOTAL"]]) == 1.0 and float(s[S["SKIPPED_IN_A_ROW"]]) == 1.0 and step == 1.0
        assert float(w[W["APPLY_NOW"]]) == 0.0
        _frozen("skipped close window", w, w1, but=(W["MICRO"], W["APPLY_NOW"]))             # EMA_OMD and EMA_UPDATES as they were
        _frozen("skipped close state", s, s1, but=(S["SKIP_NOW"], S["SKIPPED_TOTAL"], S["SKIPPED_IN_A_ROW"], S["GRAD_NORM"]))
        a.call(1.0)
        s, w, step = a.call(4.0)                                                             # the next window applies
        assert float(s[S["SKIP_NOW"]]) == 0.0 and step == 2.0 and float(w[W["APPLY_NOW"]]) == 1.0 and float(w[W["EMA_UPDATES"]]) == 2.0
        assert float(s[S["SKIPPED_TOTAL"]]) == 1.0 and float(s[S["SKIPPED_IN_A_ROW"]]) == 0.0
    else:
        assert float(s[S["SKIP_NOW"]]) == 0.0 and step == 2.0 and float(w[W["APPLY_NOW"]]) == 1.0 and float(w[W["EMA_UPDATES"]]) == 2.0


def run_prepare_lower_k(be):
    """k lowered from 4 to 2 by the host while MICRO = 2: the next call closes"""
    a = Records(be, hyper_words(max_norm=1.0), window_words(k=4))
    a.call(1.0)
    s, w, step = a.call(1.0)
    assert float(w[W["MICRO"]]) == 2.0 and step == 0.0
    a.host_write(W["ACCUM_STEPS"], 2.0)
    s, w, step = a.call(1.0)
    assert float(w[W["MICRO"]]) == 0.0 and float(w[W["APPLY_NOW"]]) == 1.0 and float(s[S["SKIP_NOW"]]) == 0.0 and step == 1.0
    s, w, step = a.call(1.0)
    assert float(w[W["MICRO"]]) == 1.0 and float(s[S["SKIP_NOW"]]) == 2.0 and step == 1.0


def omd_mirror(d, warm, u):
    """fp64 host mirror of 1 - d_now on the fp32 word d"""
    d = f32(d)
    return 1.0 - (min(d, (1.0 + u) / (10.0 + u)) if warm else d)


OMD = [(w, d) for w in (0, 1) for d in (0.999, 0.9)]


def run_ema_omd(be, warm, d):
    """EMA_OMD for u = 0 .. 40 (41 consecutive updates) and u = 10^6 (seeded) at one fp32 ulp of the fp64 mirror"""
    worst = 0.0
    for u0, calls in ((0.0, 41), (1e6, 1)):
        a = Records(be, hyper_words(max_norm=1.0), window_words(k=1, d=d, warm=warm, updates=u0))
        for i in range(calls):
            s, w, _ = a.call(4.0)
            u = u0 + i
            want, got = omd_mirror(d, warm, u), float(w[W["EMA_OMD"]])
            ulps = abs(got - want) / (want * ULP)
            assert ulps <= 1.0, "EMA_OMD at u = %g, warm %d, d %g: %r, mirror %r (%.2f ulp)" % (u, warm, d, got, want, ulps)
            assert float(w[W["EMA_UPDATES"]]) == u + 1.0
            worst = max(worst, ulps)
    if warm:
        assert omd_mirror(d, 1, 0.0) == 0.9 and omd_mirror(d, 1, 1e6) == 1.0 - f32(d)       # the reference itself: 1 / 10 first, d in the end
    record("EMA_OMD warm %d d %g worst (ulp)" % (warm, d), worst, 1.0)


def run_prepare_accum_rejects(be):
    dev = be.dev
    hyper, state, window = hyper_words(max_norm=1.0), fresh_state(), window_words(k=2)
    for drop, shift in [(i, None) for i in range(5)] + [(None, "hyper"), (None, "state"), (None, "window")]:
        hr, sr, wr = (Rec(dev, t, shift=1 if shift == name else 0) for name, t in (("hyper", hyper), ("state", state), ("window", window)))
        st, ss = Guard(1, dev, start=torch.tensor([3.0])), Guard(1, dev, start=torch.tensor([4.0]))
        args = [hr.out, sr.out, wr.out, st.out, ss.out]
        if drop is not None:
            args[drop] = None
        rc, msg = be.call("optim_prepare_accum", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("optim_prepare_accum"), (drop, shift, rc, msg)
        assert all(x.untouched() for x in (hr, sr, wr, st, ss)), (drop, shift)


# ------------------------------------------------------------------------------------------------------------ 3. vptr_adamw_ctl_ema
EMA_LAUNCH = [(s, sh) for s in SIZES for sh in (None, "p", "g", "m", "v", "ema")]
EMA_D = 0.9


def _ema_start(n):
    return rn((n,), 8300 + n % 89, 0.5)


def _prepared(be, step=6.0, sumsq=4.0, max_norm=None, d=EMA_D):
    """the records after one applied k = 1 update prepared from `step`: (state Rec, window Rec)"""
    a = Records(be, hyper_words(max_norm=max_norm), window_words(k=1, d=d, warm=0), step=step)
    s, w, _ = a.call(sumsq)
    assert float(s[S["SKIP_NOW"]]) == 0.0 and float(w[W["EMA_OMD"]]) == f32(1.0 - f32(d))
    return a


def ema_bound_ok(tag, ema, ema0, p_new, omd):
    want = ema0.double() + float(omd) * (p_new.double() - ema0.double())
    err, bar = (ema.double() - want).abs(), ULP * (ema0.double().abs() + p_new.double().abs())
    bad = err > bar
    assert not bool(bad.any()), "%s: EMA outside 2^-23 (|ema_0| + |p_new|) in %d of %d elements (worst %.3e of its bar)" % (
        tag, int(bad.sum()), ema.numel(), float((err / bar.clamp_min(1e-300)).max()))
    return float((err / bar.clamp_min(1e-300)).max())


def run_ema_same_bits(be, size, shift):
    """p, m, v torch.equal to vptr_adamw_ctl on the same inputs and records; the EMA within its two-rounding bound"""
    n, dev = SIZES[size], be.dev
    state = adamw_inputs(n, 7, HYPER["b1"], HYPER["b2"])
    sumsq = C._sumsq_of(state[1])
    a = _prepared(be, sumsq=sumsq, max_norm=f32(sumsq ** 0.5 / 3.0))
    e0 = _ema_start(n)
    pg, gd_, mg, vg = C._slabs(be, state, shift)
    eg = Guard(n, dev, start=e0, shift=1 if shift == "ema" else 0)
    assert be.call("adamw_ctl_ema", pg.out, gd_, mg.out, vg.out, eg.out, n, a.sr.out, a.wr.out) == 0, be.last_error()
    be.sync()
    assert same_bits(gd_.cpu(), state[1]), "adamw_ctl_ema changed the gradient"
    got = C._slab_result((pg, mg, vg, eg))
    pg2, gd2, mg2, vg2 = C._slabs(be, state, shift)
    assert be.call("adamw_ctl", pg2.out, gd2, mg2.out, vg2.out, n, a.sr.out) == 0
    be.sync()
    C._assert_same("adamw_ctl_ema %s shift %s" % (size, shift), got[:3], C._slab_result((pg2, mg2, vg2)))
    assert not same_bits(got[0], state[0]) and not same_bits(got[3], e0)
    omd = float(a.wr.words()[W["EMA_OMD"]])
    record("adamw_ctl_ema %s shift %s worst EMA error (of its bar)" % (size, shift), ema_bound_ok("adamw_ctl_ema %s" % size, got[3], e0, got[0], omd), 1.0)


EMA_SKIP = [(s, v) for s in ("n3", "n1027", "big") for v in (1.0, 2.0)]


def run_ema_skip(be, size, skip_now):
    """SKIP_NOW = 1 (skipped) and 2 (hold): all four slabs bit-identical"""
    n, dev = SIZES[size], be.dev
    a = _prepared(be)
    sw = a.sr.out.cpu().clone()
    sw[S["SKIP_NOW"]] = skip_now
    sr = Rec(dev, sw)
    state = adamw_inputs(n, 7, HYPER["b1"], HYPER["b2"])
    pg, gd_, mg, vg = C._slabs(be, state)
    eg = Guard(n, dev, start=seeded(n, 8400))
    assert be.call("adamw_ctl_ema", pg.out, gd_, mg.out, vg.out, eg.out, n, sr.out, a.wr.out) == 0
    be.sync()
    assert pg.untouched() and mg.untouched() and vg.untouched() and eg.untouched(), "adamw_ctl_ema %s: SKIP_NOW = %g wrote to a slab" % (size, skip_now)


def run_ema_rejects(be):
    dev = be.dev
    a = _prepared(be)
    state = adamw_inputs(1027, 7, HYPER["b1"], HYPER["b2"])
    sw, ww = a.sr.out.cpu().clone(), a.wr.out.cpu().clone()
    for drop, n, shift in [(i, 1027, None) for i in (0, 1, 2, 3, 4, 6, 7)] + [(None, 0, None), (None, -1, None), (None, 1027, "state"), (None, 1027, "window")]:
        sr, wr = Rec(dev, sw, shift=1 if shift == "state" else 0), Rec(dev, ww, shift=1 if shift == "window" else 0)
        pg, gd_, mg, vg = C._slabs(be, state)
        eg = Guard(1027, dev, start=_ema_start(1027))
        args = [pg.out, gd_, mg.out, vg.out, eg.out, n, sr.out, wr.out]
        if drop is not None:
            args[drop] = None
        rc, msg = be.call("adamw_ctl_ema", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("adamw_ctl_ema"), (drop, n, shift, rc, msg)
        assert all(x.untouched() for x in (pg, mg, vg, eg, sr, wr)), (drop, n, shift)


TRAJ_D, TRAJ_STEPS = 0.9, 12


@functools.lru_cache(maxsize=1)
def ema_trajectory_reference():
    """optim_ctl_cases.trajectory_reference's 12 steps (torch.optim.AdamW on fp64 parameters under LambdaLR + clip_grad_norm_) with the EMA of
    the fp64 parameters beside them (d = 0.9 with the warm-up: d_now = min(d, (1 + u) / (10 + u))), and the fp32 emulation of both for the bars"""
    n, sched = 1027, LRSchedule("cosine", warmup_steps=3, total_steps=12, min_ratio=0.1)
    h = {k: f32(x) for k, x in HYPER.items()}
    p0 = adamw_inputs(n, 1, HYPER["b1"], HYPER["b2"])[0]
    par = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([par], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    lam = torch.optim.lr_scheduler.LambdaLR(opt, sched.factor)
    emu = (p0.clone(), torch.zeros(n), torch.zeros(n))
    ema64, ema32 = p0.double().clone(), p0.clone()
    for i in range(TRAJ_STEPS):
        g = C._grad(n, i)
        par.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([par], f32(1.0))
        opt.step()
        lam.step()
        emu = adamw_f32_emulation(emu[0], g, emu[1], emu[2], i + 1, f32(h["lr"] * sched.factor(i)), h["b1"], h["b2"], h["eps"], h["wd"],
                                  coef=clip_coef_f32(C._sumsq_of(g), 1.0, 1.0))
        omd = omd_mirror(TRAJ_D, 1, float(i))
        ema64 = ema64 + omd * (par.detach() - ema64)
        ema32 = (ema32 + torch.tensor(omd).float() * (emu[0] - ema32)).float()
    st = opt.state[par]
    want = (par.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), ema64)
    dist = [rel(e, w) for e, w in zip(emu + (ema32,), want)]
    bars = [ADAMW_BAR_FACTOR * d for d in dist]
    bars[3] = bars[0]                                   # the EMA at the bar of the parameters it averages
    return sched, p0, want, bars, dist


def run_ema_trajectory(be):
    sched, p0, want, bars, dist = ema_trajectory_reference()
    n, dev = p0.numel(), be.dev
    a = Records(be, hyper_words(max_norm=1.0, sched=sched), window_words(k=1, d=TRAJ_D, warm=1))
    cur = (p0, torch.zeros(n), torch.zeros(n), p0.clone())
    for i in range(TRAJ_STEPS):
        g = C._grad(n, i)
        a.call(C._sumsq_of(g))
        pg, gd_, mg, vg = C._slabs(be, (cur[0], g, cur[1], cur[2]))
        eg = Guard(n, dev, start=cur[3])
        assert be.call("adamw_ctl_ema", pg.out, gd_, mg.out, vg.out, eg.out, n, a.sr.out, a.wr.out) == 0
        be.sync()
        cur = C._slab_result((pg, mg, vg, eg))
    print("ema trajectory: fp32 emulation to fp64: p %.3e m %.3e v %.3e ema %.3e" % tuple(dist))
    vals = [record("ema trajectory %s" % name, rel(x, w), bar) for name, x, w, bar in zip(("p", "m", "v", "ema"), cur, want, bars)]
    assert all(x <= b for x, b in zip(vals, bars)), (vals, bars)


# ---------------------------------------------------------------------------------------------------------------- 4. vptr_slab_swap
SWAP = [(s, sh) for s in SIZES for sh in (None, "a", "b")]


def run_swap(be, size, shift):
    n, dev = SIZES[size], be.dev
    a0, b0 = seeded(n, 8500), rn((n,), 8501, 2.0)
    ag, bg = Guard(n, dev, start=a0, shift=1 if shift == "a" else 0), Guard(n, dev, start=b0, shift=1 if shift == "b" else 0)
    assert be.call("slab_swap", ag.out, bg.out, n) == 0, be.last_error()
    be.sync()
    assert ag.guards_intact() and bg.guards_intact(), "slab_swap wrote outside a slab"
    assert same_bits(ag.out.cpu(), b0) and same_bits(bg.out.cpu(), a0), "slab_swap %s shift %s" % (size, shift)


def run_swap_rejects(be):
    dev, n = be.dev, 1027
    for case in ("null_a", "null_b", "n0", "n_neg", "overlap_lo", "overlap_hi", "same"):
        ag, bg = Guard(2 * n, dev, start=rn((2 * n,), 8600, 1.0)), Guard(n, dev, start=rn((n,), 8601, 1.0))
        args = {"null_a": (None, bg.out, n), "null_b": (ag.out, None, n), "n0": (ag.out, bg.out, 0), "n_neg": (ag.out, bg.out, -4),
                "overlap_lo": (ag.out[:n], ag.out[n - 1:2 * n - 1], n), "overlap_hi": (ag.out[4:4 + n], ag.out[:n], n), "same": (ag.out[:n], ag.out[:n], n)}[case]
        rc, msg = be.call("slab_swap", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("slab_swap"), (case, rc, msg)
        assert ag.untouched() and bg.untouched(), case
    # adjacent ranges do not overlap
    ag = Guard(2 * n, dev, start=rn((2 * n,), 8602, 1.0))
    assert be.call("slab_swap", ag.out[:n], ag.out[n:], n) == 0, be.last_error()
    be.sync()
    assert same_bits(ag.out.cpu()[:n], ag.start[n:]) and same_bits(ag.out.cpu()[n:], ag.start[:n]) and ag.guards_intact()


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
# mutation -> the cases (functions of this module with their arguments) that must fail under it
MUTATIONS = {
    "begin_zeroes_open_window": [("run_begin", ("n3", 0, 1)), ("run_begin", ("n1027", 1, 2)), ("run_begin", ("big", 0, 1))],
    "hold_advances_step": [("run_prepare_k3", ()), ("run_prepare_nonfinite_hold", ()), ("run_prepare_lower_k", ())],
    "hold_counts_nonfinite": [("run_prepare_nonfinite_hold", ())],
    "close_keeps_micro": [("run_prepare_k3", ()), ("run_prepare_nonfinite_close", (1,)), ("run_prepare_lower_k", ())],
    "ema_reads_old_p": [("run_ema_same_bits", ("n1", None)), ("run_ema_same_bits", ("n1027", "ema")), ("run_ema_trajectory", ())],
    "warmup_u_plus_1": [("run_ema_omd", (1, 0.999)), ("run_ema_omd", (1, 0.9))],
    "skipped_close_advances_ema": [("run_prepare_nonfinite_close", (1,)), ("run_prepare_k1", ())],
    "swap_one_way": [("run_swap", ("n1", None)), ("run_swap", ("n1027", "a")), ("run_swap", ("big", "b")), ("run_swap_rejects", ())],
}


class AccumEmu(C.OptimEmu):
    """optim_ctl_cases.OptimEmu plus fp32 CPU emulations of the four entry points of include/vptr_hip_accum.h.  mutation: one of MUTATIONS."""

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        super().__init__(None)
        self.mutation = mutation

    def accum_begin(self, grad, n, window):
        if n <= 0:
            return self._fail("accum_begin: n must be positive")
        if grad is None or window is None:
            return self._fail("accum_begin: a pointer is NULL")
        if window.data_ptr() % 64:
            return self._fail("accum_begin: window is not 64-byte aligned")
        if window.numpy()[W["MICRO"]] == 0 or self.mutation == "begin_zeroes_open_window":
            grad.reshape(-1)[:n].numpy()[:] = F(0)
        return 0

    def optim_prepare_accum(self, hyper, state, window, step_dev, sumsq_dev):
        if any(t is None for t in (hyper, state, window, step_dev, sumsq_dev)):
            return self._fail("optim_prepare_accum: a pointer is NULL")
        if hyper.data_ptr() % 64 or state.data_ptr() % 64 or window.data_ptr() % 64:
            return self._fail("optim_prepare_accum: a record is not 64-byte aligned")
        w, s, h = window.numpy(), state.numpy(), hyper.numpy()
        micro = F(w[W["MICRO"]] + F(1))
        if micro < w[W["ACCUM_STEPS"]]:
            w[W["MICRO"]], w[W["APPLY_NOW"]], s[S["SKIP_NOW"]] = micro, 0, 2
            if self.mutation == "hold_advances_step":
                step_dev += 1.0
            if self.mutation == "hold_counts_nonfinite" and h[H["SKIP_NONFINITE"]] != 0 and not np.isfinite(sumsq_dev.numpy()[0]):
                s[S["SKIPPED_TOTAL"]] += F(1)
            return 0
        if self.mutation != "close_keeps_micro":
            w[W["MICRO"]] = 0
        rc = self.optim_prepare(hyper, state, step_dev, sumsq_dev)
        assert rc == 0
        w[W["APPLY_NOW"]] = F(1) - s[S["SKIP_NOW"]]
        if s[S["SKIP_NOW"]] == 0 or self.mutation == "skipped_close_advances_ema":
            u, d = float(w[W["EMA_UPDATES"]]), float(w[W["EMA_DECAY"]])
            uu = u + 1.0 if self.mutation == "warmup_u_plus_1" else u
            d_now = min(d, (1.0 + uu) / (10.0 + uu)) if w[W["EMA_WARMUP"]] != 0 else d
            w[W["EMA_OMD"]] = F(1.0 - d_now)
            w[W["EMA_UPDATES"]] = F(w[W["EMA_UPDATES"]] + F(1))
        return 0

    def adamw_ctl_ema(self, p, g, m, v, ema, n, state, window):
        if n <= 0:
            return self._fail("adamw_ctl_ema: n must be positive")
        if any(t is None for t in (p, g, m, v, ema, state, window)):
            return self._fail("adamw_ctl_ema: a pointer is NULL")
        if state.data_ptr() % 64 or window.data_ptr() % 64:
            return self._fail("adamw_ctl_ema: a record is not 64-byte aligned")
        s = state.numpy()
        if s[S["SKIP_NOW"]] != 0:
            return 0
        old = p.reshape(-1)[:n].numpy().copy()
        self._update(p, g, m, v, n, *(s[S[k]] for k in C.SCALARS))
        with np.errstate(all="ignore"):
            ev = ema.reshape(-1)[:n].numpy()
            src = old if self.mutation == "ema_reads_old_p" else p.reshape(-1)[:n].numpy()
            ev[:] = C._fma(window.numpy()[W["EMA_OMD"]], src - ev, ev)
        return 0

    def slab_swap(self, a, b, n):
        if n <= 0:
            return self._fail("slab_swap: n must be positive")
        if a is None or b is None:
            return self._fail("slab_swap: a pointer is NULL")
        if not (a.data_ptr() + 4 * n <= b.data_ptr() or b.data_ptr() + 4 * n <= a.data_ptr()):
            return self._fail("slab_swap: the ranges overlap")
        av, bv = a.reshape(-1)[:n].numpy(), b.reshape(-1)[:n].numpy()
        tmp = av.copy()
        av[:] = bv
        if self.mutation != "swap_one_way":
            bv[:] = tmp
        return 0


def all_cases():
    out = [("run_begin", c) for c in BEGIN] + [("run_begin_rejects", ())]
    out += [("run_prepare_k1", ()), ("run_prepare_k3", ()), ("run_prepare_nonfinite_hold", ()), ("run_prepare_nonfinite_close", (0,)), ("run_prepare_nonfinite_close", (1,)),
            ("run_prepare_lower_k", ())] + [("run_ema_omd", c) for c in OMD] + [("run_prepare_accum_rejects", ())]
    out += [("run_ema_same_bits", c) for c in EMA_LAUNCH] + [("run_ema_skip", c) for c in EMA_SKIP] + [("run_ema_rejects", ()), ("run_ema_trajectory", ())]
    out += [("run_swap", c) for c in SWAP] + [("run_swap_rejects", ())]
    return out


def case_id(c):
    return c[0][4:] + "".join("-%s" % a for a in c[1])
