"""Case runner of tests/test_09j_param_groups_gpu.py: the parameter groups of the device-resident optimizer controls called through the C
ABI (include/vptr_hip_groups.h) -- vptr_optim_group_scalars and vptr_adamw_groups, in the plain form and in the EMA form.

The runner talks to a BACKEND as tests/optim_ctl_cases.py and tests/accum_cases.py do (`call(name, *args)` without the trailing stream,
`last_error()`, `sync()`, and `group_map(layout, group_of, numel)`: the host function that lays the byte map out).  `GroupEmu` is an fp32
CPU emulation of the two entry points written from the header, on top of accum_cases.AccumEmu; tests/test_param_groups_cpu.py runs every
case against it and against six named mutations, each of which must fail the cases listed in `MUTATIONS`.

Every slab, record and table sits inside NaN guard rows (`Guard`, `Rec`, `Tab`); the map inside 0xEE guard bytes (`ByteGuard`).  The
reserved words of both tables carry bit patterns that must survive.

References.  (1) Bit for bit: the ungrouped kernels.  For each group g, vptr_adamw_ctl (vptr_adamw_ctl_ema) is run on the same inputs with
a copy of the state record whose STEP_SIZE and DECAY words are gstate[g]'s; element i of the grouped result must equal element i of the
run of group gid[i].  That pins the map lookup -- every launch class, every boundary -- without any tolerance.  (2) fp64: `groups_ref64`,
helpers.adamw_ref per group with lr_g = base_lr * f(k) * lr_scale_g, which tests/test_param_groups_cpu.py pins to torch.optim.AdamW with
param_groups + LambdaLR + clip_grad_norm_ at 1e-12.  Bars as tests/test_09d derives them (step_tail_cases.adamw_bars' rule): five times
the rel-L2 distance to fp64 of an fp32 evaluation of the same formulas (helpers.adamw_f32_emulation per group), p, m, v separately."""
import functools

import numpy as np
import torch

import accum_cases as A
import optim_ctl_cases as C
from helpers import adamw_f32_emulation, adamw_ref, f32, rel
from optim_ctl_cases import BASE_LR, S, Guard, Rec, bits, fresh_state, hyper_words, same_bits
from step_tail_cases import ADAMW_BAR_FACTOR, ADAMW_BIG, HYPER, adamw_inputs, clip_coef_f32, record, rn, scalar, shifted
from vptr_amd.optim import LRSchedule

F = np.float32
MAX_GROUPS, G_WORDS = 16, 4
# word indices of include/vptr_hip_groups.h (tests/test_param_groups_cpu.py compares them with the header's #defines)
GH = dict(LR_SCALE=0, WEIGHT_DECAY=1)
GS = dict(STEP_SIZE=0, DECAY=1, LR=2)
TAB = MAX_GROUPS * G_WORDS
GH_RESERVED_BITS, GS_RESERVED_BITS = 0x7FC0BEEF, 0x0BADCAFE
SIZES = {"n1": 1, "n3": 3, "n4": 4, "n5": 5, "n1027": 1027, "big": ADAMW_BIG}     # big: the second grid-stride trip plus a scalar tail
NAN = float("nan")
WD = HYPER["wd"]


def _i32(b):
    return b - (1 << 32) if b >> 31 else b


def ghyper_words(specs):
    """the table the host writes: {lr_scale, weight_decay, reserved, reserved} per group (reserved: NaN -- must not leak into anything);
    the records past the last group are NaN altogether"""
    w = torch.full((TAB,), NAN)
    for g, (scale, wd) in enumerate(specs):
        w[g * G_WORDS:g * G_WORDS + 2] = torch.tensor([scale, wd], dtype=torch.float64).float()
    return w


def fresh_gstate():
    """zeros with a bit pattern in the reserved word (word 3) of every record"""
    w = torch.zeros(TAB)
    w.view(torch.int32)[3::G_WORDS] = _i32(GS_RESERVED_BITS)
    return w


class Tab(Guard):
    """a 16 x 4 word group table inside its guards"""

    def __init__(self, dev, start, shift=0):
        super().__init__(TAB, dev, start=start, shift=shift)
        assert shift or self.out.data_ptr() % 64 == 0

    def words(self):
        assert self.guards_intact(), "write outside a group table"
        return self.out.cpu().clone()


class ByteGuard:
    """n map bytes inside 16 guard bytes of 0xEE on both sides; shift = 1 puts the map one byte past a 4-byte boundary"""

    def __init__(self, gid, dev, shift=0):
        self.n, self.lo = gid.numel(), 16 + shift
        self.start = gid.detach().reshape(-1).to(torch.uint8).cpu().clone()
        self.buf = torch.full((self.lo + self.n + 16,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = self.buf[self.lo:self.lo + self.n]
        self.out.copy_(self.start)
        assert self.out.data_ptr() % 4 == shift

    def untouched(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == 0xEE).all()) and bool((b[self.lo + self.n:] == 0xEE).all()) and torch.equal(b[self.lo:self.lo + self.n], self.start)


class Recs:
    """hyper, state, step_dev (and window, for the EMA form) on the backend's device, prepared by the launch that belongs to the form:
    vptr_optim_prepare, or vptr_optim_prepare_accum with k = 1"""

    def __init__(self, be, ema, hyper, step=0.0, d=0.9):
        dev = be.dev
        self.be, self.ema, self.hyper = be, ema, hyper
        self.hr, self.sr = Rec(dev, hyper), Rec(dev, fresh_state())
        self.st = Guard(1, dev, start=torch.tensor([float(step)]))
        self.wr = Rec(dev, A.window_words(k=1, d=d, warm=0)) if ema else None

    def prepare(self, sumsq):
        ss = scalar(sumsq, self.be.dev)
        if self.ema:
            rc = self.be.call("optim_prepare_accum", self.hr.out, self.sr.out, self.wr.out, self.st.out, ss)
        else:
            rc = self.be.call("optim_prepare", self.hr.out, self.sr.out, self.st.out, ss)
        assert rc == 0, self.be.last_error()
        self.be.sync()
        return self.sr.words()

    def window(self):
        return self.wr.out if self.ema else None


def make_map(n, ngroups, kind="mix", seed=0):
    """mix: neighbours in different groups (7 is coprime to every group count used), the pattern shifted every 5 elements so that it has
    no period of 4; runs: contiguous runs of unequal lengths"""
    idx = torch.arange(n, dtype=torch.int64)
    if kind == "mix":
        return ((idx * 7 + (idx // 5) * 3 + seed) % ngroups).to(torch.uint8)
    edges = sorted({(j * n) // ngroups + (j % 3) for j in range(1, ngroups)})
    return torch.bucketize(idx, torch.tensor(edges, dtype=torch.int64), right=True).clamp_max(ngroups - 1).to(torch.uint8)


def _ema_start(n):
    return rn((n,), 9300 + n % 89, 0.5)


def _inputs(n, k=7):
    return adamw_inputs(n, k, HYPER["b1"], HYPER["b2"])


def scalars_call(be, r, gh, gs, ngroups):
    rc = be.call("optim_group_scalars", r.sr.out, gh.out, gs.out, ngroups)
    assert rc == 0, be.last_error()
    be.sync()
    assert gh.untouched(), "optim_group_scalars wrote to ghyper"
    return gs.words()


def groups_call(be, r, state4, e0, gid, gs, ngroups, shift=None):
    """vptr_adamw_groups on guarded copies -> (p, m, v[, ema]) on the CPU; the gradient, the map, state, window and gstate must come back
    bit for bit"""
    n, dev = state4[0].numel(), be.dev
    pg, gd_, mg, vg = C._slabs(be, state4, shift)
    eg = Guard(n, dev, start=e0, shift=1 if shift == "ema" else 0) if r.ema else None
    mp = ByteGuard(gid, dev, shift=1 if shift == "gid" else 0)
    s0, g0 = r.sr.out.cpu().clone(), gs.out.cpu().clone()
    w0 = r.wr.out.cpu().clone() if r.ema else None
    rc = be.call("adamw_groups", pg.out, gd_, mg.out, vg.out, eg.out if r.ema else None, mp.out, n, r.sr.out, r.window(), gs.out, ngroups)
    assert rc == 0, be.last_error()
    be.sync()
    assert same_bits(gd_.cpu(), state4[1]) and mp.untouched(), "adamw_groups changed the gradient or the map"
    assert same_bits(r.sr.words(), s0) and same_bits(gs.words(), g0) and (not r.ema or same_bits(r.wr.words(), w0)), "adamw_groups wrote to a record"
    return C._slab_result((pg, mg, vg) + ((eg,) if r.ema else ()), finite=False)


def by_groups_reference(be, r, state4, e0, gid, gstate, ngroups, groups=None):
    """the ungrouped kernel once per group that the map uses, with that group's step size and decay in the state record; element i from
    the run of group gid[i]"""
    n, dev = state4[0].numel(), be.dev
    out = None
    for g in sorted(set(int(x) for x in gid.unique()) if groups is None else groups):
        sw = r.sr.out.cpu().clone()
        sw[S["STEP_SIZE"]], sw[S["DECAY"]] = gstate[g * G_WORDS + GS["STEP_SIZE"]], gstate[g * G_WORDS + GS["DECAY"]]
        sr = Rec(dev, sw)
        pg, gd_, mg, vg = C._slabs(be, state4)
        if r.ema:
            eg = Guard(n, dev, start=e0)
            assert be.call("adamw_ctl_ema", pg.out, gd_, mg.out, vg.out, eg.out, n, sr.out, r.wr.out) == 0, be.last_error()
        else:
            assert be.call("adamw_ctl", pg.out, gd_, mg.out, vg.out, n, sr.out) == 0, be.last_error()
        be.sync()
        res = C._slab_result((pg, mg, vg) + ((eg,) if r.ema else ()), finite=False)
        if out is None:
            out = [t.clone() for t in res]
        sel = gid == g
        for o, t in zip(out, res):
            o[sel] = t[sel]
    return out


def assert_same(tag, got, want):
    for name, x, y in zip(("p", "m", "v", "ema"), got, want):
        assert same_bits(x, y), "%s: %s differs from the per-group reference in %d of %d elements (first at %d)" % (
            tag, name, int((bits(x) != bits(y)).sum()), x.numel(), int((bits(x) != bits(y)).nonzero()[0]))


SPECS3 = [(1.0, WD), (0.1, 0.0), (2.5, 0.05)]


def _step(be, ema, n, gid, specs, shift=None, k=7, ngroups=None):
    """prepare -> group scalars -> grouped update with the clip active; -> (records, state, ema start, gstate words, result)"""
    ngroups = len(specs) if ngroups is None else ngroups
    state4 = _inputs(n, k)
    sumsq = C._sumsq_of(state4[1])
    r = Recs(be, ema, hyper_words(max_norm=f32(sumsq ** 0.5 / 3.0)), step=k - 1.0)
    r.prepare(sumsq)
    gs = Tab(be.dev, fresh_gstate())
    gstate = scalars_call(be, r, Tab(be.dev, ghyper_words(specs)), gs, ngroups)
    e0 = _ema_start(n) if ema else None
    return r, state4, e0, gstate, gs, groups_call(be, r, state4, e0, gid, gs, ngroups, shift)


# ------------------------------------------------------------------------------------------------------------------------ 1. sizes
SIZE_CASES = [(s, e) for s in SIZES for e in (0, 1)]


def run_sizes(be, size, ema):
    n = SIZES[size]
    gid = make_map(n, 3)
    r, state4, e0, gstate, gs, got = _step(be, ema, n, gid, SPECS3)
    assert_same("adamw_groups %s ema %d" % (size, ema), got, by_groups_reference(be, r, state4, e0, gid, gstate, 3))
    assert not same_bits(got[0], state4[0]) and bool(torch.isfinite(torch.stack([t.double().abs().max() for t in got])).all())


# ----------------------------------------------------------------------------------------------------------- 2. misaligned pointers
SHIFT_CASES = [("n1027", sh, e) for e in (0, 1) for sh in ("p", "g", "m", "v", "gid") + (("ema",) if e else ())] + [("big", "gid", 0), ("big", "p", 1)]


def run_shift(be, size, shift, ema):
    """one pointer off its grid: the all-scalar path, bit-identical to the float4 path"""
    n = SIZES[size]
    gid = make_map(n, 3, seed=3)
    _, _, _, _, _, aligned = _step(be, ema, n, gid, SPECS3)
    _, state4, _, _, _, off = _step(be, ema, n, gid, SPECS3, shift=shift)
    assert_same("adamw_groups %s shift %s ema %d" % (size, shift, ema), off, aligned)
    assert not same_bits(off[0], state4[0])


# -------------------------------------------------------------------------------------------------------------- 3. group boundaries
BOUND_N = 4099                     # 1024 float4 on 5 workgroups and a 3-element tail
BOUNDARIES = {"quad1": 1, "quad2": 2, "quad3": 3, "mid_quad": 2050, "k1024": 1024, "k3072": 3072, "last": BOUND_N - 1, "tail": BOUND_N - 2}
BOUND_CASES = [(b, e) for b in BOUNDARIES for e in (0, 1)]


def run_boundary(be, where, ema):
    """group 0 below the boundary, group 1 from it on; the elements on either side carry their own group's update"""
    b = BOUNDARIES[where]
    gid = (torch.arange(BOUND_N) >= b).to(torch.uint8)
    specs = [(1.0, WD), (0.25, 0.0)]
    r, state4, e0, gstate, gs, got = _step(be, ema, BOUND_N, gid, specs)
    want = by_groups_reference(be, r, state4, e0, gid, gstate, 2)
    assert_same("boundary %s ema %d" % (where, ema), got, want)
    other = by_groups_reference(be, r, state4, e0, 1 - gid, gstate, 2)
    assert bits(got[0])[b - 1] != bits(other[0])[b - 1] and bits(got[0])[b] != bits(other[0])[b], "the two groups do not differ at the boundary"


NGROUPS_CASES = [(g, kind, e) for g in (1, 2, 16) for kind in ("mix", "runs") for e in (0, 1)]


def run_ngroups(be, ngroups, kind, ema):
    specs = [(1.0 + 0.125 * g if g % 3 else 0.5 / (g + 1), WD * (g % 4)) for g in range(ngroups)]
    gid = make_map(BOUND_N, ngroups, kind, seed=ngroups)
    assert int(gid.max()) == ngroups - 1 and len(gid.unique()) == ngroups
    r, state4, e0, gstate, gs, got = _step(be, ema, BOUND_N, gid, specs)
    assert_same("ngroups %d %s ema %d" % (ngroups, kind, ema), got, by_groups_reference(be, r, state4, e0, gid, gstate, ngroups))


def run_empty_group(be, ema):
    """group 1 of 3 owns no element: its record is computed and nothing else changes"""
    gid = make_map(BOUND_N, 2, seed=5) * 2
    r, state4, e0, gstate, gs, got = _step(be, ema, BOUND_N, gid, SPECS3)
    assert_same("empty group ema %d" % ema, got, by_groups_reference(be, r, state4, e0, gid, gstate, 3))
    assert float(gstate[G_WORDS + GS["LR"]]) == f32(f32(BASE_LR) * f32(0.1))


def run_byte_out_of_range(be, ema):
    """a map byte of 200 with 3 groups: no fault, nothing outside the slabs touched (groups_call checks every guard and record), every
    element in range as its group says, and the stray elements as ONE of the groups says"""
    gid = make_map(1027, 3, seed=9)
    stray = [0, 5, 514, 1024, 1026]
    bad = gid.clone()
    bad[stray] = 200
    r, state4, e0, gstate, gs, got = _step(be, ema, 1027, bad, SPECS3)
    want = by_groups_reference(be, r, state4, e0, gid, gstate, 3)
    keep = torch.ones(1027, dtype=torch.bool)
    keep[stray] = False
    assert_same("byte 200 ema %d" % ema, [t[keep] for t in got], [t[keep] for t in want])
    per_group = [by_groups_reference(be, r, state4, e0, torch.full((1027,), g, dtype=torch.uint8), gstate, 3) for g in range(3)]
    for i in stray:
        assert any(all(bits(x)[i] == bits(y)[i] for x, y in zip(got, ref)) for ref in per_group), "element %d follows no group" % i


def run_pad_group(be):
    """the host's map: parameters of 5 and 6 elements in groups 1 and 2 and one pad element -- the pad belongs to group 0"""
    layout, group_of = [(0, 5, None), (5, 6, None)], [1, 2]
    gid = be.group_map(layout, group_of, 12)
    assert gid.dtype == torch.uint8 and gid.tolist() == [1] * 5 + [2] * 6 + [0], gid.tolist()
    r, state4, e0, gstate, gs, got = _step(be, 0, 12, gid, SPECS3)
    assert_same("pad element", got, by_groups_reference(be, r, state4, e0, torch.tensor([1] * 5 + [2] * 6 + [0], dtype=torch.uint8), gstate, 3))


# --------------------------------------------------------------------------------------------------------------------- 4. bit identity
IDENT_CASES = [(s, g, e) for s in ("n5", "n1027", "big") for g in (1, 16) for e in (0, 1)]


def run_identity(be, size, ngroups, ema):
    """every group at lr_scale 1 with the optimizer's decay: gstate words == state words, and p, m, v (ema) == the ungrouped kernel's for
    an arbitrary map"""
    n = SIZES[size]
    gid = make_map(n, ngroups, seed=11)
    r, state4, e0, gstate, gs, got = _step(be, ema, n, gid, [(1.0, WD)] * ngroups)
    sw = r.sr.words()
    for g in range(ngroups):
        assert bits(gstate)[g * G_WORDS + GS["STEP_SIZE"]] == bits(sw)[S["STEP_SIZE"]] and bits(gstate)[g * G_WORDS + GS["DECAY"]] == bits(sw)[S["DECAY"]], g
        assert bits(gstate)[g * G_WORDS + GS["LR"]] == bits(sw)[S["LR_NOW"]], g
    pg, gd_, mg, vg = C._slabs(be, state4)
    if ema:
        eg = Guard(n, be.dev, start=e0)
        assert be.call("adamw_ctl_ema", pg.out, gd_, mg.out, vg.out, eg.out, n, r.sr.out, r.wr.out) == 0
    else:
        assert be.call("adamw_ctl", pg.out, gd_, mg.out, vg.out, n, r.sr.out) == 0
    be.sync()
    assert_same("identity %s %d groups ema %d" % (size, ngroups, ema), got, C._slab_result((pg, mg, vg) + ((eg,) if ema else ())))
    assert not same_bits(got[0], state4[0])


# --------------------------------------------------------------------------------------------------------------------- 5. the scalars
def run_scalars(be):
    """lr_g, step_size_g, decay_g of 16 groups under a cosine schedule at step 10 against their definitions; records past ngroups and the
    reserved words stay"""
    sched = LRSchedule("cosine", warmup_steps=2, total_steps=40, min_ratio=0.1)
    r = Recs(be, 0, hyper_words(max_norm=1.0, sched=sched), step=9.0)
    sw = r.prepare(4.0)
    specs = [(s, w) for s in (0.0, 0.1, 1.0, 2.5) for w in (0.0, 0.01)] + [(1.0, WD), (0.5, 0.3), (3.0, 0.0), (1e-3, 1.0)]
    gs0 = fresh_gstate()
    gs0[12 * G_WORDS:] = rn((TAB - 12 * G_WORDS,), 9100, 1.0)
    got = scalars_call(be, r, Tab(be.dev, ghyper_words(specs)), Tab(be.dev, gs0), 12)
    lr_now, step_size = F(sw[S["LR_NOW"]]), F(sw[S["STEP_SIZE"]])
    for g, (scale, wd) in enumerate(specs):
        lr = lr_now * F(scale)
        want = (step_size * F(scale), C._fma(-lr, F(wd), F(1)), lr)
        for name, w in zip(("STEP_SIZE", "DECAY", "LR"), want):
            assert bits(got)[g * G_WORDS + GS[name]] == bits(torch.tensor([float(w)], dtype=torch.float32))[0], (g, name, float(got[g * G_WORDS + GS[name]]), float(w))
    assert float(got[GS["STEP_SIZE"]]) == 0.0 and float(got[GS["DECAY"]]) == 1.0 and float(got[GS["LR"]]) == 0.0      # lr_scale 0
    assert bits(got)[8 * G_WORDS + GS["STEP_SIZE"]] == bits(sw)[S["STEP_SIZE"]] and bits(got)[8 * G_WORDS + GS["DECAY"]] == bits(sw)[S["DECAY"]]
    assert same_bits(got[12 * G_WORDS:], gs0[12 * G_WORDS:]) and same_bits(got[3::G_WORDS], gs0[3::G_WORDS]), "a record past ngroups or a reserved word changed"
    # one rounding more than fp32(lr_g / bc1): within 1 ulp of it
    for g, (scale, _) in enumerate(specs):
        if scale:
            bc1 = float(lr_now) / float(step_size)
            assert abs(float(got[g * G_WORDS]) - float(lr_now) * f32(scale) / bc1) <= 2.0 * C.ULP * float(got[g * G_WORDS]), g


# ------------------------------------------------------------------------------------------------------------------- 6. against fp64
REF_SCALES, REF_DECAYS = (0.0, 0.1, 1.0, 2.5), (0.0, 0.01)
REF_SPECS = [(s, w) for s in REF_SCALES for w in REF_DECAYS]
REF_STEPS = (1, 2, 10, 1000)
REF_N = 4099
REF_SCHED = dict(kind="cosine", warmup_steps=3, total_steps=2000, min_ratio=0.1)
REF_CLIP = 1.0 / 3.0               # max_norm as a multiple of the gradient norm: the clip is active


def ref_inputs(k):
    state4 = _inputs(REF_N, k)
    sumsq = C._sumsq_of(state4[1])
    return state4, sumsq, f32(sumsq ** 0.5 * REF_CLIP), make_map(REF_N, len(REF_SPECS), seed=k)


def groups_ref64(state4, gid, specs, k, lr_now, sumsq, max_norm, b1=HYPER["b1"], b2=HYPER["b2"], eps=HYPER["eps"]):
    """fp64 p, m, v of one grouped step: helpers.adamw_ref per group with lr_g = lr_now * fp32(lr_scale_g) and fp32(weight_decay_g);
    lr_now = fp32(base_lr) * f(k - 1) in fp64"""
    p, g, m, v = state4
    out = [t.double().clone() for t in (p, m, v)]
    for grp, (scale, wd) in enumerate(specs):
        res = adamw_ref(p, g, m, v, k, lr_now * f32(scale), f32(b1), f32(b2), f32(eps), f32(wd), sumsq=sumsq, max_norm=f32(max_norm), abi_hyper=False)
        sel = gid == grp
        for o, t in zip(out, res):
            o[sel] = t[sel]
    return out


@functools.lru_cache(maxsize=None)
def ref_case(k):
    """inputs, the fp64 reference, and the bars: ADAMW_BAR_FACTOR x the distance of the fp32 evaluation of the same formulas"""
    state4, sumsq, max_norm, gid = ref_inputs(k)
    sched = LRSchedule(**REF_SCHED)
    lr_now = f32(BASE_LR) * sched.factor(k - 1)
    want = groups_ref64(state4, gid, REF_SPECS, k, lr_now, sumsq, max_norm)
    emu = [t.clone() for t in (state4[0], state4[2], state4[3])]
    coef = clip_coef_f32(sumsq, max_norm, 1.0)
    for grp, (scale, wd) in enumerate(REF_SPECS):
        res = adamw_f32_emulation(*state4, k, float(F(f32(lr_now)) * F(scale)), HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, coef=coef)
        sel = gid == grp
        for o, t in zip(emu, res):
            o[sel] = t[sel]
    dist = [rel(e, w) for e, w in zip(emu, want)]
    return state4, sumsq, max_norm, gid, sched, want, [ADAMW_BAR_FACTOR * d for d in dist], dist


REF_CASES = [(k, e) for k in REF_STEPS for e in (0, 1)]


def run_fp64(be, k, ema):
    state4, sumsq, max_norm, gid, sched, want, bars, dist = ref_case(k)
    r = Recs(be, ema, hyper_words(max_norm=max_norm, sched=sched), step=k - 1.0)
    r.prepare(sumsq)
    gs = Tab(be.dev, fresh_gstate())
    gstate = scalars_call(be, r, Tab(be.dev, ghyper_words(REF_SPECS)), gs, len(REF_SPECS))
    e0 = _ema_start(REF_N) if ema else None
    got = groups_call(be, r, state4, e0, gid, gs, len(REF_SPECS))
    tag = "groups fp64 step %d ema %d" % (k, ema)
    print("%s: fp32 evaluation to fp64: p %.3e m %.3e v %.3e" % ((tag,) + tuple(dist)))
    vals = [record("%s %s" % (tag, name), rel(x, w), bar) for name, x, w, bar in zip("pmv", got, want, bars)]
    assert all(x <= b for x, b in zip(vals, bars)), (tag, vals, bars)
    frozen = (gid == 0) | (gid == 1)                       # the two groups at lr_scale 0
    assert same_bits(got[0][frozen], state4[0][frozen]), "%s: a parameter of a group at lr_scale 0 changed" % tag
    assert not bool((bits(got[1][frozen]) == bits(state4[2][frozen])).all()) and not bool((bits(got[2][frozen]) == bits(state4[3][frozen])).all()), \
        "%s: the moments of a group at lr_scale 0 did not move" % tag
    assert not bool((bits(got[0][~frozen]) == bits(state4[0][~frozen])).any())
    if ema:
        omd = float(r.wr.words()[A.W["EMA_OMD"]])
        A.ema_bound_ok(tag, got[3], e0, got[0], omd)


def run_scale0_special_values(be):
    """lr_scale 0: -0.0, +0.0, denormals and huge parameters keep their bits (fmaf(p, 1, -0))"""
    n = 8
    p0 = torch.tensor([-0.0, 0.0, 1e-45, -1e-40, 3e38, -3e38, 1.0, -2.5])
    _, g, m, v = _inputs(n)
    gid = torch.zeros(n, dtype=torch.uint8)
    r = Recs(be, 0, hyper_words(max_norm=1.0), step=6.0)
    r.prepare(4.0)
    gs = Tab(be.dev, fresh_gstate())
    scalars_call(be, r, Tab(be.dev, ghyper_words([(0.0, 0.3), (1.0, WD)])), gs, 2)
    got = groups_call(be, r, (p0, g, m, v), None, gid, gs, 2)
    assert same_bits(got[0], p0), (got[0], p0)
    assert not same_bits(got[1], m) and not same_bits(got[2], v)


# -------------------------------------------------------------------------------------------------------------------- 7. skip and hold
SKIP_CASES = [(s, v, e) for s in ("n3", "n1027", "big") for v in (1.0, 2.0) for e in (0, 1)]


def run_skip(be, size, skip_now, ema):
    """SKIP_NOW = 1 (skipped) and 2 (hold): neither launch writes -- p, m, v, ema and gstate keep their bits"""
    n, dev = SIZES[size], be.dev
    r = Recs(be, ema, hyper_words(max_norm=1.0), step=6.0)
    r.prepare(4.0)
    sw = r.sr.out.cpu().clone()
    sw[S["SKIP_NOW"]] = skip_now
    r.sr = Rec(dev, sw)
    gs0 = fresh_gstate()
    gs0[:3 * G_WORDS] = rn((3 * G_WORDS,), 9200, 1.0)
    gh, gs = Tab(dev, ghyper_words(SPECS3)), Tab(dev, gs0)
    assert be.call("optim_group_scalars", r.sr.out, gh.out, gs.out, 3) == 0, be.last_error()
    state4 = _inputs(n)
    pg, gd_, mg, vg = C._slabs(be, state4)
    eg = Guard(n, dev, start=A.seeded(n, 9400)) if ema else None
    mp = ByteGuard(make_map(n, 3), dev)
    assert be.call("adamw_groups", pg.out, gd_, mg.out, vg.out, eg.out if ema else None, mp.out, n, r.sr.out, r.window(), gs.out, 3) == 0, be.last_error()
    be.sync()
    assert gs.untouched() and gh.untouched(), "SKIP_NOW = %g: optim_group_scalars wrote" % skip_now
    assert pg.untouched() and mg.untouched() and vg.untouched() and (not ema or eg.untouched()), "SKIP_NOW = %g: adamw_groups wrote to a slab" % skip_now


# ------------------------------------------------------------------------------------------------------------------------ 8. rejects
def run_scalars_rejects(be):
    dev = be.dev
    r = Recs(be, 0, hyper_words(max_norm=1.0), step=6.0)
    sw = r.prepare(4.0)
    cases = [(i, 3, None) for i in range(3)] + [(None, g, None) for g in (0, -1, 17, 1 << 20)] + [(None, 3, s) for s in ("state", "ghyper", "gstate")]
    for drop, ngroups, shift in cases:
        sr = Rec(dev, sw, shift=1 if shift == "state" else 0)
        gh, gs = Tab(dev, ghyper_words(SPECS3), shift=1 if shift == "ghyper" else 0), Tab(dev, fresh_gstate(), shift=1 if shift == "gstate" else 0)
        args = [sr.out, gh.out, gs.out, ngroups]
        if drop is not None:
            args[drop] = None
        rc, msg = be.call("optim_group_scalars", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("optim_group_scalars"), (drop, ngroups, shift, rc, msg)
        assert sr.untouched() and gh.untouched() and gs.untouched(), (drop, ngroups, shift)


def run_groups_rejects(be):
    dev, n = be.dev, 1027
    state4, gid = _inputs(n), make_map(n, 3)
    r = Recs(be, 1, hyper_words(max_norm=1.0), step=6.0)
    sw = r.prepare(4.0)
    ww = r.wr.out.cpu().clone()
    gs0 = fresh_gstate()
    gs0[:3 * G_WORDS] = rn((3 * G_WORDS,), 9201, 1.0)
    # (argument to drop, n, ngroups, record to misalign, form); arguments: p g m v ema gid n state window gstate ngroups
    cases = [(i, n, 3, None, 1) for i in (0, 1, 2, 3, 5, 7, 9)] + [(i, n, 3, None, 0) for i in (0, 5, 9)]
    cases += [(4, n, 3, None, 1), (8, n, 3, None, 1)]                            # ema without window, window without ema
    cases += [(None, bad, 3, None, e) for bad in (0, -1) for e in (0, 1)] + [(None, n, g, None, e) for g in (0, -2, 17) for e in (0, 1)]
    cases += [(None, n, 3, s, 1) for s in ("state", "window", "gstate")] + [(None, n, 3, s, 0) for s in ("state", "gstate")]
    for drop, nn, ngroups, shift, ema in cases:
        sr, wr = Rec(dev, sw, shift=1 if shift == "state" else 0), Rec(dev, ww, shift=1 if shift == "window" else 0)
        gs = Tab(dev, gs0, shift=1 if shift == "gstate" else 0)
        pg, gd_, mg, vg = C._slabs(be, state4)
        eg, mp = Guard(n, dev, start=_ema_start(n)), ByteGuard(gid, dev)
        args = [pg.out, gd_, mg.out, vg.out, eg.out if ema else None, mp.out, nn, sr.out, wr.out if ema else None, gs.out, ngroups]
        if drop is not None:
            args[drop] = None
        rc, msg = be.call("adamw_groups", *args), be.last_error()
        be.sync()
        assert rc != 0 and msg.startswith("adamw_groups"), (drop, nn, ngroups, shift, ema, rc, msg)
        assert all(x.untouched() for x in (pg, mg, vg, eg, mp, sr, wr, gs)), (drop, nn, ngroups, shift, ema)


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
# mutation -> the cases (functions of this module with their arguments) that must fail under it
MUTATIONS = {
    "quad_takes_first_group": [("run_boundary", ("quad1", 0)), ("run_boundary", ("quad2", 1)), ("run_boundary", ("quad3", 0)), ("run_boundary", ("mid_quad", 0)),
                               ("run_sizes", ("n5", 0))],
    "decay_from_group0": [("run_sizes", ("n1027", 0)), ("run_boundary", ("k1024", 1)), ("run_fp64", (10, 0)), ("run_ngroups", (16, "mix", 0))],
    "scale_on_decay_only": [("run_scalars", ()), ("run_fp64", (1, 0)), ("run_fp64", (1000, 1)), ("run_scale0_special_values", ())],
    "moments_frozen_at_scale0": [("run_fp64", (1, 0)), ("run_fp64", (2, 1)), ("run_scale0_special_values", ())],
    "pad_in_last_group": [("run_pad_group", ())],
    "map_index_off_by_one": [("run_sizes", ("n3", 0)), ("run_sizes", ("big", 1)), ("run_boundary", ("last", 0)), ("run_boundary", ("k3072", 1)),
                             ("run_empty_group", (0,))],
}


def host_group_map(layout, group_of, numel, pad_group=0):
    gid = torch.full((numel,), pad_group, dtype=torch.uint8)
    for (off, n, _), g in zip(layout, group_of):
        gid[off:off + n] = g
    return gid


class GroupEmu(A.AccumEmu):
    """accum_cases.AccumEmu plus fp32 CPU emulations of the two entry points of include/vptr_hip_groups.h.  mutation: one of MUTATIONS."""

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        super().__init__(None)
        self.gmutation = mutation

    def group_map(self, layout, group_of, numel):
        return host_group_map(layout, group_of, numel, pad_group=max(group_of) if self.gmutation == "pad_in_last_group" else 0)

    def optim_group_scalars(self, state, ghyper, gstate, ngroups):
        if any(t is None for t in (state, ghyper, gstate)):
            return self._fail("optim_group_scalars: a pointer is NULL")
        if not 1 <= ngroups <= MAX_GROUPS:
            return self._fail("optim_group_scalars: ngroups is outside 1 .. 16")
        if state.data_ptr() % 64 or ghyper.data_ptr() % 64 or gstate.data_ptr() % 64:
            return self._fail("optim_group_scalars: a record is not 64-byte aligned")
        s, gh, gs = state.numpy(), ghyper.numpy(), gstate.numpy()
        if s[S["SKIP_NOW"]] != 0:
            return 0
        with np.errstate(all="ignore"):
            for g in range(ngroups):
                scale, wd = gh[g * G_WORDS], gh[g * G_WORDS + 1]
                lr = F(s[S["LR_NOW"]] * scale)
                gs[g * G_WORDS + GS["STEP_SIZE"]] = s[S["STEP_SIZE"]] if self.gmutation == "scale_on_decay_only" else F(s[S["STEP_SIZE"]] * scale)
                gs[g * G_WORDS + GS["DECAY"]] = C._fma(-lr, wd, F(1))
                gs[g * G_WORDS + GS["LR"]] = lr
        return 0

    def adamw_groups(self, p, g, m, v, ema, gid, n, state, window, gstate, ngroups):
        if n <= 0:
            return self._fail("adamw_groups: n must be positive")
        if any(t is None for t in (p, g, m, v, gid, state, gstate)):
            return self._fail("adamw_groups: a pointer is NULL")
        if (ema is None) != (window is None):
            return self._fail("adamw_groups: ema and window must both be present or both be NULL")
        if not 1 <= ngroups <= MAX_GROUPS:
            return self._fail("adamw_groups: ngroups is outside 1 .. 16")
        if state.data_ptr() % 64 or gstate.data_ptr() % 64 or (window is not None and window.data_ptr() % 64):
            return self._fail("adamw_groups: a record is not 64-byte aligned")
        s, gs = state.numpy(), gstate.numpy()
        if s[S["SKIP_NOW"]] != 0:
            return 0
        idx = gid.reshape(-1)[:n].numpy().astype(np.int64) & (MAX_GROUPS - 1)
        idx = np.where(idx < ngroups, idx, 0)
        if self.gmutation == "quad_takes_first_group":
            idx = idx[(np.arange(n) // 4) * 4]
        if self.gmutation == "map_index_off_by_one":
            idx = idx[np.minimum(np.arange(n) + 1, n - 1)]
        step_size, decay = gs[idx * G_WORDS + GS["STEP_SIZE"]], gs[(0 if self.gmutation == "decay_from_group0" else idx) * G_WORDS + GS["DECAY"]]
        pv, mv, vv = (t.reshape(-1)[:n].numpy() for t in (p, m, v))
        keep = (mv.copy(), vv.copy())
        scal = {k: s[S[k]] for k in C.SCALARS}
        scal["STEP_SIZE"], scal["DECAY"] = step_size, decay
        self._update(p, g, m, v, n, *(scal[k] for k in C.SCALARS))
        if self.gmutation == "moments_frozen_at_scale0":
            still = step_size == 0
            mv[still], vv[still] = keep[0][still], keep[1][still]
        if ema is not None:
            with np.errstate(all="ignore"):
                ev = ema.reshape(-1)[:n].numpy()
                ev[:] = C._fma(window.numpy()[A.W["EMA_OMD"]], pv - ev, ev)
        return 0


def all_cases():
    out = [("run_sizes", c) for c in SIZE_CASES] + [("run_shift", c) for c in SHIFT_CASES] + [("run_boundary", c) for c in BOUND_CASES]
    out += [("run_ngroups", c) for c in NGROUPS_CASES] + [("run_empty_group", (e,)) for e in (0, 1)] + [("run_byte_out_of_range", (e,)) for e in (0, 1)]
    out += [("run_pad_group", ())] + [("run_identity", c) for c in IDENT_CASES] + [("run_scalars", ())] + [("run_fp64", c) for c in REF_CASES]
    out += [("run_scale0_special_values", ())] + [("run_skip", c) for c in SKIP_CASES] + [("run_scalars_rejects", ()), ("run_groups_rejects", ())]
    return out


def case_id(c):
    return c[0][4:] + "".join("-%s" % a for a in c[1])
