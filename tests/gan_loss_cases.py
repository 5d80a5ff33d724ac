"""Case runner of tests/test_09i_gan_loss_gpu.py and tests/test_gan_loss_cpu.py: vptr_gan_loss_fwd / vptr_gan_loss_bwd
(include/vptr_hip_gan.h) called through the C ABI and compared with `vptr_amd.model.criterion.GANLoss` on fp64 CPU tensors -- its labels
rounded to fp32 first, as the class's own buffers are -- with autograd of g_a * l_a + g_b * l_b + g_total * coef * (l_a + l_b).

The runner talks to a BACKEND as tests/recon_loss_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's
order without the trailing stream (tensors for pointers, None for NULL) and returns the return code.  The GPU file's backend hands the
pointers to the library; `GanEmu` below is an fp32 CPU emulation of the two entry points written from the header (fp32 element arithmetic,
fp32 sums of 2048-element chunks added in fp64), which tests/test_gan_loss_cpu.py runs the same cases against -- and against named
mutations of it, each of which must fail its listed cases.

Every output, scratch and dx buffer is a `Guard` (step_tail_cases): NaN-filled, between NaN guard rows that must stay NaN; the scratch is
sized exactly as the header says and must come back finite everywhere.

Geometries (na, nb, stride_a, stride_b, a_is_real, b_is_real); nb None: xb == NULL.  2048 is the workgroup's chunk:
    n1, n3                 the smallest tensors, alone
    n2047_2049             one below / one above the chunk, as a pair (na != nb)
    n2048_3, n2049_1       at / above the chunk, flags (real, fake) and (real, real)
    n2880_s4               K64's 80 x 6 x 6 logits, both tensors at stride 4
    n2880_2160_s4_1        stride 4 beside stride 1, na != nb
    n70001                 above KTH128's 62 720 (35 partials), beside a stride-4 tensor
    n70001_single_s4       the same alone at stride 4
A strided tensor lives in a buffer whose gaps hold NaN: one read of a gap poisons the sum or the gradient.
Inputs: seeded normal logits times the scale (0.5, 3, 20) with the planted values 0, -0, +-30, +-90, +-104 in front (the last n of them
when n < 8), where a naive log(1 + exp(-x)) gives inf and a naive e^x / (1 + e^x) gives NaN.
Settings (scale, (real_label, fake_label), coef): (0.5, (1, 0), 0.005), (3, (0.9, 0.1), 1), (20, (1, 0), 1), (20, (0.9, 0.1), 0.005).
Upstream scalars (g_a, g_b, g_total), None = NULL: five combinations; with all three present also dxa NULL and dxb NULL.

Bars (derived, not measured): with eps = 1e-6, the project's bar for the fused losses,
    forward   |out - ref| <= eps * mean(|x| (1 + |t|) + 1)  (vanilla),  eps * mean (x - t)^2  (lsgan),  eps * mean |x|  (wgangp);
              out3[2]: |coef| times the sum of the two bounds.  Each is the mean of the magnitudes an element's terms have: an fp32 sum of
              2048 terms in a tree over eight-term runs carries about sqrt(19) roundings of 2^-24 of that mean, a few 1e-7.
    gradient  per element 4 * 2^-24 * |g_eff| / n * u,  u = max(1, |x - t|) for lsgan and 1 otherwise, g_eff = g + coef g_total:
              one rounding for g_eff, up to two for the sigmoid (|sigma| <= 1), one for the product.
The emulation stays inside every bar (tests/test_gan_loss_cpu.py)."""
import functools

import numpy as np
import torch

from helpers import margin
from step_tail_cases import Guard, rn, same_bits, scalar

EPS_VALUE = 1e-6
GRAD_UNITS = 4.0
UNIT = 2.0 ** -24
CHUNK = 2048
NAN = float("nan")
MODES = {"vanilla": 0, "lsgan": 1, "wgangp": 2}
PLANTED = [0.0, -0.0, 30.0, -30.0, 90.0, -90.0, 104.0, -104.0]

# id -> (na, nb, stride_a, stride_b, a_is_real, b_is_real)
GEOMS = {
    "n1": (1, None, 1, 1, 1, 0),
    "n3": (3, None, 1, 1, 0, 0),
    "n2047_2049": (2047, 2049, 1, 1, 0, 1),
    "n2048_3": (2048, 3, 1, 1, 1, 0),
    "n2049_1": (2049, 1, 1, 1, 1, 1),
    "n2880_s4": (2880, 2880, 4, 4, 0, 1),
    "n2880_2160_s4_1": (2880, 2160, 4, 1, 0, 1),
    "n70001": (70001, 2880, 1, 4, 0, 1),
    "n70001_single_s4": (70001, None, 4, 1, 1, 0),
}
# id -> (scale, (real_label, fake_label), coef)
SETTINGS = {"s0.5": (0.5, (1.0, 0.0), 0.005), "s3_soft": (3.0, (0.9, 0.1), 1.0), "s20": (20.0, (1.0, 0.0), 1.0), "s20_soft": (20.0, (0.9, 0.1), 0.005)}
# id -> (g_a, g_b, g_total); None = NULL
UPSTREAM = {"total": (None, None, 1.0), "a": (1.0, None, None), "all": (1.3, 1.0, 1.3), "ab": (1.0, 1.3, None), "none": (None, None, None)}


def f32(v):
    return float(np.float32(v))


def all_cases():
    return [(m, g, s) for m in MODES for g in GEOMS for s in SETTINGS]


def case_id(c):
    return "%s-%s-%s" % c


def scratch_floats(na, nb):
    """the header's scratch size"""
    return -(-na // CHUNK) + (0 if nb is None else -(-nb // CHUNK))


def record(name, value, bound):
    margin("gan_loss " + name, value, bound)
    print("%s: %.3e (bar %.3e)" % (name, value, bound))
    return value


@functools.lru_cache(maxsize=None)
def logits(n, seed, scale):
    """n seeded fp32 logits with the planted values in front (the last n of them when n < 8)"""
    x = (rn((n,), seed, 1.0) * scale).float()
    p = torch.tensor(PLANTED[-n:] if n < len(PLANTED) else PLANTED)
    x[:p.numel()] = p
    return x


@functools.lru_cache(maxsize=None)
def inputs(geom, setting):
    """(xa, xb or None): the logical elements, fp32 on the CPU"""
    na, nb, *_ = GEOMS[geom]
    scale = SETTINGS[setting][0]
    return logits(na, 9100, scale), (None if nb is None else logits(nb, 9200, scale))


def strided(x, stride, dev):
    """a device buffer with x at the given element stride and NaN in the gaps"""
    if x is None:
        return None
    buf = torch.full((x.numel() * stride,), NAN)
    buf[::stride] = x
    return buf.to(dev)


def criterion_eval(mode, xa, a_real, xb, b_real, labels, coef, ups, crit=None):
    """GANLoss(mode, labels rounded to fp32) of `crit` (vptr_amd.model.criterion) on fp64 tensors and autograd of
    g_a * l_a + g_b * l_b + g_total * coef * (l_a + l_b) (None = 0): {"out": [l_a, l_b, total], "dxa", "dxb"}"""
    if crit is None:
        from vptr_amd.model import criterion as crit
    G = crit.GANLoss(mode, target_real_label=f32(labels[0]), target_fake_label=f32(labels[1])).double()
    a = xa.double().clone().requires_grad_(True)
    b = None if xb is None else xb.double().clone().requires_grad_(True)
    la = G(a, bool(a_real))
    lb = G(b, bool(b_real)) if b is not None else torch.zeros((), dtype=torch.float64)
    total = f32(coef) * (la + lb)
    ga, gb, gt = (0.0 if u is None else f32(u) for u in ups)
    (ga * la + gb * lb + gt * total).backward()
    return {"out": [float(la.detach()), float(lb.detach()), float(total.detach())], "dxa": a.grad.detach(), "dxb": None if b is None else b.grad.detach()}


@functools.lru_cache(maxsize=256)
def reference(mode, geom, setting, up):
    na, nb, sa, sb, ar, br = GEOMS[geom]
    _, labels, coef = SETTINGS[setting]
    xa, xb = inputs(geom, setting)
    return criterion_eval(mode, xa, ar, xb, br, labels, coef, UPSTREAM[up])


def value_bound(mode, x, t):
    """the forward bar of one tensor (see the module docstring); x fp32 logical elements, t the fp32 target"""
    if x is None:
        return 0.0
    x = x.double()
    if mode == "vanilla":
        return EPS_VALUE * float((x.abs() * (1.0 + abs(t)) + 1.0).mean())
    if mode == "lsgan":
        return EPS_VALUE * float(((x - t) ** 2).mean())
    return EPS_VALUE * float(x.abs().mean())


def grad_bound(mode, x, t, g_eff):
    """per-element gradient bar, a tensor of x's shape"""
    u = torch.clamp((x.double() - t).abs(), min=1.0) if mode == "lsgan" else torch.ones_like(x, dtype=torch.float64)
    return GRAD_UNITS * UNIT * abs(g_eff) / x.numel() * u


def targets(geom, setting):
    _, _, _, _, ar, br = GEOMS[geom]
    rl, fl = (f32(v) for v in SETTINGS[setting][1])
    return (rl if ar else fl), (rl if br else fl)


def run_case(be, mode, geom, setting):
    """one forward into NaN-filled guarded outputs and an exactly sized scratch, then one backward per UPSTREAM entry and, with all three
    scalars, one with dxa NULL and one with dxb NULL"""
    dev = be.dev
    na, nb, sa, sb, ar, br = GEOMS[geom]
    _, (rl, fl), coef = SETTINGS[setting]
    xa, xb = inputs(geom, setting)
    da, db = strided(xa, sa, dev), strided(xb, sb, dev)
    m = MODES[mode]
    tag = case_id((mode, geom, setting))
    nb_arg = 0 if nb is None else nb
    scratch, out3 = Guard(scratch_floats(na, nb), dev), Guard(3, dev)
    assert be.call("gan_loss_fwd", da, na, sa, ar, db, nb_arg, sb, br, m, rl, fl, coef, scratch.out, out3.out) == 0, tag
    be.sync()
    scratch.result()
    got = out3.result()
    ref = reference(mode, geom, setting, "all")["out"]
    ta, tb = targets(geom, setting)
    ba, bb = value_bound(mode, xa, ta), value_bound(mode, xb, tb)
    for i, (k, bound) in enumerate((("l_a", ba), ("l_b", bb), ("total", abs(f32(coef)) * (ba + bb)))):
        v = record("%s %s" % (tag, k), abs(float(got[i]) - ref[i]), bound)
        assert v <= bound, (tag, k, float(got[i]), ref[i], v, bound)
    if nb is None:
        assert float(got[1]) == 0.0, tag

    def backward(ups, want_a=True, want_b=True):
        ga = Guard(na, dev) if want_a else None
        gb = Guard(nb, dev) if (want_b and nb is not None) else None
        rc = be.call("gan_loss_bwd", da, na, sa, ar, None if ga is None else ga.out, db, nb_arg, sb, br, None if gb is None else gb.out, m, rl, fl,
                     coef, *(scalar(u, dev) for u in ups))
        assert rc == 0, (tag, ups)
        be.sync()
        return (None if ga is None else ga.result()), (None if gb is None else gb.result())

    full = None
    for up, ups in UPSTREAM.items():
        want = reference(mode, geom, setting, up)
        dxa, dxb = backward(ups)
        if up == "all":
            full = (dxa, dxb)
        g_t = 0.0 if ups[2] is None else f32(ups[2])
        for name, d, x, t, g, w in (("dxa", dxa, xa, ta, ups[0], want["dxa"]), ("dxb", dxb, xb, tb, ups[1], want["dxb"])):
            if d is None:
                continue
            g_eff = (0.0 if g is None else f32(g)) + f32(coef) * g_t
            if g_eff == 0.0:
                assert float(w.abs().max()) == 0.0 and float(d.abs().max()) == 0.0, (tag, up, name)
                continue
            bound = grad_bound(mode, x, t, g_eff)
            units = float(((d.double() - w).abs() / bound).max()) * GRAD_UNITS
            record("%s %s %s [units of 2^-24 |g_eff| u / n]" % (tag, name, up), units, GRAD_UNITS)
            assert units <= GRAD_UNITS, (tag, up, name, units)
    # a gradient that is not wanted: the other one is what the full call wrote
    only_b = backward(UPSTREAM["all"], want_a=False)
    only_a = backward(UPSTREAM["all"], want_b=False)
    assert only_b[0] is None and only_a[1] is None
    assert same_bits(only_a[0], full[0]), (tag, "dxb NULL")
    if nb is not None:
        assert same_bits(only_b[1], full[1]), (tag, "dxa NULL")
    for buf, x, s in ((da, xa, sa), (db, xb, sb)):
        assert buf is None or same_bits(buf.cpu()[::s], x), "%s: a call changed its input" % tag


# what both calls must refuse, as changes to a valid pair call: argument name -> value
REJECTS = [dict(xa=None), dict(na=0), dict(na=-5), dict(nb=0), dict(nb=-1), dict(stride_a=0), dict(stride_a=-4), dict(stride_b=0), dict(mode=-1),
           dict(mode=3), dict(real_label=NAN), dict(real_label=float("inf")), dict(fake_label=NAN), dict(fake_label=float("-inf")),
           dict(coef=NAN), dict(coef=float("inf"))]
REJECTS_FWD = [dict(scratch=None), dict(out3=None)]
REJECTS_BWD = [dict(xb=None, nb=0)]                                       # a dxb without an xb
FWD_ARGS = ("xa", "na", "stride_a", "a_is_real", "xb", "nb", "stride_b", "b_is_real", "mode", "real_label", "fake_label", "coef", "scratch", "out3")
BWD_ARGS = ("xa", "na", "stride_a", "a_is_real", "dxa", "xb", "nb", "stride_b", "b_is_real", "dxb", "mode", "real_label", "fake_label", "coef",
            "g_a", "g_b", "g_total")


def run_rejects(be):
    """every documented reject: non-zero return code, all guards and outputs still NaN; and what is NOT a reject"""
    dev = be.dev
    x, g = rn((64,), 9400).to(dev), scalar(1.0, dev)

    def attempt(which, change):
        scratch, out3, dxa, dxb = Guard(2, dev), Guard(3, dev), Guard(16, dev), Guard(16, dev)
        vals = dict(xa=x, na=16, stride_a=1, a_is_real=0, xb=x, nb=16, stride_b=2, b_is_real=1, mode=0, real_label=1.0, fake_label=0.0, coef=0.5,
                    scratch=scratch.out, out3=out3.out, dxa=dxa.out, dxb=dxb.out, g_a=g, g_b=g, g_total=g)
        vals.update(change)
        rc = be.call("gan_loss_" + which, *(vals[k] for k in (FWD_ARGS if which == "fwd" else BWD_ARGS)))
        be.sync()
        return rc, (scratch, out3, dxa, dxb)

    for change in REJECTS + REJECTS_FWD:
        rc, bufs = attempt("fwd", change)
        assert rc != 0, ("fwd", change)
        assert all(b.untouched() for b in bufs), ("fwd", change)
    for change in REJECTS + REJECTS_BWD:
        rc, bufs = attempt("bwd", change)
        assert rc != 0, ("bwd", change)
        assert all(b.untouched() for b in bufs), ("bwd", change)
    # accepted: nb and stride_b are ignored without an xb; no gradient wanted launches nothing
    rc, (scratch, out3, _, _) = attempt("fwd", dict(xb=None, nb=0, stride_b=0, scratch=Guard(1, dev).out))
    assert rc == 0 and float(out3.result()[1]) == 0.0
    rc, bufs = attempt("bwd", dict(dxa=None, dxb=None))
    assert rc == 0 and all(b.untouched() for b in bufs)


def run_twice_identical(be, mode, geom, setting):
    """two calls on the same inputs: every output bit for bit"""
    dev = be.dev
    na, nb, sa, sb, ar, br = GEOMS[geom]
    _, (rl, fl), coef = SETTINGS[setting]
    xa, xb = inputs(geom, setting)
    da, db = strided(xa, sa, dev), strided(xb, sb, dev)
    nb_arg = 0 if nb is None else nb
    gs = [scalar(u, dev) for u in UPSTREAM["all"]]
    seen = []
    for _ in range(2):
        scratch, out3, dxa, dxb = Guard(scratch_floats(na, nb), dev), Guard(3, dev), Guard(na, dev), Guard(nb_arg or 1, dev)
        assert be.call("gan_loss_fwd", da, na, sa, ar, db, nb_arg, sb, br, MODES[mode], rl, fl, coef, scratch.out, out3.out) == 0
        assert be.call("gan_loss_bwd", da, na, sa, ar, dxa.out, db, nb_arg, sb, br, None if nb is None else dxb.out, MODES[mode], rl, fl, coef, *gs) == 0
        be.sync()
        seen.append((scratch.result(), out3.result(), dxa.result()) + (() if nb is None else (dxb.result(),)))
    assert all(same_bits(p, q) for p, q in zip(*seen)), (mode, geom, setting)


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
_PAIRS = ["n2047_2049", "n2048_3", "n2880_s4", "n70001"]
# mutation -> the cases (of all_cases()) that must fail under it
MUTATIONS = {
    # log(1 + exp(-x)): inf at the planted -90 and -104
    "naive_softplus": [("vanilla", g, s) for g in ("n1", "n3", "n2047_2049", "n70001") for s in ("s0.5", "s20_soft")],
    # e^x / (1 + e^x) everywhere: NaN at the planted +90 and +104
    "naive_sigmoid": [("vanilla", g, s) for g in ("n3", "n2048_3", "n2880_s4", "n70001_single_s4") for s in ("s3_soft", "s20")],
    # the sums and the gradients not divided by n
    "missing_inv_n": [(m, g, "s3_soft") for m in MODES for g in ("n3", "n2049_1", "n2880_2160_s4_1", "n70001")],
    # real_label where fake_label belongs and the reverse (wgangp has no labels)
    "labels_swapped": [(m, g, s) for m in ("vanilla", "lsgan") for g in ("n1", "n2047_2049", "n2880_s4") for s in ("s0.5", "s3_soft")],
    # element i read at x[i]: the gaps of a strided tensor hold NaN
    "stride_ignored": [(m, g, "s0.5") for m in MODES for g in ("n2880_s4", "n2880_2160_s4_1", "n70001", "n70001_single_s4")],
    # out3[2] = coef * l_a + l_b, and the same slip in the gradient of xb
    "coef_on_one_term": [(m, g, s) for m in MODES for g in _PAIRS for s in ("s0.5", "s20_soft")],
    # +x for a real target
    "wgangp_sign_flipped": [("wgangp", g, s) for g in ("n1", "n2049_1", "n2047_2049", "n70001_single_s4") for s in ("s0.5", "s20")],
    # the gradient formed from g_a / g_b alone
    "g_total_dropped": [(m, g, s) for m in MODES for g in ("n3", "n2048_3", "n2880_s4") for s in ("s0.5", "s3_soft")],
}


class GanEmu:
    """fp32 CPU emulation of vptr_gan_loss_fwd / vptr_gan_loss_bwd from include/vptr_hip_gan.h: fp32 element arithmetic, fp32 sums of
    2048-element chunks into the scratch, the partials of a tensor added in fp64 and divided by n; the gradient's scale (g + coef g_total)
    rounded to fp32 once and multiplied by 1 / n and dl/dx in fp64; the documented argument checks with a non-zero return.
    mutation: one of MUTATIONS."""
    dev = "cpu"

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation

    def sync(self):
        pass

    def call(self, name, *a):
        return getattr(self, name)(*a)

    @staticmethod
    def _bad(xa, na, sa, xb, nb, sb, mode, rl, fl, coef):
        fin = all(np.isfinite(np.float32(v)) for v in (rl, fl, coef))
        return xa is None or na < 1 or sa < 1 or (xb is not None and (nb < 1 or sb < 1)) or mode not in (0, 1, 2) or not fin

    def _elems(self, x, n, stride):
        s = 1 if self.mutation == "stride_ignored" else stride
        return x.reshape(-1)[: (n - 1) * s + 1: s].float()

    def _sel(self, mode, is_real, rl, fl):
        if self.mutation == "labels_swapped":
            rl, fl = fl, rl
        if mode == 2:
            real_sign = 1.0 if self.mutation == "wgangp_sign_flipped" else -1.0
            return torch.tensor(real_sign if is_real else 1.0)
        return torch.tensor(f32(rl if is_real else fl))

    def _loss(self, mode, x, sel):
        if mode == 0:
            if self.mutation == "naive_softplus":
                return x - x * sel + torch.log(1.0 + torch.exp(-x))
            return torch.clamp(x, min=0) - x * sel + torch.log1p(torch.exp(-x.abs()))
        if mode == 1:
            return (x - sel) * (x - sel)
        return sel * x

    def _dloss(self, mode, x, sel):
        """fp64 dl/dx from fp32 pieces"""
        if mode == 0:
            if self.mutation == "naive_sigmoid":
                e = torch.exp(x)
                s = e / (1.0 + e)
            else:
                e = torch.exp(-x.abs())
                s = torch.where(x >= 0, torch.ones_like(e), e) / (1.0 + e)
            assert s.dtype == torch.float32
            return s.double() - sel.double()
        if mode == 1:
            return 2.0 * (x.double() - sel.double())
        return sel.double().expand_as(x)

    def _mean(self, mode, x, n, sel):
        """-> (fp32 chunk partials, the fp64 mean)"""
        el = self._loss(mode, x, sel)
        assert el.dtype == torch.float32
        part = torch.stack([c.sum() for c in el.split(CHUNK)])
        tot = part.double().sum()
        return part, (tot if self.mutation == "missing_inv_n" else tot / n)

    def gan_loss_fwd(self, xa, na, sa, a_real, xb, nb, sb, b_real, mode, rl, fl, coef, scratch, out3):
        if self._bad(xa, na, sa, xb, nb, sb, mode, rl, fl, coef) or scratch is None or out3 is None:
            return -1
        pa, la = self._mean(mode, self._elems(xa, na, sa), na, self._sel(mode, a_real, rl, fl))
        parts, lb = [pa], torch.zeros((), dtype=torch.float64)
        if xb is not None:
            pb, lb = self._mean(mode, self._elems(xb, nb, sb), nb, self._sel(mode, b_real, rl, fl))
            parts.append(pb)
        parts = torch.cat(parts)
        scratch.reshape(-1)[:parts.numel()].copy_(parts)
        la, lb, c = la.float(), lb.float(), torch.tensor(f32(coef))
        total = (c * la + lb) if self.mutation == "coef_on_one_term" else c * (la + lb)
        out3.reshape(-1)[:3].copy_(torch.stack([la, lb, total]))
        return 0

    def gan_loss_bwd(self, xa, na, sa, a_real, dxa, xb, nb, sb, b_real, dxb, mode, rl, fl, coef, g_a, g_b, g_total):
        if self._bad(xa, na, sa, xb, nb, sb, mode, rl, fl, coef) or (xb is None and dxb is not None):
            return -1
        gt = 0.0 if (g_total is None or self.mutation == "g_total_dropped") else float(g_total)
        for x, n, s, is_real, dx, g, second in ((xa, na, sa, a_real, dxa, g_a, False), (xb, nb, sb, b_real, dxb, g_b, True)):
            if dx is None:
                continue
            c = 1.0 if (second and self.mutation == "coef_on_one_term") else f32(coef)
            g_eff = f32((0.0 if g is None else float(g)) + c * gt)                 # fmaf: the fp64 sum of an exact product, rounded once
            scale = g_eff if self.mutation == "missing_inv_n" else g_eff * (1.0 / n)
            d = (scale * self._dloss(mode, self._elems(x, n, s), self._sel(mode, is_real, rl, fl))).float()
            dx.reshape(-1)[:n].copy_(d)
        return 0
