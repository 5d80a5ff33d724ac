"""Case runner of tests/test_09h_recon_loss_gpu.py and tests/test_recon_loss_cpu.py: vptr_recon_loss_fwd / vptr_recon_loss_bwd
(include/vptr_hip_loss.h) called through the C ABI and compared with `vptr_amd.model.criterion`'s MSELoss, L1Loss and GDL on .double()
inputs, with autograd of g_mse * mse + g_l1 * l1 + g_gdl * gdl.

The runner talks to a BACKEND as tests/step_tail_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's
order without the trailing stream (tensors for pointers, None for NULL) and returns the return code.  The GPU file's backend hands the
pointers to the library; `ReconEmu` below is an fp32 CPU emulation of the two entry points written from the header, which
tests/test_recon_loss_cpu.py runs the same cases against -- and against named mutations of it, each of which must fail its listed cases.

Every output and the scratch are `Guard`s (step_tail_cases): NaN-filled, between NaN guard rows that must stay NaN; the scratch is sized
exactly as the header says and must come back finite everywhere.

Geometries [N, T, C, H, W] (one 6-D [N, T, TP, C, H, W]), the smallest that reach each hazard:
    2,3,3,17,5     plane -> t with wrap over N and planes_per_frame 3; a one-row last band
    1,1,1,2,2      the minimum size; T = 1
    2,5,1,33,4     one-row last band at H = 33
    5,4,15,5,3     300 planes: the final kernel's loop takes a second trip
    1,2,1,16,300   exactly one band; wide rows
    2,3,2,1,4,4    6-D: planes_per_frame = TP * C
Options: weights none / w_point only / w_gdl only / both with different values (temporal_weight_func(T) and a vector with a 0);
alpha 1, 2, 1.5, 3; upstream scalars unequal, each one NULL in turn, all NULL (dpred == 0).

Inputs are seeded: pred == gt on the first rows and two equal neighbours in the last row, so exact ties occur; for the seeds below
helpers.gdl_sign_disagreements is 0 and fp32 / fp64 agree on sign(pred - gt) everywhere (asserted on the CPU): no element is excluded.

Bars: alpha 1 and 2 -- values 1e-6 relative, dpred 2e-6 rel-L2 (the bars of the MSE + GDL kernels: the arithmetic is of the same
class).  alpha 1.5 and 3 (powf) -- POW_BAR_FACTOR = 5 times the distance to fp64 of an fp32 torch evaluation of the same criterion
classes on the same inputs (the ADAMW_BAR_FACTOR rule of tests/test_09d_step_tail_gpu.py), floored at the bars above."""
import functools

import numpy as np
import torch

from helpers import gdl_sign_disagreements, margin, rel
from step_tail_cases import Guard, rn, same_bits, scalar

TOL_VALUE = 1e-6
TOL_GRAD = 2e-6
POW_BAR_FACTOR = 5.0

# id -> (shape, seed)
GEOMS = {"2x3x3x17x5": ((2, 3, 3, 17, 5), 7100), "1x1x1x2x2": ((1, 1, 1, 2, 2), 7100), "2x5x1x33x4": ((2, 5, 1, 33, 4), 7100),
         "5x4x15x5x3": ((5, 4, 15, 5, 3), 7100), "1x2x1x16x300": ((1, 2, 1, 16, 300), 7100), "2x3x2x1x4x4": ((2, 3, 2, 1, 4, 4), 7100)}
GEOMS_5D = [k for k, (s, _) in GEOMS.items() if len(s) == 5]
WEIGHTS = ("none", "point", "gdl", "both")
ALPHAS = (1.0, 2.0, 1.5, 3.0)
# id -> (g_mse, g_l1, g_gdl); None = NULL
UPSTREAM = {"all": (0.7, 1.3, 1.9), "no_mse": (None, 1.3, 1.9), "no_l1": (0.7, None, 1.9), "no_gdl": (0.7, 1.3, None), "none": (None, None, None)}
# (planes, planes_per_frame, T, H, W, alpha) that both calls must refuse
REJECTS = [(4, 1, 2, 1, 4, 1.0), (4, 1, 2, 4, 1, 1.0), (4, 1, 0, 4, 4, 1.0), (4, 0, 2, 4, 4, 1.0), (4, 3, 1, 4, 4, 1.0), (4, 1, 3, 4, 4, 1.0),
           (0, 1, 1, 4, 4, 1.0), (4, 1, 2, 4, 4, 0.5), (4, 1, 2, 4, 4, 0.999), (4, 1, 2, 4, 4, float("nan")), (4, 1, 2, 4, 4, float("inf")),
           (4, 1, 2, 4, 4, -2.0)]


def geometry(geom):
    """(planes, planes_per_frame, T, H, W) of a GEOMS entry"""
    shape = GEOMS[geom][0]
    H, W = shape[-2:]
    ppf = int(np.prod(shape[2:-2]))
    return int(np.prod(shape[:-2])), ppf, shape[1], H, W


def scratch_floats(planes, H):
    return planes * ((H + 15) // 16) * 4


def record(name, value, bound):
    margin("recon_loss " + name, value, bound)
    print("%s: %.3e (bar %.3e)" % (name, value, bound))
    return value


@functools.lru_cache(maxsize=None)
def inputs(geom):
    """seeded pred, gt of the geometry's shape: pred == gt on the first rows of every plane (d = 0 and every sign argument of those
    pairs an exact 0) and two equal neighbours in the last row (pd == 0 next to gd != 0)"""
    shape, seed = GEOMS[geom]
    H = shape[-2]
    gt, pred = rn(shape, seed, 0.3), rn(shape, seed + 1, 0.3)
    ties = 1 if H < 4 else min(3, H // 2)
    pred[..., :ties, :] = gt[..., :ties, :]
    pred[..., -1, 0] = pred[..., -1, 1]
    return pred, gt


def exp_weights(T):
    from vptr_amd.model.criterion import temporal_weight_func
    return temporal_weight_func(T).float()


@functools.lru_cache(maxsize=None)
def weights(geom, mode):
    """(w_point, w_gdl) fp32 CPU vectors or None: w_point = temporal_weight_func(T) (T = 1: one value off 1), w_gdl a seeded vector of
    other values whose first entry is 0 when T > 1"""
    T = GEOMS[geom][0][1]
    wp = exp_weights(T) if T > 1 else torch.tensor([1.7])
    wg = (0.4 + rn((T,), 7300 + T).abs()).float()
    if T > 1:
        wg[0] = 0.0
    return (wp if mode in ("point", "both") else None), (wg if mode in ("gdl", "both") else None)


def criteria_eval(pred, gt, wp, wg, alpha, ups, dtype, crit=None):
    """MSELoss(wp)(gt, pred), L1Loss(wp)(gt, pred), GDL(alpha, wg)(gt, pred) of `crit` (vptr_amd.model.criterion) in `dtype` and autograd of
    g_mse * mse + g_l1 * l1 + g_gdl * gdl (None = 0): {"mse", "l1", "gdl": floats, "dpred": tensor of pred's shape}"""
    if crit is None:
        from vptr_amd.model import criterion as crit
    p, g = pred.to(dtype).clone().requires_grad_(True), gt.to(dtype)
    wp, wg = (None if w is None else w.to(dtype) for w in (wp, wg))
    a = int(alpha) if float(alpha) == int(alpha) else float(alpha)
    lm, ll, lg = crit.MSELoss(temporal_weight=wp)(g, p), crit.L1Loss(temporal_weight=wp)(g, p), crit.GDL(alpha=a, temporal_weight=wg)(g, p)
    gm, gl, gg = (0.0 if u is None else float(np.float32(u)) for u in ups)            # the device scalars are fp32
    (gm * lm + gl * ll + gg * lg).backward()
    return {"mse": float(lm.detach()), "l1": float(ll.detach()), "gdl": float(lg.detach()), "dpred": p.grad.detach()}


@functools.lru_cache(maxsize=64)
def reference(geom, mode, alpha, up):
    pred, gt = inputs(geom)
    return criteria_eval(pred, gt, *weights(geom, mode), alpha, UPSTREAM[up], torch.float64)


@functools.lru_cache(maxsize=None)
def bars(geom, mode, alpha, up):
    """(value bar per output, dpred bar) of a case"""
    if alpha in (1.0, 2.0):
        return {"mse": TOL_VALUE, "l1": TOL_VALUE, "gdl": TOL_VALUE}, TOL_GRAD
    pred, gt = inputs(geom)
    ref, f32 = reference(geom, mode, alpha, up), criteria_eval(pred, gt, *weights(geom, mode), alpha, UPSTREAM[up], torch.float32)
    vb = {k: max(TOL_VALUE, POW_BAR_FACTOR * abs(f32[k] - ref[k]) / abs(ref[k])) for k in ("mse", "l1", "gdl")}
    gb = TOL_GRAD if up == "none" else max(TOL_GRAD, POW_BAR_FACTOR * rel(f32["dpred"], ref["dpred"]))
    return vb, gb


def input_tie_counts(geom):
    """(GDL sign arguments on which fp32 and fp64 disagree, elements on which they disagree about sign(pred - gt), elements with pred == gt)"""
    pred, gt = inputs(geom)
    planes, _, _, H, W = geometry(geom)
    p3, g3 = pred.reshape(planes, H, W), gt.reshape(planes, H, W)
    d32, d64 = torch.sign(p3 - g3), torch.sign(p3.double() - g3.double())
    return gdl_sign_disagreements(p3, g3), int((d32.double() != d64).sum()), int((d32 == 0).sum())


def all_cases():
    return [(g, m, a) for g in GEOMS for m in WEIGHTS for a in ALPHAS]


def case_id(c):
    return "%s-%s-a%g" % c


def _dev_weights(geom, mode, dev):
    return tuple(None if w is None else w.to(dev) for w in weights(geom, mode))


def run_case(be, geom, mode, alpha):
    """one forward into NaN-filled guarded outputs and an exactly sized scratch, then one backward per UPSTREAM entry"""
    dev = be.dev
    planes, ppf, T, H, W = geometry(geom)
    pred, gt = inputs(geom)
    pd_, gd_ = pred.to(dev).reshape(-1), gt.to(dev).reshape(-1)
    wp, wg = _dev_weights(geom, mode, dev)
    tag = "%s %s alpha %g" % (geom, mode, alpha)
    scratch, out3 = Guard(scratch_floats(planes, H), dev), Guard(3, dev)
    assert be.call("recon_loss_fwd", pd_, gd_, wp, wg, scratch.out, out3.out, planes, ppf, T, H, W, alpha) == 0, tag
    be.sync()
    scratch.result()
    got = out3.result()
    ref = reference(geom, mode, alpha, "all")
    vb, _ = bars(geom, mode, alpha, "all")
    for i, k in enumerate(("mse", "l1", "gdl")):
        v = record("%s %s" % (tag, k), abs(float(got[i]) - ref[k]) / abs(ref[k]), vb[k])
        assert v < vb[k], (tag, k, v, vb[k])
    for up, ups in UPSTREAM.items():
        dpred = Guard(planes * H * W, dev)
        assert be.call("recon_loss_bwd", pd_, gd_, wp, wg, *(scalar(u, dev) for u in ups), dpred.out, planes, ppf, T, H, W, alpha) == 0, (tag, up)
        be.sync()
        d, want = dpred.result().view(pred.shape), reference(geom, mode, alpha, up)["dpred"]
        if up == "none":
            assert float(want.abs().max()) == 0.0 and float(d.abs().max()) == 0.0, (tag, up)
            continue
        gb = bars(geom, mode, alpha, up)[1]
        v = record("%s dpred %s" % (tag, up), rel(d, want), gb)
        assert v < gb, (tag, up, v, gb)
    for w, src in ((wp, weights(geom, mode)[0]), (wg, weights(geom, mode)[1])):
        assert w is None or torch.equal(w.cpu(), src), "%s: a call changed a weight vector" % tag


def run_rejects(be):
    """every documented reject, by both calls: non-zero return code, all guards and outputs still NaN"""
    dev = be.dev
    x, w = rn((64,), 7400).to(dev), torch.ones(4, device=dev)

    def outs():
        return Guard(64, dev), Guard(3, dev), Guard(64, dev)

    def refused(fwd_args, bwd_args, what):
        scratch, out3, dpred = outs()
        fa = [scratch.out if a == "scratch" else (out3.out if a == "out3" else a) for a in fwd_args]
        ba = [dpred.out if a == "dpred" else a for a in bwd_args]
        assert be.call("recon_loss_fwd", *fa) != 0, ("fwd", what)
        assert be.call("recon_loss_bwd", *ba) != 0, ("bwd", what)
        be.sync()
        assert scratch.untouched() and out3.untouched() and dpred.untouched(), what

    g = scalar(1.0, dev)
    for planes, ppf, T, H, W, alpha in REJECTS:
        refused((x, x, w, w, "scratch", "out3", planes, ppf, T, H, W, alpha), (x, x, w, w, g, g, g, "dpred", planes, ppf, T, H, W, alpha),
                (planes, ppf, T, H, W, alpha))
    geo = (4, 1, 2, 4, 4, 1.0)
    for i in (0, 1, 4, 5):                   # pred, gt, scratch, out3 NULL
        fa = [x, x, w, w, "scratch", "out3"]
        fa[i] = None
        scratch, out3, _ = outs()
        fa = [scratch.out if a == "scratch" else (out3.out if a == "out3" else a) for a in fa]
        assert be.call("recon_loss_fwd", *fa, *geo) != 0, i
        be.sync()
        assert scratch.untouched() and out3.untouched(), i
    for i in (0, 1, 7):                      # pred, gt, dpred NULL
        ba = [x, x, w, w, g, g, g, "dpred"]
        ba[i] = None
        dpred = Guard(64, dev)
        ba = [dpred.out if a == "dpred" else a for a in ba]
        assert be.call("recon_loss_bwd", *ba, *geo) != 0, i
        be.sync()
        assert dpred.untouched(), i


def run_bit_identity(be, geom):
    """the default settings against vptr_mse_gdl_fwd / _bwd on the same inputs: mse and gdl bit for bit, dpred torch.equal"""
    dev = be.dev
    planes, ppf, T, H, W = geometry(geom)
    pred, gt = inputs(geom)
    pd_, gd_ = pred.to(dev).reshape(-1), gt.to(dev).reshape(-1)
    gm, gg = scalar(0.7, dev), scalar(1.9, dev)
    s_old, mse, gdl, d_old = Guard(planes * ((H + 15) // 16) * 3, dev), Guard(1, dev), Guard(1, dev), Guard(planes * H * W, dev)
    assert be.call("mse_gdl_fwd", pd_, gd_, s_old.out, mse.out, gdl.out, planes, H, W) == 0
    assert be.call("mse_gdl_bwd", pd_, gd_, gm, gg, d_old.out, planes, H, W) == 0
    s_new, out3, d_new = Guard(scratch_floats(planes, H), dev), Guard(3, dev), Guard(planes * H * W, dev)
    assert be.call("recon_loss_fwd", pd_, gd_, None, None, s_new.out, out3.out, planes, ppf, T, H, W, 1.0) == 0
    assert be.call("recon_loss_bwd", pd_, gd_, None, None, gm, None, gg, d_new.out, planes, ppf, T, H, W, 1.0) == 0
    be.sync()
    got = out3.result()
    assert same_bits(got[0:1], mse.result()), (geom, "mse", float(got[0]), float(mse.result()))
    assert same_bits(got[2:3], gdl.result()), (geom, "gdl", float(got[2]), float(gdl.result()))
    assert torch.equal(d_new.result(), d_old.result()), (geom, "dpred")
    # the partial sums the two scratch layouts share
    old, new = s_old.result().view(-1, 3), s_new.result().view(-1, 4)
    assert same_bits(new[:, :3].contiguous(), old), (geom, "partials")


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
# mutation -> the cases (of all_cases()) that must fail under it
MUTATIONS = {
    # t = plane / planes_per_frame without % T: past the first sample the index leaves the vector (the emulation reads 1 there)
    "no_mod_T": [("2x3x3x17x5", "point", 1.0), ("2x3x3x17x5", "both", 2.0), ("2x5x1x33x4", "gdl", 1.0), ("5x4x15x5x3", "both", 1.5), ("2x3x2x1x4x4", "point", 3.0)],
    # the GDL weighted with w_point
    "gdl_uses_w_point": [("2x3x3x17x5", "point", 1.0), ("2x3x3x17x5", "gdl", 2.0), ("2x3x3x17x5", "both", 1.5), ("1x1x1x2x2", "both", 1.0), ("1x2x1x16x300", "gdl", 3.0)],
    # alpha * d^alpha for the gradient, which is alpha * d^(alpha - 1)
    "alpha_d_alpha": [("2x3x3x17x5", "none", 2.0), ("1x1x1x2x2", "none", 3.0), ("2x5x1x33x4", "both", 1.5), ("1x2x1x16x300", "point", 3.0), ("2x3x2x1x4x4", "gdl", 2.0)],
    # L1 gradient with sign(0) = 1
    "l1_sign0_is_1": [("2x3x3x17x5", "none", 1.0), ("1x1x1x2x2", "point", 2.0), ("5x4x15x5x3", "both", 1.5), ("2x3x2x1x4x4", "none", 3.0)],
    # the weighted means divided by the sum of the weights instead of the element count
    "mean_over_weight_sum": [("2x3x3x17x5", "point", 1.0), ("2x5x1x33x4", "gdl", 2.0), ("1x1x1x2x2", "both", 1.0), ("2x3x2x1x4x4", "both", 1.5)],
    # the final kernel's loop advancing by 512 partials: rows 256 .. 511 are never added
    "final_stride_512": [("5x4x15x5x3", "none", 1.0), ("5x4x15x5x3", "both", 2.0), ("5x4x15x5x3", "point", 1.5), ("5x4x15x5x3", "gdl", 3.0)],
    # planes_per_frame ignored (t = plane % T)
    "ppf_ignored": [("2x3x3x17x5", "point", 1.0), ("5x4x15x5x3", "gdl", 2.0), ("2x3x2x1x4x4", "both", 1.0)],
}


class ReconEmu:
    """fp32 CPU emulation of vptr_recon_loss_fwd / vptr_recon_loss_bwd from include/vptr_hip_loss.h: fp32 element arithmetic, fp32 band sums
    multiplied by the plane's weights into the scratch rows, the rows added in fp64 by 256 strided readers, the documented argument checks
    with a non-zero return.  mutation: one of MUTATIONS."""
    dev = "cpu"

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation

    def sync(self):
        pass

    def call(self, name, *a):
        return getattr(self, name)(*a)

    @staticmethod
    def _bad(ptrs, planes, ppf, T, H, W, alpha):
        alpha = float(np.float32(alpha))
        return (any(t is None for t in ptrs) or H < 2 or W < 2 or T < 1 or ppf < 1 or planes < 1 or planes % (ppf * T) != 0
                or not (alpha >= 1.0 and np.isfinite(alpha)))

    def _plane_weights(self, w, planes, ppf, T):
        """the weight of every plane, [planes] fp32"""
        if w is None:
            return torch.ones(planes)
        plane = torch.arange(planes)
        t = plane // ppf
        if self.mutation == "ppf_ignored":
            t = plane
        if self.mutation != "no_mod_T":
            t = t % T
        ext = torch.cat([w.float().reshape(-1), torch.ones(planes)])          # what an index past the vector reads here
        return ext[t]

    @staticmethod
    def _pairs(p, g):
        pdh, gdh = p[:, 1:, :] - p[:, :-1, :], g[:, 1:, :] - g[:, :-1, :]
        pdw, gdw = p[:, :, :-1] - p[:, :, 1:], g[:, :, :-1] - g[:, :, 1:]
        return pdh, gdh, pdw, gdw

    def recon_loss_fwd(self, pred, gt, w_point, w_gdl, scratch, out3, planes, ppf, T, H, W, alpha):
        if self._bad((pred, gt, scratch, out3), planes, ppf, T, H, W, alpha):
            return -1
        alpha = float(np.float32(alpha))
        p, g = pred.float().reshape(planes, H, W), gt.float().reshape(planes, H, W)
        pdh, gdh, pdw, gdw = self._pairs(p, g)
        d = p - g
        sq, ab, dh, dw = d * d, d.abs(), torch.zeros_like(p), torch.zeros_like(p)
        ah, aw = (gdh.abs() - pdh.abs()).abs(), (gdw.abs() - pdw.abs()).abs()
        dh[:, :-1, :] = ah if alpha == 1.0 else (ah * ah if alpha == 2.0 else ah.pow(alpha))      # the pair (y, y + 1) belongs to row y
        dw[:, :, :-1] = aw if alpha == 1.0 else (aw * aw if alpha == 2.0 else aw.pow(alpha))
        bands = -(-H // 16)
        wg_sel = w_point if self.mutation == "gdl_uses_w_point" else w_gdl
        wp, wg = self._plane_weights(w_point, planes, ppf, T), self._plane_weights(wg_sel, planes, ppf, T)
        rows = [torch.stack([t[:, b * 16: b * 16 + 16].sum((1, 2)) for b in range(bands)], 1) * wt[:, None]
                for t, wt in ((sq, wp), (dh, wg), (dw, wg), (ab, wp))]
        part = torch.stack(rows, 2).reshape(-1, 4)                                               # [planes * bands, 4] fp32
        assert part.dtype == torch.float32
        scratch.reshape(-1)[:part.numel()].copy_(part.reshape(-1))
        n, stride = part.shape[0], (512 if self.mutation == "final_stride_512" else 256)
        seen = torch.cat([torch.arange(t, n, stride) for t in range(min(256, n))])
        tot = part[seen].double().sum(0)
        den = [float(planes) * H * W, float(planes) * (H - 1) * W, float(planes) * H * (W - 1)]
        if self.mutation == "mean_over_weight_sum":
            sp, sg = float(wp.double().sum()) / planes, float(wg.double().sum()) / planes
            den = [den[0] * sp, den[1] * sg, den[2] * sg]
        out3.reshape(-1)[:3].copy_(torch.tensor([tot[0] / den[0], tot[3] / den[0], tot[1] / den[1] + tot[2] / den[2]], dtype=torch.float64).float())
        return 0

    def recon_loss_bwd(self, pred, gt, w_point, w_gdl, g_mse, g_l1, g_gdl, dpred, planes, ppf, T, H, W, alpha):
        if self._bad((pred, gt, dpred), planes, ppf, T, H, W, alpha):
            return -1
        alpha = float(np.float32(alpha))
        F = torch.float32
        p, g = pred.float().reshape(planes, H, W), gt.float().reshape(planes, H, W)
        gm, gl, gg = (torch.tensor(0.0 if u is None else float(u), dtype=F) for u in (g_mse, g_l1, g_gdl))
        wg_sel = w_point if self.mutation == "gdl_uses_w_point" else w_gdl
        wp, wg = self._plane_weights(w_point, planes, ppf, T)[:, None, None], self._plane_weights(wg_sel, planes, ppf, T)[:, None, None]
        pdh, gdh, pdw, gdw = self._pairs(p, g)

        def pair(pd, gd):
            u = gd.abs() - pd.abs()
            s, a = torch.sign(u) * torch.sign(pd), u.abs()
            if alpha == 1.0:
                return s
            if alpha == 2.0:
                return (2.0 * a * (a if self.mutation == "alpha_d_alpha" else 1.0)) * s
            e = alpha if self.mutation == "alpha_d_alpha" else alpha - 1.0
            return torch.where(a > 0, alpha * a.pow(e), torch.zeros_like(a)) * s
        sh, sw = pair(pdh, gdh), pair(pdw, gdw)
        th, tw = torch.zeros_like(p), torch.zeros_like(p)
        th[:, :-1, :] += sh                    # pd = p[y+1] - p[y]:  d | |gd| - |pd| | / d p[y] = +s, / d p[y+1] = -s
        th[:, 1:, :] -= sh
        tw[:, :, :-1] -= sw                    # pd = p[x] - p[x+1]:  / d p[x] = -s, / d p[x+1] = +s
        tw[:, :, 1:] += sw
        n = float(planes)
        inv = [torch.tensor(1.0 / v, dtype=F) for v in (n * H * W, n * (H - 1) * W, n * H * (W - 1))]
        if self.mutation == "mean_over_weight_sum":
            sp, sg = float(wp.double().sum()) / planes, float(wg.double().sum()) / planes
            inv = [inv[0] / sp, inv[1] / sg, inv[2] / sg]
        d = p - g
        sd = torch.sign(d)
        if self.mutation == "l1_sign0_is_1":
            sd = torch.where(d == 0, torch.ones_like(d), sd)
        cm = inv[0] * wp
        out = (gm + gm) * d * cm + (gg * wg) * (th * inv[1] + tw * inv[2]) + gl * sd * cm
        assert out.dtype == F
        dpred.reshape(-1)[:out.numel()].copy_(out.reshape(-1))
        return 0
