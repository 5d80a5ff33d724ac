"""Case runner of tests/test_09d_step_tail_gpu.py: the tail of every train step called through the C ABI (include/vptr_hip.h) -- the fused losses
vptr_mse_gdl_fwd / _bwd and vptr_nce_fwd / _bwd, the optimizer's vptr_sumsq / vptr_sumsq_ws / vptr_adamw, and the counter-based RNG behind
vptr_dropout / vptr_droppath_scales -- compared with plain torch fp64 (helpers.mse_gdl_ref / nce_ref / adamw_ref, an fp64 sum) and, for the RNG,
bit for bit with the integer emulation helpers.hash3_emu.

The runner talks to a BACKEND, as tests/convffn_fwd_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's order
without the trailing stream (tensors for pointers, None for NULL) and returns the call's return code.  The GPU file's backend hands the
pointers to the library; `EmuBackend` below is a CPU emulation written from the header (closed forms where the references use autograd), which
tests/test_cpu.py runs the same cases against: a wrong argument order, layout, reference or bar of a CASE fails there, without a GPU.

Every output and every scratch buffer is a `Guard`: the payload inside a NaN-filled allocation with 16 guard floats on both sides, which must
come back NaN; a scratch is sized exactly as the header says and must come back finite everywhere.  Accumulated destinations (vptr_sumsq) start
from a non-zero value.  A rejected call returns non-zero and leaves every output as it was.

Bars: MSE / GDL values 1e-6 relative, their gradient 2e-6 rel-L2 (tests/test_00_ops_gpu.py) and per element of the last band 1e-6 of the sum of
the magnitudes of the element's terms (about six fp32 roundings of 2^-24 each); NCE value 2e-6, gradients 1e-5 (test_00), the scratch sections
inv / S / rlse / clse 2e-6 rel-L2 (the loss is their function and carries that bar); sums of squares 1e-6 relative; AdamW p, m, v: five times
the rel-L2 distance to fp64 of an fp32 evaluation of the same formulas whose bias corrections do not cancel (helpers.adamw_f32_emulation) on
the case's inputs; RNG: torch.equal.

Not covered: the `idx >> 32` term of vptr_hash3 needs an element index of 2^32 or more, a tensor of 16 GB; it stays untested on the device (the
emulation's own term is exercised on the CPU)."""
import functools

import numpy as np
import torch

from helpers import (adamw_f32_emulation, adamw_ref, drop_scale_emu, droppath_emu, f32, gdl_sign_disagreements, margin, mse_gdl_ref, nce_f32_emulation, nce_ref, rel,
                     step_tail_class)
from oracle import fill

NAN = float("nan")
GUARD = 16                       # floats on both sides of a payload
TOL_LOSS = 1e-6                  # MSE / GDL values
TOL_LOSS_GRAD = 2e-6             # their gradient, rel-L2
TOL_LOSS_ELEM = 1e-6             # per element of the last band, of the summed magnitudes of its terms
TOL_NCE = 2e-6                   # NCE value; the scratch sections
TOL_NCE_GRAD = 1e-5
TOL_SUMSQ = 1e-6
ADAMW_BAR_FACTOR = 5.0


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def record(name, value, bound):
    """print and log (helpers.margin) one measured distance and its bar"""
    margin("step_tail " + name, value, bound)
    print("%s: %.3e (bar %.3e)" % (name, value, bound))
    return value


class Guard:
    """n floats inside a NaN-filled allocation with GUARD floats on both sides; shift = 1 puts the payload one float past a 16-byte boundary"""

    def __init__(self, n, dev, start=None, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), NAN, device=dev)
        self.out = self.buf[self.lo: self.lo + n]
        assert self.out.data_ptr() % 16 == 4 * shift
        self.start = None if start is None else start.detach().reshape(-1).float().cpu().clone()
        if start is not None:
            self.out.copy_(self.start)

    def guards_intact(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:self.lo]).all()) and bool(torch.isnan(b[self.lo + self.n:]).all())

    def untouched(self):
        """the payload is what it was before the call (NaN, or the start values bit for bit) and the guards are intact"""
        got = self.out.cpu()
        return self.guards_intact() and (bool(torch.isnan(got).all()) if self.start is None else same_bits(got, self.start))

    def result(self):
        """guards intact, payload finite everywhere; returns the payload on the CPU"""
        assert self.guards_intact(), "write outside the payload"
        got = self.out.cpu().clone()
        assert bool(torch.isfinite(got).all()), "payload not written everywhere"
        return got


def shifted(t, dev):
    """a device copy of the flat fp32 tensor t that starts one float past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=dev)
    v = buf[1: 1 + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def scalar(value, dev):
    return None if value is None else torch.tensor([value], dtype=torch.float32, device=dev)


def seed_tensor(value, dev):
    """the 64-bit seed word as the device holds it (one int64 read as uint64)"""
    value &= 0xFFFFFFFFFFFFFFFF
    return torch.tensor([value - (1 << 64) if value >> 63 else value], dtype=torch.int64, device=dev)


def close(got, want, tol):
    return abs(float(got) - float(want)) <= tol * abs(float(want))


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
class EmuBackend:
    """CPU emulation of the entry points from include/vptr_hip.h in fp64 on the fp32 inputs, outputs rounded to fp32, float arguments rounded
    to fp32 as the ABI passes them, the documented argument checks with a non-zero return code.  The losses and their gradients are closed
    forms (the references differentiate the oracle's losses by autograd), AdamW is the bias-corrected-moments form of the paper (the reference
    uses torch's step-size form)."""
    dev = "cpu"

    def sync(self):
        pass

    def call(self, name, *a):
        return getattr(self, name)(*a)

    # -- MSE + GDL
    @staticmethod
    def _pairs(p, g):
        pdh, gdh = p[:, 1:, :] - p[:, :-1, :], g[:, 1:, :] - g[:, :-1, :]
        pdw, gdw = p[:, :, :-1] - p[:, :, 1:], g[:, :, :-1] - g[:, :, 1:]
        return pdh, gdh, pdw, gdw

    def mse_gdl_fwd(self, pred, gt, scratch, mse_out, gdl_out, planes, H, W):
        if any(t is None for t in (pred, gt, scratch, mse_out, gdl_out)) or planes <= 0 or H < 2 or W < 2:
            return -1
        p, g = pred.double().reshape(planes, H, W), gt.double().reshape(planes, H, W)
        pdh, gdh, pdw, gdw = self._pairs(p, g)
        sq, dh, dw = (p - g) ** 2, torch.zeros_like(p), torch.zeros_like(p)
        dh[:, :-1, :] = (gdh.abs() - pdh.abs()).abs()              # the pair (y, y + 1) belongs to row y, the pair (x, x + 1) to column x
        dw[:, :, :-1] = (gdw.abs() - pdw.abs()).abs()
        bands = -(-H // 16)
        part = torch.stack([torch.stack([t[:, b * 16: b * 16 + 16].sum((1, 2)) for b in range(bands)], 1) for t in (sq, dh, dw)], 2)
        scratch.reshape(-1)[:planes * bands * 3].copy_(part.reshape(-1).float())
        tot = part.float().double().sum((0, 1))
        mse_out.fill_(float(tot[0] / (planes * H * W)))
        gdl_out.fill_(float(tot[1] / (planes * (H - 1) * W) + tot[2] / (planes * H * (W - 1))))
        return 0

    def mse_gdl_bwd(self, pred, gt, g_mse, g_gdl, dpred, planes, H, W):
        if any(t is None for t in (pred, gt, dpred)) or planes <= 0 or H < 2 or W < 2:
            return -1
        p, g = pred.double().reshape(planes, H, W), gt.double().reshape(planes, H, W)
        gm, gg = (0.0 if g_mse is None else float(g_mse)), (0.0 if g_gdl is None else float(g_gdl))
        pdh, gdh, pdw, gdw = self._pairs(p, g)
        sh, sw = torch.sign(gdh.abs() - pdh.abs()) * torch.sign(pdh), torch.sign(gdw.abs() - pdw.abs()) * torch.sign(pdw)
        th, tw = torch.zeros_like(p), torch.zeros_like(p)
        th[:, :-1, :] += sh                    # pd = p[y+1] - p[y]:  d | |gd| - |pd| | / d p[y] = +s, / d p[y+1] = -s
        th[:, 1:, :] -= sh
        tw[:, :, :-1] -= sw                    # pd = p[x] - p[x+1]:  / d p[x] = -s, / d p[x+1] = +s
        tw[:, :, 1:] += sw
        d = gm * 2.0 * (p - g) / (planes * H * W) + gg * (th / (planes * (H - 1) * W) + tw / (planes * H * (W - 1)))
        dpred.reshape(-1)[:d.numel()].copy_(d.reshape(-1).float())
        return 0

    # -- BiPatchNCE
    def nce_fwd(self, g, p, scratch, loss_out, frames, L, C, tau):
        if any(t is None for t in (g, p, scratch, loss_out)) or frames <= 0 or L <= 0 or C <= 0 or tau <= 0:
            return -1
        tau, R = f32(tau), frames * L
        gd, pd = g.double().reshape(R, C), p.double().reshape(R, C)
        inv = 1.0 / torch.cat([(gd * gd).sum(1).sqrt(), (pd * pd).sum(1).sqrt()]).clamp_min(1e-12)
        gh, ph = (gd * inv[:R, None]).view(frames, L, C), (pd * inv[R:, None]).view(frames, L, C)
        S = torch.einsum("fic,fjc->fij", gh, ph) / tau
        S = S.float().double()                                   # nce_stats_kernel reads the scores the scores kernel stored
        rlse, clse = torch.logsumexp(S, 2), torch.logsumexp(S, 1)
        part = (rlse + clse - 2.0 * torch.diagonal(S, dim1=1, dim2=2)).sum(1)
        scratch.reshape(-1)[:R * (4 + L) + frames].copy_(torch.cat([inv, S.reshape(-1), rlse.reshape(-1), clse.reshape(-1), part]).float())
        loss_out.fill_(float(part.sum() * 0.5 / R))
        return 0

    def nce_bwd(self, g, p, scratch, gout, dg, dp, frames, L, C, tau):
        if any(t is None for t in (g, p, scratch, dg, dp)) or frames <= 0 or L <= 0 or C <= 0 or tau <= 0:
            return -1
        if C > 640 or C % 4 or any(t.data_ptr() % 16 for t in (g, p, dg, dp)):
            return -1
        tau, R = f32(tau), frames * L
        go = 1.0 if gout is None else float(gout)
        sc = scratch.double().reshape(-1)
        inv, S = sc[:2 * R], sc[2 * R: 2 * R + R * L].view(frames, L, L)
        rlse, clse = sc[2 * R + R * L: 3 * R + R * L].view(frames, L), sc[3 * R + R * L: 4 * R + R * L].view(frames, L)
        gd, pd = g.double().reshape(R, C), p.double().reshape(R, C)
        gh, ph = (gd * inv[:R, None]).view(frames, L, C), (pd * inv[R:, None]).view(frames, L, C)
        eye, c = torch.eye(L, dtype=torch.float64), 0.5 / R
        A, B = c * (torch.exp(S - rlse[:, :, None]) - eye), c * (torch.exp(S - clse[:, None, :]) - eye)
        dgh = (torch.einsum("fij,fjc->fic", A, ph) + torch.diagonal(B, dim1=1, dim2=2)[:, :, None] * ph) * (go / tau)
        dph = (torch.einsum("fij,fic->fjc", B, gh) + torch.diagonal(A, dim1=1, dim2=2)[:, :, None] * gh) * (go / tau)
        for dst, x, xh, dxh, iv in ((dg, gd, gh.reshape(R, C), dgh.reshape(R, C), inv[:R]), (dp, pd, ph.reshape(R, C), dph.reshape(R, C), inv[R:])):
            dot = (xh * dxh).sum(1, keepdim=True)
            dot = torch.where(iv[:, None] >= 1e12, torch.zeros_like(dot), dot)       # the clamp cuts the norm's gradient
            dst.reshape(-1)[:R * C].copy_(((dxh - xh * dot) * iv[:, None]).reshape(-1).float())
        return 0

    # -- optimizer
    def sumsq(self, g, n, sumsq_dev):
        if n <= 0 or sumsq_dev is None:
            return -1
        x = g.reshape(-1)[:n].double()
        sumsq_dev += float((x * x).sum())
        return 0

    def sumsq_ws(self, g, n, sumsq_dev, ws, nws):
        if n <= 0 or sumsq_dev is None or ws is None or nws < 1 or nws > 65536:
            return -1
        x = g.reshape(-1)[:n].double()
        part = torch.zeros(nws, dtype=torch.float64).index_add_(0, (torch.arange(n) // 256) % nws, x * x)     # workgroup b: strides of nws * 256
        ws.reshape(-1)[:nws].copy_(part.float())
        sumsq_dev.fill_(float(part.float().double().sum()))
        return 0

    def adamw(self, p, g, m, v, n, lr, b1, b2, eps, wd, step_dev, sumsq_dev, max_norm, grad_scale):
        if n <= 0 or any(t is None for t in (p, g, m, v, step_dev)):
            return -1
        lr, b1, b2, eps, wd, max_norm, grad_scale = (f32(x) for x in (lr, b1, b2, eps, wd, max_norm, grad_scale))
        k = float(step_dev)
        gd = g.reshape(-1)[:n].double() * grad_scale
        if sumsq_dev is not None:
            gd = gd * min(1.0, max_norm / (float(sumsq_dev) ** 0.5 * grad_scale + 1e-6))
        pv, mv, vv = p.reshape(-1)[:n], m.reshape(-1)[:n], v.reshape(-1)[:n]
        md, vd = b1 * mv.double() + (1.0 - b1) * gd, b2 * vv.double() + (1.0 - b2) * gd * gd
        mhat, vhat = md / (1.0 - b1 ** k), vd / (1.0 - b2 ** k)
        # torch adds eps to sqrt(v) / sqrt(bc2), not to sqrt(v_hat) -- the same number
        pd = pv.double() * (1.0 - lr * wd) - lr * mhat / (vhat.sqrt() + eps)
        pv.copy_(pd.float())
        mv.copy_(md.float())
        vv.copy_(vd.float())
        return 0

    # -- RNG
    def dropout(self, x, y, n, p, seed, site):
        if n <= 0 or seed is None or not 0.0 < p < 1.0:
            return -1
        y.reshape(-1)[:n].copy_(x.reshape(-1)[:n] * drop_scale_emu(int(seed[0]), site, torch.arange(n), p))
        return 0

    def droppath_scales(self, keep, out, nreq, maxcount, seed, site0):
        if any(t is None for t in (keep, out, seed)) or nreq <= 0 or maxcount <= 0:
            return -1
        out.reshape(-1)[:nreq * maxcount].copy_(droppath_emu(keep[:nreq], maxcount, int(seed[0]), site0).reshape(-1))
        return 0


# ------------------------------------------------------------------------------------- 1. vptr_mse_gdl_fwd / vptr_mse_gdl_bwd
# (planes, H, W) -> seed of the inputs.  What each geometry reaches (helpers.step_tail_class, asserted in tests/test_cpu.py):
#   (300, 5, 3)    300 partials: a second trip of mse_gdl_final_kernel's loop
#   (2, 17, 9)     two bands, the last of one row
#   (1, 2, 2)      the minimum: one vertical and one horizontal pair per column / row
#   (2, 33, 300)   W above the workgroup: a band is 4800 elements (19 trips), three bands, the last of one row
#   (7, 16, 16)    exactly one band of exactly 256 elements
#   (40, 64, 64)   160 partials, the bench step's count
# For these seeds gdl_sign_disagreements is 0 (test_cpu.py asserts it): no element is excluded.
MSE_GEOMS = {(300, 5, 3): 2000, (2, 17, 9): 2000, (1, 2, 2): 2000, (2, 33, 300): 2000, (7, 16, 16): 2000, (40, 64, 64): 2000}
MSE_VARIANTS = {"both": (0.7, 1.9), "no_mse": (None, 1.9), "no_gdl": (0.7, None), "neither": (None, None)}
MSE_REJECTS = [(2, 1, 4), (2, 4, 1), (0, 4, 4)]


def mse_tie_rows(H):
    return 1 if H < 4 else min(3, H // 2)


@functools.lru_cache(maxsize=None)
def mse_inputs(geom):
    """seeded pred, gt [planes, H, W]: pred == gt on the first rows (every sign argument of those pairs is an exact 0) and two equal neighbours
    in the last row (pd == 0 next to gd != 0)"""
    seed = MSE_GEOMS[geom]
    gt, pred = rn(geom, seed, 0.3), rn(geom, seed + 1, 0.3)
    pred[:, :mse_tie_rows(geom[1]), :] = gt[:, :mse_tie_rows(geom[1]), :]
    pred[:, -1, 0] = pred[:, -1, 1]
    return pred, gt


@functools.lru_cache(maxsize=8)
def _mse_ref(geom, variant):
    pred, gt = mse_inputs(geom)
    return mse_gdl_ref(pred, gt, *(None if w is None else f32(w) for w in MSE_VARIANTS[variant]))      # the device scalars are fp32


def run_mse_gdl(be, geom, variant):
    planes, H, W = geom
    cls, dev = step_tail_class("mse_gdl", planes=planes, H=H, W=W), be.dev
    pred, gt = mse_inputs(geom)
    ref = _mse_ref(geom, variant)
    gm, gg = MSE_VARIANTS[variant]
    tag = "mse_gdl %dx%dx%d %s" % (geom + (variant,))
    pd_, gd_ = pred.to(dev), gt.to(dev)
    scratch, mse, gdl, dpred = Guard(cls["scratch"], dev), Guard(1, dev), Guard(1, dev), Guard(planes * H * W, dev)
    assert be.call("mse_gdl_fwd", pd_, gd_, scratch.out, mse.out, gdl.out, planes, H, W) == 0, tag
    assert be.call("mse_gdl_bwd", pd_, gd_, scalar(gm, dev), scalar(gg, dev), dpred.out, planes, H, W) == 0, tag
    be.sync()
    scratch.result()
    vm = record(tag + " mse", abs(float(mse.result()) - ref["mse"]) / ref["mse"], TOL_LOSS)
    vg = record(tag + " gdl", abs(float(gdl.result()) - ref["gdl"]) / ref["gdl"], TOL_LOSS)
    assert vm < TOL_LOSS and vg < TOL_LOSS, (tag, vm, vg)
    got, want = dpred.result().view(planes, H, W), ref["dpred"]
    if variant == "neither":
        assert float(want.abs().max()) == 0.0 and float(got.abs().max()) == 0.0, tag
        return
    v = record(tag + " dpred", rel(got, want), TOL_LOSS_GRAD)
    assert v < TOL_LOSS_GRAD, (tag, v)
    # the last band's rows element by element, against the summed magnitudes of an element's terms
    y0 = 16 * (cls["bands"] - 1)
    n = float(planes)
    mag = abs(gm or 0.0) * 2.0 * (pred.double() - gt.double()).abs() / (n * H * W) + abs(gg or 0.0) * (2.0 / (n * (H - 1) * W) + 2.0 / (n * H * (W - 1)))
    ratio = ((got.double() - want).abs() / (TOL_LOSS_ELEM * mag + 1e-300))[:, y0:, :]
    worst = record(tag + " dpred last band per element / bound", float(ratio.max()), 1.0)
    assert worst <= 1.0, (tag, worst)


def run_mse_gdl_rejects(be):
    """H = 1, W = 1 (no pair to take a difference of) and planes = 0: non-zero return code, nothing written"""
    dev = be.dev
    x = rn((8,), 1).to(dev)
    for planes, H, W in MSE_REJECTS:
        assert step_tail_class("mse_gdl", planes=planes, H=H, W=W) == {"kernel": "reject"}
        scratch, mse, gdl, dpred = Guard(8, dev), Guard(1, dev), Guard(1, dev), Guard(8, dev)
        assert be.call("mse_gdl_fwd", x, x, scratch.out, mse.out, gdl.out, planes, H, W) != 0
        assert be.call("mse_gdl_bwd", x, x, scalar(1.0, dev), scalar(1.0, dev), dpred.out, planes, H, W) != 0
        be.sync()
        assert scratch.untouched() and mse.untouched() and gdl.untouched() and dpred.untouched(), (planes, H, W)


# ------------------------------------------------------------------------------------------------ 2. vptr_nce_fwd / vptr_nce_bwd
# channels at (frames, L) = (2, 35): every NV class of nce_bwd_kernel (4: C <= 64, 16: <= 256, 34: <= 544, 40: <= 640), both sides of every
# boundary, the limit, widths that are no multiple of 16 (the c < C guard of nce_scores_kernel); L = 35: one 64-row block with 29 dead rows, a
# partial third 16-token chunk
NCE_CHANNELS = (8, 20, 64, 68, 256, 260, 544, 548, 640)
NCE_NV = {8: 4, 20: 4, 64: 4, 68: 16, 256: 16, 260: 34, 544: 34, 548: 40, 640: 40}
# (frames, L) at C = 68 and 548: one token; exactly one block; a second block of 16 live rows = one whole chunk (L = 80: five chunks);
# a third block of 2 live rows with a partial chunk; four full blocks; 300 frames = 300 partials for nce_final_kernel
NCE_GEOMS = ((1, 1), (3, 64), (2, 80), (1, 130), (2, 256), (300, 4))
NCE_TAUS = (1.0, 0.07)
NCE_GOUT = 1.3


def nce_cases():
    out = [(2, 35, C) for C in NCE_CHANNELS] + [(f, L, C) for C in (68, 548) for f, L in NCE_GEOMS]
    return [(f, L, C, tau) for f, L, C in out for tau in NCE_TAUS]


@functools.lru_cache(maxsize=4)
def nce_inputs(frames, L, C):
    """g, p [frames * L, C] as tests/test_00_ops_gpu.py draws them; with four tokens or more, token 1 of g and token 2 of p are all zero
    (the eps clamp of the normalisation)"""
    R = frames * L
    seed = 3000 + 7 * C + 13 * L + frames
    g = rn((R, C), seed)
    p = rn((R, C), seed + 1) + 0.5 * g
    if R >= 4:
        g[1], p[2] = 0.0, 0.0
    return g, p


@functools.lru_cache(maxsize=4)
def _nce_ref(frames, L, C, tau, gout):
    g, p = nce_inputs(frames, L, C)
    return nce_ref(g, p, frames, L, f32(tau), f32(gout))                  # as the ABI's float / the device scalar hold them


def _nce_rows(frames, L):
    """(rows of g, rows of p) whose own token is not a zero token, and the rows of the last 64-row block of every frame"""
    R = frames * L
    keep_g, keep_p = torch.ones(R, dtype=torch.bool), torch.ones(R, dtype=torch.bool)
    if R >= 4:
        keep_g[1], keep_p[2] = False, False          # d/dx of x / max(|x|, 1e-12) is 1e12 * dxh: compare the other rows (as test_00 does)
    return keep_g, keep_p, (torch.arange(R) % L) >= 64 * (-(-L // 64) - 1)


def nce_emulation_distances(frames, L, C, tau, gout):
    """what fp32 storage and arithmetic alone cost against fp64 for one case (helpers.nce_f32_emulation: the kernels' operation order with
    libm's exp / log): relative distance of the loss, rel-L2 of dg / dp over the compared rows.  tests/test_cpu.py asserts that it stays inside
    test_00's bars for every case, i.e. that the bars are reachable in fp32; the bars themselves do not depend on it"""
    g, p = nce_inputs(frames, L, C)
    ref = _nce_ref(frames, L, C, tau, gout)
    loss, dg, dp = nce_f32_emulation(g, p, frames, L, f32(tau), f32(gout))
    keep_g, keep_p, _ = _nce_rows(frames, L)
    if L == 1:
        return {"loss": 0.0}
    return {"loss": abs(loss - ref["loss"]) / abs(ref["loss"]), "dg": rel(dg[keep_g], ref["dg"][keep_g]), "dp": rel(dp[keep_p], ref["dp"][keep_p])}


def _nce_fwd_check(be, frames, L, C, tau, tag):
    """the forward into an exactly sized NaN scratch; loss and the four scratch sections against fp64; returns the device tensors"""
    dev, R = be.dev, frames * L
    cls = step_tail_class("nce", frames=frames, L=L, C=C)
    g, p = nce_inputs(frames, L, C)
    ref = _nce_ref(frames, L, C, tau, 1.0)
    gd_, pd_ = g.to(dev), p.to(dev)
    scratch, loss = Guard(cls["scratch"], dev), Guard(1, dev)
    assert be.call("nce_fwd", gd_, pd_, scratch.out, loss.out, frames, L, C, tau) == 0, tag
    be.sync()
    sc = scratch.result()
    # L = 1: the loss is lse(S) - S = 0 exactly; its error is measured against the score instead
    den = abs(ref["loss"]) if L > 1 else float(ref["S"].abs().max())
    v = record(tag + " loss", abs(float(loss.result()) - ref["loss"]) / den, TOL_NCE)
    assert v < TOL_NCE, (tag, v)
    live = torch.ones(2 * R, dtype=torch.bool)
    if R >= 4:
        live[1], live[R + 2] = False, False            # the zero tokens' 1e12 would be all of the norm
    sections = {"inv": sc[:2 * R][live], "S": sc[2 * R: 2 * R + R * L], "rlse": sc[2 * R + R * L: 3 * R + R * L], "clse": sc[3 * R + R * L: 4 * R + R * L]}
    for name, got in sections.items():
        v = record("%s %s" % (tag, name), rel(got, ref[name][live] if name == "inv" else ref[name]), TOL_NCE)
        assert v < TOL_NCE, (tag, name, v)
    return gd_, pd_, scratch


def run_nce(be, frames, L, C, tau):
    """forward (loss, scratch sections), then the backward with gout = 1.3 and with gout = NULL from the same scratch: dg, dp over the rows whose
    own token is not the zero token, and over the rows of the last 64-row block of every frame on their own"""
    dev, R = be.dev, frames * L
    cls = step_tail_class("nce", frames=frames, L=L, C=C)
    tag = "nce %dx%dx%d tau %g" % (frames, L, C, tau)
    gd_, pd_, scratch = _nce_fwd_check(be, frames, L, C, tau, tag)
    before = scratch.buf.cpu()
    keep_g, keep_p, last = _nce_rows(frames, L)
    assert int(last.sum()) == frames * (64 - cls["dead_rows"])
    for gout in (NCE_GOUT, None):
        ref = _nce_ref(frames, L, C, tau, 1.0 if gout is None else gout)
        dg, dp = Guard(R * C, dev), Guard(R * C, dev)
        assert be.call("nce_bwd", gd_, pd_, scratch.out, scalar(gout, dev), dg.out, dp.out, frames, L, C, tau) == 0, tag
        be.sync()
        for name, got, want, keep in (("dg", dg.result().view(R, C), ref["dg"], keep_g), ("dp", dp.result().view(R, C), ref["dp"], keep_p)):
            t = "%s gout %s %s" % (tag, "NULL" if gout is None else "%g" % gout, name)
            if L == 1:          # one class: both cross-entropies are constant, the gradient is zero analytically
                assert float(want.abs().max()) < 1e-10 and float(got.abs().max()) < 1e-10, t
                continue
            v, vl = record(t, rel(got[keep], want[keep]), TOL_NCE_GRAD), record(t + " last block", rel(got[keep & last], want[keep & last]), TOL_NCE_GRAD)
            assert v < TOL_NCE_GRAD and vl < TOL_NCE_GRAD, (t, v, vl)
    assert torch.equal(bits(scratch.buf), bits(before)), "%s: the backward wrote into the forward's scratch" % tag


def run_nce_c6(be):
    """C = 6 (C % 4 != 0): the forward against fp64; the backward refuses it and writes nothing"""
    frames, L, C, dev = 2, 35, 6, be.dev
    assert step_tail_class("nce", frames=frames, L=L, C=C)["nv"] == "reject"
    for tau in NCE_TAUS:
        gd_, pd_, scratch = _nce_fwd_check(be, frames, L, C, tau, "nce 2x35x6 tau %g" % tau)
        dg, dp = Guard(frames * L * C, dev), Guard(frames * L * C, dev)
        assert be.call("nce_bwd", gd_, pd_, scratch.out, None, dg.out, dp.out, frames, L, C, tau) != 0
        be.sync()
        assert dg.untouched() and dp.untouched()


def run_nce_bwd_rejects(be):
    """C = 644 (above the 640 of the widest instantiation) and a g or dg that is not 16-byte aligned: non-zero return code, nothing written"""
    frames, L, dev = 2, 35, be.dev
    R = frames * L
    for C, which in ((644, None), (68, "g"), (68, "dg")):
        cls = step_tail_class("nce", frames=frames, L=L, C=C)
        assert (cls["nv"] == "reject") == (C == 644)
        g, p = rn((R, C), 3900), rn((R, C), 3901)
        gd_ = shifted(g, dev) if which == "g" else g.to(dev)
        scratch = torch.zeros(cls["scratch"], device=dev)
        dg, dp = Guard(R * C, dev, shift=1 if which == "dg" else 0), Guard(R * C, dev)
        assert be.call("nce_bwd", gd_, p.to(dev), scratch, None, dg.out, dp.out, frames, L, C, 1.0) != 0, (C, which)
        be.sync()
        assert dg.untouched() and dp.untouched(), (C, which)


# ------------------------------------------------------------------------------------------------ 3. vptr_sumsq / vptr_sumsq_ws
# 10 489 762 floats (42 MB): 256 workgroups of 1024 threads, stride 262 144 float4 -- two trips of the 4-deep unrolled loop, two full
# single-float4 trips, a partial one for the first 1000 threads, a scalar tail of two floats
SUMSQ_BIG = 4 * (2097152 + 524288 + 1000) + 2
SUMSQ_SIZES = (3, 1023, 1024, 10007, SUMSQ_BIG)
SUMSQ_WS = (1, 1024, 65536)


@functools.lru_cache(maxsize=2)
def sumsq_inputs(n):
    """n + 1 seeded floats: the aligned case reads [0, n), the unaligned one [1, n + 1)"""
    return rn((n + 1,), 4000 + n % 997)


def run_sumsq(be, n, aligned):
    """*sumsq_dev starts at a non-zero value of the sum's own size and must come back as that value plus the fp64 sum of squares"""
    dev = be.dev
    x = sumsq_inputs(n)
    xd = x.to(dev)
    view = xd[0:n] if aligned else xd[1:n + 1]
    assert view.data_ptr() % 16 == (0 if aligned else 4)
    start = f32(0.5 * n + 0.125)
    want = start + float((view.cpu().double() ** 2).sum())
    acc = Guard(1, dev, start=torch.tensor([start]))
    assert be.call("sumsq", view, n, acc.out) == 0
    be.sync()
    v = record("sumsq n %d %s" % (n, "aligned" if aligned else "one float in"), abs(float(acc.result()) - want) / want, TOL_SUMSQ)
    assert v < TOL_SUMSQ, (n, aligned, v)


def run_sumsq_ws(be, nws):
    """the fixed-order variant at the large n: the workspace starts as NaN and is overwritten everywhere, *sumsq_dev is overwritten (no
    accumulation), two calls agree bit for bit"""
    dev, n = be.dev, SUMSQ_BIG
    xd = sumsq_inputs(n).to(dev)[0:n]
    want = float((xd.cpu().double() ** 2).sum())
    outs = []
    for _ in range(2):
        ws, acc = Guard(nws, dev), Guard(1, dev)
        assert be.call("sumsq_ws", xd, n, acc.out, ws.out, nws) == 0
        be.sync()
        part, got = ws.result(), acc.result()
        vp = rel(part.double().sum(), want)
        assert vp < TOL_SUMSQ, (nws, "partials", vp)
        outs.append((part, got))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "sumsq_ws nws %d: two calls differ" % nws
    v = record("sumsq_ws n %d nws %d" % (n, nws), abs(float(outs[0][1]) - want) / want, TOL_SUMSQ)
    assert v < TOL_SUMSQ, (nws, v)


def run_sumsq_rejects(be):
    """vptr_sumsq_ws with nws = 0 and nws = 65537, n = 0 for both: non-zero return code, nothing written"""
    dev = be.dev
    xd = rn((64,), 4100).to(dev)
    for n, nws in ((64, 0), (64, 65537), (0, 4)):
        ws, acc = Guard(4, dev), Guard(1, dev, start=torch.tensor([2.5]))
        assert be.call("sumsq_ws", xd, n, acc.out, ws.out, nws) != 0, (n, nws)
        be.sync()
        assert ws.untouched() and acc.untouched(), (n, nws)
    acc = Guard(1, dev, start=torch.tensor([2.5]))
    assert be.call("sumsq", xd, 0, acc.out) != 0
    be.sync()
    assert acc.untouched()


# ------------------------------------------------------------------------------------------------------------------ 4. vptr_adamw
# 4 195 507 floats: 4096 workgroups (the cap) x 256 threads cover 1 048 576 float4, so 300 threads take a second grid-stride trip, then a
# 3-element scalar tail; with one pointer a float past a 16-byte boundary n4 = 0 and the scalar loop takes five trips
ADAMW_BIG = 4 * (4096 * 256) + 4 * 300 + 3
ADAMW_LAUNCH = {"big": (ADAMW_BIG, None), "big_p": (ADAMW_BIG, "p"), "big_g": (ADAMW_BIG, "g"), "big_m": (ADAMW_BIG, "m"), "big_v": (ADAMW_BIG, "v"),
                "n1": (1, None), "n3": (3, None), "n4": (4, None), "n1027": (1027, None)}
ADAMW_N = 4099                      # the clip and precision cases: 1024 float4 on 5 workgroups and a 3-element tail
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
# id -> (max_norm or None for sumsq_dev = NULL, grad_scale).  |g| = 0.3 sqrt(4099) = 19.2: "active" clips at a tenth of it; with grad_scale
# 0.25 the scaled norm is 4.8: clipped at 0.48, and NOT clipped at 10 although the unscaled norm is above 10 (the scale applies first)
ADAMW_CLIP = {"no_sumsq": (None, 1.0), "active": (1.9, 1.0), "inactive": (50.0, 1.0), "gs_active": (0.48, 0.25), "gs_inactive": (10.0, 0.25)}
ADAMW_WD = (0.0, 0.01)
ADAMW_STEPS = (1, 2, 3, 5, 10, 1000, 100000)
ADAMW_BETAS = ((0.9, 0.999), (0.5, 0.9))


@functools.lru_cache(maxsize=3)
def adamw_inputs(n, k, b1, b2, p_scale=2e-3):
    """a state as k - 1 steps leave it: g ~ 0.3 N(0, 1), m ~ (1 - b1^(k-1)) 0.2 N(0, 1), v ~ (1 - b2^(k-1)) 0.09 (0.5 + U), p of the size of
    two updates (so that the stored p resolves the update)"""
    seed = 5000 + (n % 1009) + 17 * (k % 1013)
    g, m = rn((n,), seed, 0.3), rn((n,), seed + 1, 0.2) * (1.0 - b1 ** (k - 1))
    v = (0.5 + fill.rand_input((n,), seed + 2)) * 0.09 * (1.0 - b2 ** (k - 1))
    return rn((n,), seed + 3, p_scale), g, m.float(), v.float()


def clip_coef_f32(sumsq, max_norm, grad_scale):
    """the coefficient adamw_kernel multiplies the raw gradient by, in fp32"""
    F = np.float32
    coef = F(grad_scale)
    if sumsq is not None:
        coef = coef * min(F(1), F(max_norm) / (np.sqrt(F(sumsq)) * F(grad_scale) + F(1e-6)))
    return F(coef)


def adamw_bars(state, k, hyper, sumsq, max_norm, grad_scale):
    """(p, m, v) bars: ADAMW_BAR_FACTOR x the rel-L2 distance of helpers.adamw_f32_emulation to adamw_ref on this state, and those distances"""
    p, g, m, v = state
    want = adamw_ref(p, g, m, v, k, sumsq=sumsq, max_norm=1.0 if max_norm is None else max_norm, grad_scale=grad_scale, **hyper)
    emu = adamw_f32_emulation(p, g, m, v, k, coef=clip_coef_f32(sumsq, max_norm, grad_scale), **hyper)
    dist = [rel(e, w) if float(w.abs().max()) > 0 else 0.0 for e, w in zip(emu, want)]
    return [ADAMW_BAR_FACTOR * d for d in dist], dist, want


def _adamw_call(be, state, k, hyper, sumsq, max_norm, grad_scale, shift=None):
    dev = be.dev
    p, g, m, v = state
    n = p.numel()
    pg, mg, vg = (Guard(n, dev, start=t, shift=1 if shift == s else 0) for s, t in (("p", p), ("m", m), ("v", v)))
    gd_ = shifted(g, dev) if shift == "g" else g.to(dev)
    step, ss = scalar(float(k), dev), scalar(sumsq, dev)
    rc = be.call("adamw", pg.out, gd_, mg.out, vg.out, n, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"], step, ss,
                 1.0 if max_norm is None else max_norm, grad_scale)
    assert rc == 0, rc
    be.sync()
    assert float(step.cpu()) == float(k) and (ss is None or float(ss.cpu()) == f32(sumsq)), "adamw changed step_dev or sumsq_dev"
    assert torch.equal(gd_.cpu(), g), "adamw changed the gradient"
    return pg.result(), mg.result(), vg.result()


def _adamw_check(tag, got, want, bars):
    """p, m, v separately against fp64 at their bars; an all-zero reference asks for exact zeros"""
    vals = []
    for name, a, w, bar in zip("pmv", got, want, bars):
        if float(w.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, (tag, name)
            vals.append(0.0)
            continue
        vals.append(record("%s %s" % (tag, name), rel(a, w), bar))
    assert all(v <= b for v, b in zip(vals, bars)), (tag, vals, bars)
    return vals


def _sumsq_of(g):
    return f32(float((g.double() ** 2).sum()))


def _bar_state(n, k, b1, b2, p_scale=2e-3):
    """the state the bars are measured on: the case's own from 1027 elements on, the 1027-element one below (a rel-L2 over a handful of
    elements is no measure of an rms rounding error)"""
    return adamw_inputs(max(n, 1027), k, b1, b2, p_scale)


def run_adamw_launch(be, case):
    """step 7 from a supplied state, clip active (max_norm a third of the norm), weight decay 0.01"""
    n, shift = ADAMW_LAUNCH[case]
    cls = step_tail_class("adamw", n=n, aligned=shift is None)
    k, state = 7, adamw_inputs(n, 7, HYPER["b1"], HYPER["b2"])
    sumsq = _sumsq_of(state[1])
    max_norm = f32(sumsq ** 0.5 / 3.0)
    bs = _bar_state(n, k, HYPER["b1"], HYPER["b2"])
    bars, _, want = adamw_bars(bs, k, HYPER, _sumsq_of(bs[1]), f32(_sumsq_of(bs[1]) ** 0.5 / 3.0), 1.0)
    if n < 1027:
        want = adamw_ref(*state, k, sumsq=sumsq, max_norm=max_norm, **HYPER)
    got = _adamw_call(be, state, k, HYPER, sumsq, max_norm, 1.0, shift)
    tag = "adamw %s" % case
    _adamw_check(tag, got, want, bars)
    if cls["vec_trips"] > 1:                # the elements of the second grid-stride trip and the scalar tail on their own
        first = cls["blocks"] * 256 * 4
        _adamw_check(tag + " second trip", [t[first:] for t in got], [t[first:] for t in want], bars)


def run_adamw_paths_equal(be):
    """the float4 path and the all-scalar path on identical values: bit-identical p, m, v (the source comment promises it)"""
    k, state = 7, adamw_inputs(ADAMW_BIG, 7, HYPER["b1"], HYPER["b2"])
    sumsq = _sumsq_of(state[1])
    a = _adamw_call(be, state, k, HYPER, sumsq, f32(sumsq ** 0.5 / 3.0), 1.0, None)
    b = _adamw_call(be, state, k, HYPER, sumsq, f32(sumsq ** 0.5 / 3.0), 1.0, "p")
    for name, x, y in zip("pmv", a, b):
        assert torch.equal(x, y), "adamw: %s differs between the float4 and the scalar path" % name


def run_adamw_clip(be, case, wd):
    """the clip folded into the step against clip_grad_norm_ on the scaled gradients + AdamW in fp64"""
    max_norm, gs = ADAMW_CLIP[case]
    k, hyper = 4, dict(HYPER, wd=wd)
    state = adamw_inputs(ADAMW_N, k, hyper["b1"], hyper["b2"])
    sumsq = None if max_norm is None else _sumsq_of(state[1])
    if max_norm is not None:
        norm = sumsq ** 0.5 * gs                       # of the scaled gradients
        assert (norm < max_norm) if "inactive" in case else (norm > 9.0 * max_norm), (case, norm)
        assert case != "gs_inactive" or sumsq ** 0.5 > max_norm
    bars, _, want = adamw_bars(state, k, hyper, sumsq, max_norm, gs)
    got = _adamw_call(be, state, k, hyper, sumsq, max_norm, gs)
    _adamw_check("adamw clip %s wd %g" % (case, wd), got, want, bars)


def run_adamw_zero_grad(be):
    """g == 0 and v == 0 everywhere, m tiny: v stays exactly 0, the denominator is eps alone, the update lr / bc1 * m / eps"""
    k = 4
    p, g, m, v = adamw_inputs(ADAMW_N, k, HYPER["b1"], HYPER["b2"])
    state = (p, torch.zeros_like(g), m * 1e-8, torch.zeros_like(v))
    bars, _, want = adamw_bars(state, k, HYPER, None, None, 1.0)
    got = _adamw_call(be, state, k, HYPER, None, None, 1.0)
    _adamw_check("adamw zero gradient", got, want, bars)


def run_adamw_precision(be, k, betas):
    """p0 = 0: the stored p is minus the update at full fp32 resolution.  One step from the state of step k - 1; the update, m and v against
    fp64 with the hyper-parameters as the ABI hands them over; the distance to fp64 with the double hyper-parameters is reported"""
    hyper = dict(HYPER, b1=betas[0], b2=betas[1])
    p, g, m, v = adamw_inputs(ADAMW_N, k, betas[0], betas[1])
    state = (torch.zeros_like(p), g, m, v)
    bars, dist, want = adamw_bars(state, k, hyper, None, None, 1.0)
    tag = "adamw update step %d betas %g/%g" % (k, betas[0], betas[1])
    print("%s: fp32 emulation to fp64: p %.3e m %.3e v %.3e" % ((tag,) + tuple(dist)))
    got = _adamw_call(be, state, k, hyper, None, None, 1.0)
    want_double = adamw_ref(*state, k, abi_hyper=False, **hyper)
    print("%s: update against fp64 with double hyper-parameters (not asserted): %.3e" % (tag, rel(got[0], want_double[0])))
    _adamw_check(tag, got, want, bars)


# --------------------------------------------------------------------------------- 5. vptr_dropout / vptr_droppath_scales bit for bit
DROP_SIZES = (1, 255, 100003)
DROP_PS = (0.1, 0.5, 0.999)
DROP_SEEDS = (0x9A3C5E7F12345678, 0x9A3C5E7F12345679, 0x1A3C5E7F12345678)       # 1st / 2nd: low word only; 1st / 3rd: high word only; 2nd / 3rd: both
DROP_SITES = (0, 1, 0xFFFFFFFF)
DROPPATH_COUNTS = (1, 257, 20000)
DROPPATH_KEEP = (0.9, 0.5, 0.75)


def run_dropout(be, n):
    """y == x * (0 or 1 / (1 - p)) with the mask of helpers.drop_scale_emu, for every p x seed x site"""
    dev = be.dev
    x = rn((n,), 6000 + n % 991) + 0.1
    xd = x.to(dev)
    for p in DROP_PS:
        for seed in DROP_SEEDS:
            sd = seed_tensor(seed, dev)
            for site in DROP_SITES:
                y = Guard(n, dev)
                assert be.call("dropout", xd, y.out, n, p, sd, site) == 0
                be.sync()
                want = x * drop_scale_emu(seed, site, torch.arange(n), p)
                assert torch.equal(y.result(), want), "dropout n %d p %g seed %#x site %#x" % (n, p, seed, site)
                assert int(sd.cpu()) & 0xFFFFFFFFFFFFFFFF == seed


def run_droppath(be, maxcount):
    """out[r][k] == floor(keep[r] + (h >> 8) / 2^24) / keep[r] in fp32, h = hash3(seed, site0 + r, k); keep = 1 gives all ones"""
    dev, nreq = be.dev, 3
    for keep in (DROPPATH_KEEP, (1.0, 1.0, 1.0)):
        kt = torch.tensor(keep, dtype=torch.float32)
        for seed in DROP_SEEDS[:2]:
            sd = seed_tensor(seed, dev)
            for site0 in (0, 7):
                out = Guard(nreq * maxcount, dev)
                assert be.call("droppath_scales", kt.to(dev), out.out, nreq, maxcount, sd, site0) == 0
                be.sync()
                got = out.result().view(nreq, maxcount)
                assert torch.equal(got, droppath_emu(kt, maxcount, seed, site0)), "droppath maxcount %d seed %#x site0 %d" % (maxcount, seed, site0)
                if keep[0] == 1.0:
                    assert bool((got == 1.0).all())
