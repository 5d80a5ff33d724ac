"""Case runner of tests/test_00b_attn_abi_gpu.py: the attention cores called through the C ABI (include/vptr_hip.h) and compared with plain torch
fp64 (helpers.win_attn_ref / temporal_attn_ref / ts_attn_ref).

The runner talks to a BACKEND: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's order without the trailing stream
(tensors for pointers, None for NULL), `seed(value)` returns the seed tensor of a new dropout scope and `dropout_mask(n, p, seed, site)` the mask
of elements 0 .. n-1 of a site (0 or 1 / (1 - p)).  The GPU file's backend hands the pointers to the library; `EmuBackend` below is a CPU
emulation of the same calls written from the header (closed-form backward, per-head loops, explicit row gathers), which tests/test_cpu.py runs
the same cases against: a wrong argument order, layout, mask shape or reference of a CASE fails there, without a GPU.

Every output lives inside a larger NaN-filled buffer (`Guarded`): one guard row of C floats, rounded up to a 64-byte multiple, before and after
it; after the call the guards must still be NaN and the (decoded) output finite."""
import functools

import torch

from helpers import current_attn_mode, margin, p16_encode, rel, temporal_attn_ref, ts_attn_ref, ts_rows, win_attn_ref
from oracle import fill
from oracle import vptr_oracle as O

TOL_FWD, TOL_BWD = 5e-5, 1e-4    # the project's bars of the attention cores (tests/test_00_ops_gpu.py TOLA), fp32 and decoded P16 alike
TOL_P16 = 1e-5                   # decoded P16 vs the fp32 output of the same call: the format's bound is 2^-17 = 7.6e-6 per element
DROP_P, DROP_SITE = 0.1, 7


def p16_decode(t):
    """as ops.core.p16_decode (restated: importing vptr_amd needs the built library, the emulated runs must not)"""
    C = t.shape[-1]
    b = t.contiguous().view(torch.bfloat16).reshape(-1, C // 16, 2, 16).float()
    return (b[:, :, 0] + b[:, :, 1]).reshape(t.shape)


class Guarded:
    """[rows, C] fp32 output inside a NaN-filled buffer with a guard of C floats (rounded up to 64 bytes) on both sides; shift: floats past the
    16-byte boundary at which the output starts"""

    def __init__(self, rows, C, dev, start=None, shift=0):
        self.g = -(-(C * 4) // 64) * 16 + shift
        self.buf = torch.full((2 * self.g + rows * C,), float("nan"), device=dev, dtype=torch.float32)
        self.out = self.buf[self.g: self.g + rows * C].view(rows, C)
        assert self.out.data_ptr() % 16 == 4 * shift
        if start is not None:
            self.out.copy_(start)

    def result(self, p16=False):
        """guards intact, output finite; returns the (decoded) output on the CPU"""
        buf = self.buf.cpu()
        n = self.out.numel()
        assert bool(torch.isnan(buf[:self.g]).all()) and bool(torch.isnan(buf[self.g + n:]).all()), "write outside the output rows"
        got = buf[self.g: self.g + n].view(self.out.shape)
        got = p16_decode(got) if p16 else got.clone()
        assert bool(torch.isfinite(got).all()), "output not written everywhere"
        return got


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
def _core_fwd_bwd(qw, kw, vw, gow, nh, bias, causal, mask, dq_scale):
    """closed-form attention of gathered problems [P, L, C] per head: returns o, dq, dk, dv [P, L, C] (gow None: forward only) and dS [P, nh, Lq, Lk]"""
    Pn, Lq, C = qw.shape
    Lk, hd = kw.shape[1], C // nh
    o, dq, dk, dv = torch.zeros_like(qw), torch.zeros_like(qw), torch.zeros_like(kw), torch.zeros_like(kw)
    dS = torch.zeros(Pn, nh, Lq, Lk, dtype=qw.dtype)
    for h in range(nh):
        sl = slice(h * hd, (h + 1) * hd)
        s = torch.einsum("pid,pjd->pij", qw[..., sl], kw[..., sl])
        if bias is not None:
            s = s + bias[h]
        if causal:
            i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
            s = torch.where(j > i, torch.full_like(s, -1e30), s)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        pr = e / e.sum(-1, keepdim=True)
        m = mask[:, h] if mask is not None else torch.ones_like(pr)
        o[..., sl] = torch.einsum("pij,pjd->pid", pr * m, vw[..., sl])
        if gow is None:
            continue
        dp = torch.einsum("pid,pjd->pij", gow[..., sl], vw[..., sl]) * m
        ds = pr * (dp - (dp * pr).sum(-1, keepdim=True))
        dS[:, h] = ds
        dq[..., sl] = torch.einsum("pij,pjd->pid", ds, kw[..., sl]) * dq_scale
        dk[..., sl] = torch.einsum("pij,pid->pjd", ds, qw[..., sl])
        dv[..., sl] = torch.einsum("pij,pid->pjd", pr * m, gow[..., sl])
    return o, dq, dk, dv, dS


class EmuBackend:
    """CPU emulation of the attention entry points (fp64 arithmetic on the fp32 inputs, outputs rounded to fp32 or encoded as P16); argument
    checks as the header documents them.  The dropout stand-in is a seeded Bernoulli stream indexed like the kernels' hash:
    element ((problem * nh + h) * Lq + i) * Lk + j."""
    dev = "cpu"

    def seed(self, value):
        return torch.tensor([int(value) + 0x9E3779B9], dtype=torch.int64)

    def dropout_mask(self, n, p, seed, site):
        g = torch.Generator().manual_seed((int(seed[0]) * 1315423911 + int(site)) & 0x7FFFFFFF)
        return (torch.rand(n, generator=g) >= p).float() / (1.0 - p)

    def call(self, name, *a):
        return getattr(self, name)(*a)

    @staticmethod
    def _put(dst, val, p16):
        val = val.float()
        dst.copy_(p16_encode(val) if p16 else val)

    def _mask(self, P, nh, Lq, Lk, p, seed, site, who):
        if not p > 0.0:
            return None
        if seed is None or p >= 1.0:
            raise RuntimeError("%s: dropout needs seed_dev" % who)
        return self.dropout_mask(P * nh * Lq * Lk, p, seed, site).double().reshape(P, nh, Lq, Lk)

    def _win(self, who, q, k, v, table, idx, go, B, H, W, C, nh, ws, p, seed, site, dq_scale, p16):
        if p16 and C % 16:
            raise RuntimeError("%s: P16 outputs need C %% 16 == 0" % who)
        if C % nh or H % ws or W % ws or ws * ws > 64:
            raise RuntimeError("%s: unsupported geometry (window too large / not a multiple)" % who)
        L, P = ws * ws, B * (H // ws) * (W // ws)
        mask = self._mask(P, nh, L, L, p, seed, site, who)
        rows = ts_rows(B, 1, H, W, ws).reshape(-1)          # frames as samples with T = 1: windows in (b, wy, wx) order, elements (ph, pw)
        bias = None if table is None else table.double()[idx.reshape(-1)].reshape(L, L, nh).permute(2, 0, 1)
        g = [t.double()[rows].reshape(P, L, C) for t in (q, k, v)]
        gow = None if go is None else go.double()[rows].reshape(P, L, C)
        res = _core_fwd_bwd(g[0], g[1], g[2], gow, nh, bias, False, mask, dq_scale)
        inv = torch.empty_like(rows)
        inv[rows] = torch.arange(rows.numel())
        return [t.reshape(P * L, C)[inv] for t in res[:4]], res[4]

    def winattn_fwd(self, q, k, v, table, idx, o, B, H, W, C, nh, ws, p, seed, site, p16):
        if table is not None and idx is None:
            raise RuntimeError("winattn_fwd: bias table needs rel_index")
        outs, _ = self._win("winattn_fwd", q, k, v, table, idx, None, B, H, W, C, nh, ws, p, seed, site, 1.0, p16)
        self._put(o, outs[0], p16)

    def winattn_bwd(self, q, k, v, table, idx, go, dq, dk, dv, dtable, B, H, W, C, nh, ws, p, seed, site, dq_scale, p16):
        outs, dS = self._win("winattn_bwd", q, k, v, table, idx, go, B, H, W, C, nh, ws, p, seed, site, dq_scale, p16)
        for dst, val in zip((dq, dk, dv), outs[1:]):
            self._put(dst, val, p16)
        if dtable is not None:                                   # ACCUMULATED
            L = ws * ws
            add = torch.zeros(dtable.shape, dtype=torch.float64).index_add_(0, idx.reshape(-1), dS.sum(0).permute(1, 2, 0).reshape(L * L, nh))
            dtable.add_(add.float())

    def winattn_bwd_ws(self, *a):
        wsp, nfl = a[-2], a[-1]
        if wsp is not None and nfl <= 0:
            raise RuntimeError("winattn_bwd: bad workspace")
        self.winattn_bwd(*a[:-2])

    def winattn_bwd_workspace(self, nh):
        return 256 * 2 * 4 * 52

    def _t(self, who, q, k, v, go, N, Tq, Tk, HW, C, nh, causal, p, seed, site, dq_scale, p16):
        if p16 and C % 16:
            raise RuntimeError("%s: P16 outputs need C %% 16 == 0" % who)
        if causal and Tq != Tk:
            raise RuntimeError("%s: causal mask needs Tq == Tk" % who)
        mask = self._mask(N * HW, nh, Tq, Tk, p, seed, site, who)

        def seq(t, T):
            return t.double().reshape(N, T, HW, C).transpose(1, 2).reshape(N * HW, T, C)
        res = _core_fwd_bwd(seq(q, Tq), seq(k, Tk), seq(v, Tk), None if go is None else seq(go, Tq), nh, None, causal, mask, dq_scale)
        Ts = (Tq, Tq, Tk, Tk)
        return [t.reshape(N, HW, T, C).transpose(1, 2).reshape(N * T * HW, C) for t, T in zip(res[:4], Ts)]

    def tattn_fwd(self, q, k, v, o, N, Tq, Tk, HW, C, nh, causal, p, seed, site, p16):
        self._put(o, self._t("tattn_fwd", q, k, v, None, N, Tq, Tk, HW, C, nh, causal, p, seed, site, 1.0, p16)[0], p16)

    def tattn_bwd(self, q, k, v, go, dq, dk, dv, N, Tq, Tk, HW, C, nh, causal, p, seed, site, dq_scale, p16):
        outs = self._t("tattn_bwd", q, k, v, go, N, Tq, Tk, HW, C, nh, causal, p, seed, site, dq_scale, p16)
        for dst, val in zip((dq, dk, dv), outs[1:]):
            self._put(dst, val, p16)

    def _ts(self, who, q, k, v, go, N, Tq, Tk, H, W, ws, C, nh, p, seed, site, p16):
        if p16 and C % 16:
            raise RuntimeError("%s: P16 outputs need C %% 16 == 0" % who)
        Lq, Lk = Tq * ws * ws, Tk * ws * ws
        rq, rk = ts_rows(N, Tq, H, W, ws), ts_rows(N, Tk, H, W, ws)
        P = rq.shape[0]
        mask = self._mask(P, nh, Lq, Lk, p, seed, site, who)
        qw, kw, vw = q.double()[rq.reshape(-1)].reshape(P, Lq, C), k.double()[rk.reshape(-1)].reshape(P, Lk, C), v.double()[rk.reshape(-1)].reshape(P, Lk, C)
        gow = None if go is None else go.double()[rq.reshape(-1)].reshape(P, Lq, C)
        res = _core_fwd_bwd(qw, kw, vw, gow, nh, None, False, mask, 1.0)
        outs = []
        for t, r in zip(res[:4], (rq, rq, rk, rk)):
            full = torch.empty(r.numel(), C, dtype=torch.float64)
            full[r.reshape(-1)] = t.reshape(-1, C)
            outs.append(full)
        return outs

    def tsattn_fwd(self, q, k, v, o, N, Tq, Tk, H, W, ws, C, nh, p, seed, site, p16):
        self._put(o, self._ts("tsattn_fwd", q, k, v, None, N, Tq, Tk, H, W, ws, C, nh, p, seed, site, p16)[0], p16)

    def tsattn_bwd(self, q, k, v, go, dq, dk, dv, N, Tq, Tk, H, W, ws, C, nh, p, seed, site, p16):
        outs = self._ts("tsattn_bwd", q, k, v, go, N, Tq, Tk, H, W, ws, C, nh, p, seed, site, p16)
        for dst, val in zip((dq, dk, dv), outs[1:]):
            self._put(dst, val, p16)


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


@functools.lru_cache(maxsize=4)
def win_inputs(B, H, W, C, nh, ws, bias):
    """seeded inputs of a window case (q and k scaled 0.5 as in tests/test_00_ops_gpu.py) and the no-dropout fp64 reference, dq_scale = hd^-0.5"""
    n = B * H * W
    q, k, v, go = rn((n, C), 150, 0.5), rn((n, C), 151, 0.5), rn((n, C), 152), rn((n, C), 154)
    table = rn(((2 * ws - 1) ** 2, nh), 153, 0.5) if bias else None
    idx = O.rpe_index(ws) if bias else None
    ref = win_attn_ref(q, k, v, go, B, H, W, nh, ws, table, idx, None, (C // nh) ** -0.5)
    return (q, k, v, go, table, idx), ref


@functools.lru_cache(maxsize=4)
def t_inputs(N, Tq, Tk, HW, C, nh, causal):
    q, k, v, go = rn((N * Tq * HW, C), 160, 0.5), rn((N * Tk * HW, C), 161, 0.5), rn((N * Tk * HW, C), 162), rn((N * Tq * HW, C), 163)
    ref = temporal_attn_ref(q, k, v, go, N, Tq, Tk, HW, nh, causal, None, (C // nh) ** -0.5)
    return (q, k, v, go), ref


@functools.lru_cache(maxsize=2)
def ts_inputs(N, Tq, Tk, H, W, ws, C, nh):
    q, k, v = rn((N * Tq * H * W, C), 180, 0.5), rn((N * Tk * H * W, C), 181, 0.5), rn((N * Tk * H * W, C), 182)
    go = rn((N * Tq * H * W, C), 183)
    return (q, k, v, go), ts_attn_ref(q, k, v, go, N, Tq, Tk, H, W, ws, nh)


def _to(be, *ts):
    return [None if t is None else t.to(be.dev) for t in ts]


def _shifted(t, shift):
    """t itself (shift 0), or a copy of it that starts `shift` floats past a 16-byte boundary"""
    if not shift:
        return t
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    out = buf[shift: shift + t.numel()].view(t.shape).copy_(t)
    assert out.data_ptr() % 16 == 4 * shift and out.is_contiguous()
    return out


# ------------------------------------------------------------------------------------------------------------------ one call each
def win_call(be, ins, B, H, W, C, nh, ws, p16, p=0.0, seed=None, table_start=None, want_dtable=True, entry="bwd", workspace=None, ws_floats=0,
             shift=0):
    """vptr_winattn_fwd + one backward entry point on guarded outputs; returns the decoded o, dq, dk, dv (and dtable) on the CPU.
    table_start: initial contents of the table gradient (None: zeros); want_dtable False: dbias_table == NULL; shift: q, k, v, dout and the four
    outputs start that many floats past a 16-byte boundary"""
    q, k, v, go, table, idx = _to(be, *ins)
    q, k, v, go = (_shifted(t, shift) for t in (q, k, v, go))
    n, ntab, scale = B * H * W, (2 * ws - 1) ** 2, (C // nh) ** -0.5
    o, dq, dk, dv = (Guarded(n, C, be.dev, shift=shift) for _ in range(4))
    be.call("winattn_fwd", q, k, v, table, idx, o.out, B, H, W, C, nh, ws, p, seed, DROP_SITE, int(p16))
    dt = None
    if table is not None and want_dtable:
        dt = Guarded(ntab, nh, be.dev, torch.zeros(ntab, nh) if table_start is None else table_start)
    args = (q, k, v, table, idx, go, dq.out, dk.out, dv.out, None if dt is None else dt.out, B, H, W, C, nh, ws, p, seed, DROP_SITE, scale, int(p16))
    if entry == "bwd":
        be.call("winattn_bwd", *args)
    else:
        be.call("winattn_bwd_ws", *(args + (workspace, ws_floats)))
    out = {"op": "winattn", "p16": bool(p16), "o": o.result(p16), "dq": dq.result(p16), "dk": dk.result(p16), "dv": dv.result(p16)}
    if dt is not None:
        out["dtable"] = dt.result()
    return out


def t_call(be, ins, N, Tq, Tk, HW, C, nh, causal, p16, p=0.0, seed=None, shift=0):
    q, k, v, go = (_shifted(t, shift) for t in _to(be, *ins))
    o, dq = Guarded(N * Tq * HW, C, be.dev, shift=shift), Guarded(N * Tq * HW, C, be.dev, shift=shift)
    dk, dv = Guarded(N * Tk * HW, C, be.dev, shift=shift), Guarded(N * Tk * HW, C, be.dev, shift=shift)
    be.call("tattn_fwd", q, k, v, o.out, N, Tq, Tk, HW, C, nh, int(causal), p, seed, DROP_SITE, int(p16))
    be.call("tattn_bwd", q, k, v, go, dq.out, dk.out, dv.out, N, Tq, Tk, HW, C, nh, int(causal), p, seed, DROP_SITE, (C // nh) ** -0.5, int(p16))
    return {"op": "tattn", "p16": bool(p16), "o": o.result(p16), "dq": dq.result(p16), "dk": dk.result(p16), "dv": dv.result(p16)}


def ts_call(be, ins, N, Tq, Tk, H, W, ws, C, nh, p16):
    q, k, v, go = _to(be, *ins)
    o, dq = Guarded(N * Tq * H * W, C, be.dev), Guarded(N * Tq * H * W, C, be.dev)
    dk, dv = Guarded(N * Tk * H * W, C, be.dev), Guarded(N * Tk * H * W, C, be.dev)
    be.call("tsattn_fwd", q, k, v, o.out, N, Tq, Tk, H, W, ws, C, nh, 0.0, None, 0, int(p16))
    be.call("tsattn_bwd", q, k, v, go, dq.out, dk.out, dv.out, N, Tq, Tk, H, W, ws, C, nh, 0.0, None, 0, int(p16))
    return {"op": "tsattn", "p16": bool(p16), "o": o.result(p16), "dq": dq.result(p16), "dk": dk.result(p16), "dv": dv.result(p16)}


def compare(got, ref, keys=("o", "dq", "dk", "dv", "dtable")):
    """every output present in both against fp64 at the project's bars; all figures are measured (and logged) before the first assertion"""
    vals = {kk: rel(got[kk], ref[kk]) for kk in keys if kk in got and kk in ref}
    for kk, val in vals.items():      # with VPTR_MARGIN_LOG: the worst value per (operator, kernel-family routing, output) against its bar
        margin("attn_abi %s %s %s%s" % (got["op"], current_attn_mode(), kk, " p16" if got["p16"] and kk != "dtable" else ""), val,
               TOL_FWD if kk == "o" else TOL_BWD)
    for kk, val in vals.items():
        assert val < (TOL_FWD if kk == "o" else TOL_BWD), (kk, vals)
    return vals


def compare_p16(got16, got32):
    """decoded P16 outputs vs the fp32 outputs of the same call repeated with p16 = 0"""
    vals = {kk: rel(got16[kk], got32[kk]) for kk in ("o", "dq", "dk", "dv")}
    for kk, val in vals.items():
        margin("attn_abi %s %s %s p16-vs-fp32" % (got16["op"], current_attn_mode(), kk), val, TOL_P16)
    assert max(vals.values()) < TOL_P16, vals
    return vals


# ------------------------------------------------------------------------------------------------------------------ the cases
# (nh, C): head dim and the instantiation class (ceil(hd / 32), ceil(hd / 16)) it reaches
HEAD_CLASSES = {"hd8_c11": (2, 16), "hd24_c12": (2, 48), "hd40_c23": (2, 80), "hd56_c24": (2, 112), "hd66_c35": (8, 528), "hd88_c36": (2, 176),
                "hd96_c36_limit": (2, 192), "hd94_oddpair_span96": (2, 188), "hd98_over_limit_vector": (2, 196)}
# kind, then (B, H, W, ws, bias) or (N, Tq, Tk, HW, causal)
GEOMS = {"win4_B3_8x8_bias": ("win", 3, 8, 8, 4, True), "win8_B1_8x16": ("win", 1, 8, 16, 8, False), "win2_B2_4x6_generic": ("win", 2, 4, 6, 2, True),
         "t5x5_causal": ("t", 2, 5, 5, 9, True), "t3x7": ("t", 2, 3, 7, 9, False), "t20x20_causal_2qblocks": ("t", 1, 20, 20, 5, True),
         "t40x33_tileshare": ("t", 1, 40, 33, 3, False)}
TABLE_GEOMS = {"win4_B3_8x8": ("win", 3, 8, 8, 4, True), "win8_B1_8x16": ("win", 1, 8, 16, 8, True)}
DROP_GEOMS = ("win4_B3_8x8_bias", "win8_B1_8x16", "t5x5_causal", "t3x7", "t20x20_causal_2qblocks")
DROP_HEADS = ("hd24_c12", "hd66_c35")
# launch classes: id -> (geometry, (nh, C) list, modes or None for all five)
LAUNCH_CASES = {
    "win4_1547win_loop_wpb8_tail": (("win", 7, 52, 68, 4, True), [(2, 48), (8, 192)], None),
    "win4_65win_wpb2_tail": (("win", 5, 4, 52, 4, True), [(2, 48), (8, 192)], ("vector",)),
    "win2_2139win_generic_wpb4_tail": (("win", 3, 46, 62, 2, True), [(2, 16), (8, 16)], ("default",)),
    "t5_causal_1551px_4px_per_wave": (("t", 3, 5, 5, 517, True), [(2, 48), (8, 192)], None),
    "t10_hd66_1551px_pf": (("t", 3, 10, 10, 517, False), [(2, 132)], None),
    "t11_hd66_1551px_pf_limit": (("t", 3, 11, 11, 517, True), [(2, 132)], None),     # 11 * att_pitch(66) / 2 = 374 <= 384 < 408
    "t16_hd66_1551px_no_pf": (("t", 3, 16, 16, 517, False), [(2, 132)], None),
    "mfma_win4_15prob_4slots": (("win", 5, 4, 4, 4, True), [(3, 48)], ("mfma",)),
    "mfma_t20_15prob_2slots": (("t", 1, 20, 20, 5, True), [(3, 48)], ("mfma",)),
    "mfma_t40_9prob_1slot": (("t", 1, 40, 40, 3, False), [(3, 48)], ("mfma",)),
}


def head_modes(hc, modes):
    """hd 98 is over the MFMA families' limit: only the default routing and VPTR_ATTN_MFMA=2 are asked to fall through to the vector kernels"""
    return [m for m in modes if hc != "hd98_over_limit_vector" or m in ("default", "mfma")]


def geom_inputs(geom, nh, C):
    if geom[0] == "win":
        _, B, H, W, ws, bias = geom
        return win_inputs(B, H, W, C, nh, ws, bias)
    _, N, Tq, Tk, HW, causal = geom
    return t_inputs(N, Tq, Tk, HW, C, nh, causal)


def geom_call(be, geom, ins, nh, C, p16, **kw):
    if geom[0] == "win":
        _, B, H, W, ws, _ = geom
        return win_call(be, ins, B, H, W, C, nh, ws, p16, **kw)
    _, N, Tq, Tk, HW, causal = geom
    return t_call(be, ins, N, Tq, Tk, HW, C, nh, causal, p16, **kw)


def run_parity(be, geom, nh, C):
    """fp32 outputs vs fp64 at the bars; with C % 16 == 0 the same call with P16 outputs: decoded vs fp64 at the same bars and vs the fp32 run"""
    ins, ref = geom_inputs(geom, nh, C)
    got = geom_call(be, geom, ins, nh, C, False)
    compare(got, ref)
    if C % 16 == 0:
        got16 = geom_call(be, geom, ins, nh, C, True)
        compare(got16, ref)
        compare_p16(got16, got)


def run_unaligned(be, geom, nh, C):
    """fp32 outputs with q, k, v, dout, o, dq, dk, dv all 8 bytes past a 16-byte boundary, same bars"""
    ins, ref = geom_inputs(geom, nh, C)
    compare(geom_call(be, geom, ins, nh, C, False, shift=2), ref)


def problem_dims(geom, nh):
    if geom[0] == "win":
        _, B, H, W, ws, _ = geom
        return B * (H // ws) * (W // ws), ws * ws, ws * ws
    _, N, Tq, Tk, HW, _ = geom
    return N * HW, Tq, Tk


def masked_ref(geom, ins, nh, C, mask):
    scale = (C // nh) ** -0.5
    if geom[0] == "win":
        _, B, H, W, ws, _ = geom
        q, k, v, go, table, idx = ins
        return win_attn_ref(q, k, v, go, B, H, W, nh, ws, table, idx, mask, scale)
    _, N, Tq, Tk, HW, causal = geom
    q, k, v, go = ins
    return temporal_attn_ref(q, k, v, go, N, Tq, Tk, HW, nh, causal, mask, scale)


def run_dropout(be, geom, nh, C):
    """dropout 0.1 on the probabilities, P16 outputs: the mask of element ((problem * nh + h) * Lq + i) * Lk + j is regenerated as
    (problems, nh, Lq, Lk) and injected into the fp64 reference; the zero share must be in (0.08, 0.12) and the mask-free reference far away"""
    ins, ref0 = geom_inputs(geom, nh, C)
    P, Lq, Lk = problem_dims(geom, nh)
    seed = be.seed(2468)
    got16 = geom_call(be, geom, ins, nh, C, True, p=DROP_P, seed=seed)
    got32 = geom_call(be, geom, ins, nh, C, False, p=DROP_P, seed=seed)
    mask = be.dropout_mask(P * nh * Lq * Lk, DROP_P, seed, DROP_SITE).reshape(P, nh, Lq, Lk).cpu()
    share = float((mask == 0).float().mean())
    assert 0.08 < share < 0.12, share
    ref = masked_ref(geom, ins, nh, C, mask)
    assert rel(ref0["o"], ref["o"]) > 10 * TOL_FWD          # the check would be vacuous otherwise
    compare(got16, ref)
    compare(got32, ref)
    compare_p16(got16, got32)


def seeded_table_start(ref, ntab, nh):
    """non-zero start of the table gradient, scaled to the RMS of the reference gradient"""
    return rn((ntab, nh), 190) * float(ref["dtable"].pow(2).mean().sqrt())


def run_table_contract(be, geom, nh, C, p16=True):
    """dbias_table is ACCUMULATED: from a seeded non-zero start the result minus the start must equal the reference gradient at 1e-4; with
    dbias_table == NULL (bias table present) dq, dk, dv keep their values"""
    _, B, H, W, ws, bias = geom
    assert bias
    ins, ref = geom_inputs(geom, nh, C)
    start = seeded_table_start(ref, (2 * ws - 1) ** 2, nh)
    got = win_call(be, ins, B, H, W, C, nh, ws, p16, table_start=start)
    compare(got, ref, ("o", "dq", "dk", "dv"))
    val = rel(got["dtable"].double() - start.double(), ref["dtable"])
    assert val < TOL_BWD, val
    got_null = win_call(be, ins, B, H, W, C, nh, ws, p16, want_dtable=False)
    assert "dtable" not in got_null
    compare(got_null, ref)
    for kk in ("dq", "dk", "dv"):
        assert rel(got_null[kk], got[kk]) < TOL_P16, kk


def run_workspace_contract(be, geom, nh, C):
    """vptr_winattn_bwd_ws with a NaN-filled workspace of vptr_winattn_bwd_workspace(nh) floats (the full grid), one float too small (atomic
    fallback) and NULL: the same table gradient at 1e-4 from a seeded start; the workspace form twice: bit-identical"""
    _, B, H, W, ws, _ = geom
    ins, ref = geom_inputs(geom, nh, C)
    start = seeded_table_start(ref, (2 * ws - 1) ** 2, nh)
    nfl = int(be.call("winattn_bwd_workspace", nh))
    full = []
    for rep in range(2):
        wsp = torch.full((nfl,), float("nan"), device=be.dev)
        full.append(win_call(be, ins, B, H, W, C, nh, ws, True, table_start=start, entry="ws", workspace=wsp, ws_floats=nfl))
    assert torch.equal(full[0]["dtable"], full[1]["dtable"])
    wsp = torch.full((nfl,), float("nan"), device=be.dev)
    small = win_call(be, ins, B, H, W, C, nh, ws, True, table_start=start, entry="ws", workspace=wsp, ws_floats=nfl - 1)
    null = win_call(be, ins, B, H, W, C, nh, ws, True, table_start=start, entry="ws", workspace=None, ws_floats=0)
    for got in (full[0], small, null):
        compare(got, ref, ("o", "dq", "dk", "dv"))
        val = rel(got["dtable"].double() - start.double(), ref["dtable"])
        assert val < TOL_BWD, val


def run_tslma(be, N, Tq, Tk, H, W, ws, C, nh):
    ins, ref = ts_inputs(N, Tq, Tk, H, W, ws, C, nh)
    got = ts_call(be, ins, N, Tq, Tk, H, W, ws, C, nh, False)
    compare(got, ref)
    got16 = ts_call(be, ins, N, Tq, Tk, H, W, ws, C, nh, True)
    compare(got16, ref)
    compare_p16(got16, got)


def run_guards(be, raises):
    """argument errors that must be reported before any launch; raises(callable): asserts that the call raises the backend's error"""
    d = be.dev
    z = torch.zeros(64 * 40, device=d)                       # big enough for every (rejected) geometry below, in case a check is missing
    C = 40                                                   # C % 4 == 0, C % 16 != 0
    raises(lambda: be.call("winattn_fwd", z, z, z, None, None, z, 1, 4, 4, C, 2, 4, 0.0, None, 0, 1))
    raises(lambda: be.call("winattn_bwd", z, z, z, None, None, z, z, z, z, None, 1, 4, 4, C, 2, 4, 0.0, None, 0, 1.0, 1))
    raises(lambda: be.call("winattn_bwd_ws", z, z, z, None, None, z, z, z, z, None, 1, 4, 4, C, 2, 4, 0.0, None, 0, 1.0, 1, None, 0))
    raises(lambda: be.call("tattn_fwd", z, z, z, z, 1, 4, 4, 4, C, 2, 0, 0.0, None, 0, 1))
    raises(lambda: be.call("tattn_bwd", z, z, z, z, z, z, z, 1, 4, 4, 4, C, 2, 0, 0.0, None, 0, 1.0, 1))
    raises(lambda: be.call("tsattn_fwd", z, z, z, z, 1, 2, 2, 2, 2, 2, C, 2, 0.0, None, 0, 1))
    raises(lambda: be.call("tsattn_bwd", z, z, z, z, z, z, z, 1, 2, 2, 2, 2, 2, C, 2, 0.0, None, 0, 1))
    # causal with Tq != Tk
    raises(lambda: be.call("tattn_fwd", z, z, z, z, 1, 3, 5, 4, 16, 2, 1, 0.0, None, 0, 0))
    raises(lambda: be.call("tattn_bwd", z, z, z, z, z, z, z, 1, 3, 5, 4, 16, 2, 1, 0.0, None, 0, 1.0, 0))
    # ws * ws > 64
    raises(lambda: be.call("winattn_fwd", z, z, z, None, None, z, 1, 9, 9, 16, 2, 9, 0.0, None, 0, 0))
    raises(lambda: be.call("winattn_bwd", z, z, z, None, None, z, z, z, z, None, 1, 9, 9, 16, 2, 9, 0.0, None, 0, 1.0, 0))
    # dropout without a seed
    raises(lambda: be.call("winattn_fwd", z, z, z, None, None, z, 1, 4, 4, 16, 2, 4, 0.1, None, 7, 0))
    raises(lambda: be.call("winattn_bwd", z, z, z, None, None, z, z, z, z, None, 1, 4, 4, 16, 2, 4, 0.1, None, 7, 1.0, 0))
    raises(lambda: be.call("tattn_fwd", z, z, z, z, 1, 4, 4, 4, 16, 2, 0, 0.1, None, 7, 0))
    raises(lambda: be.call("tattn_bwd", z, z, z, z, z, z, z, 1, 4, 4, 4, 16, 2, 0, 0.1, None, 7, 1.0, 0))
    raises(lambda: be.call("tsattn_fwd", z, z, z, z, 1, 2, 2, 2, 2, 2, 16, 2, 0.1, None, 7, 0))
    raises(lambda: be.call("tsattn_bwd", z, z, z, z, z, z, z, 1, 2, 2, 2, 2, 2, 16, 2, 0.1, None, 7, 0))
