"""Case runner of tests/test_09c_convffn_fwd_gpu.py: the forward kernels of the conv-FFN called through the C ABI (include/vptr_hip.h) --
vptr_norm_act_fwd in every launch class, vptr_dwconv3x3_fwd with its frame_stats epilogue, the fused vptr_dwconv3x3_norm_fwd in its LDS-slab and
register forms -- and compared with plain torch fp64 (helpers.norm_act_fwd_ref / dwconv3x3_fwd_ref / dwconv_norm_fwd_ref).

The runner talks to a BACKEND, as tests/attn_abi_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's order
without the trailing stream (tensors for pointers, None for NULL) and returns the call's return code, `seed(value)` returns the seed tensor of a
new dropout scope, `dropout_mask(n, p, seed, site)` the mask of elements 0 .. n-1 of a site (0 or 1 / (1 - p)), `p16_decode(t)` the fp32 image of
a P16 tensor.  The GPU file's backend hands the pointers to the library; `EmuBackend` below is a CPU emulation written from the header, which
tests/test_cpu.py runs the same cases against: a wrong argument order, layout or reference of a CASE fails there, without a GPU.

Every output lives inside a larger NaN-filled buffer (`Guarded`); statistics rows are [frames][VPTR_FRAME_STATS_STRIDE] with a NaN sentinel of a
known bit pattern in the 30 unused slots, compared bit for bit after the call.

Bars: fp32 outputs and statistics 2e-5 rel-L2, a decoded P16 output 2^-16, the fp16 side copy |ah - ref| <= 2^-11 |ref| +
2^-24 per element (round-to-nearest of a correct value: half an ulp of a normal, half the subnormal spacing below 2^-14) and rel-L2 < 2^-11."""
import functools

import torch
import torch.nn.functional as F

from helpers import VAR_GUARD, convffn_fwd_class, dwconv3x3_fwd_ref, dwconv_norm_fwd_ref, margin, norm_act_fwd_ref, p16_encode, rel
from oracle import fill

TOLV = 2e-5                      # fp32 vector kernels
TOLP16 = 2.0 ** -16              # a P16 image of a kernel's output
TOLH = 2.0 ** -11                # the fp16 side copy
STRIDE = 32                      # VPTR_FRAME_STATS_STRIDE
NAN = float("nan")
SENTINEL = 0x7FC01234            # a quiet NaN with a payload: the unused statistics slots
DROP_P, SITE = 0.1, 13
NONE, GELU, RELU = 0, 1, 2


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Guarded:
    """[rows, C] output (fp32 or fp16) inside a NaN-filled buffer with a guard of C elements (rounded up to 64 bytes) on both sides"""

    def __init__(self, rows, C, dev, dtype=torch.float32, start=None):
        per64 = 16 if dtype == torch.float32 else 32
        self.g = -(-C // per64) * per64
        self.buf = torch.full((2 * self.g + rows * C,), NAN, device=dev, dtype=dtype)
        self.out = self.buf[self.g: self.g + rows * C].view(rows, C)
        assert self.out.data_ptr() % 64 == 0
        if start is not None:
            self.out.copy_(start)

    def guards_intact(self):
        buf, n = self.buf.cpu(), self.out.numel()
        return bool(torch.isnan(buf[:self.g]).all()) and bool(torch.isnan(buf[self.g + n:]).all())

    def untouched(self):
        """nothing was written at all (a rejected call)"""
        return bool(torch.isnan(self.buf.cpu()).all())

    def result(self, decode=None):
        """guards intact, output finite; returns the (decoded) output on the CPU"""
        assert self.guards_intact(), "write outside the output rows"
        got = self.out.cpu()
        got = decode(got) if decode is not None else got.clone()
        assert bool(torch.isfinite(got).all()), "output not written everywhere"
        return got


def stats_rows(s0, s1):
    """[frames][STRIDE] fp32 rows: slot 0 / 1 from the fp64 vectors s0 / s1 rounded to fp32, the other 30 slots the NaN sentinel"""
    rows = torch.full((s0.numel(), STRIDE), SENTINEL, dtype=torch.int32).view(torch.float32)
    rows[:, 0], rows[:, 1] = s0.float(), s1.float()
    return rows


def ideal_sums(x, frames):
    xf = x.double().reshape(frames, -1)
    return xf.sum(1), (xf * xf).sum(1)


def check_stats(after, before, want0, want1, tag):
    """slots 0 / 1 vs their fp64 targets at TOLV (None: must be bit-identical), slots 2 .. 31 bit-identical"""
    after = after.cpu()
    assert same_bits(after[:, 2:], before[:, 2:]), "%s: an unused statistics slot changed" % tag
    if want0 is None:
        assert same_bits(after[:, :2], before[:, :2]), "%s: the statistics rows changed" % tag
        return
    v0, v1 = rel(after[:, 0], want0), rel(after[:, 1], want1)
    print("%s: frame sums rel %.3e, sums of squares rel %.3e" % (tag, v0, v1))
    assert v0 < TOLV and v1 < TOLV, (tag, v0, v1)


def half_figures(ah, ref, tag):
    """the fp16 side copy against fp64: (rel-L2, worst per-element error / (2^-11 |ref| + 2^-24), elements over that bound); printed and logged"""
    got, ref = ah.double(), ref.double()
    err, bound = (got - ref).abs(), TOLH * ref.abs() + 2.0 ** -24
    ratio = err / bound
    worst, over, r = float(ratio.max()), int((err > bound).sum()), rel(got, ref)
    margin("convffn_fwd %s fp16 per-element" % tag, worst, 1.0)
    i = int(ratio.reshape(-1).argmax())
    print("%s: fp16 copy rel-L2 %.3e; worst element error / bound %.3f (ref %.4e, got %.4e), %d of %d over the bound"
          % (tag, r, worst, float(ref.reshape(-1)[i]), float(got.reshape(-1)[i]), over, ref.numel()))
    return r, worst, over


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
class EmuBackend:
    """CPU emulation of the three entry points from include/vptr_hip.h: fp64 arithmetic on the fp32 inputs in the modules' own formulation
    (F.batch_norm / F.layer_norm, nine shifted adds for the depthwise taps), outputs rounded to fp32 / fp16 or encoded as P16, accumulated
    statistics added onto what the buffer holds, the documented argument checks with a non-zero return code.  The dropout stand-in is a seeded
    Bernoulli stream indexed by the flat element index."""
    dev = "cpu"

    def seed(self, value):
        return torch.tensor([int(value) + 0x9E3779B9], dtype=torch.int64)

    def dropout_mask(self, n, p, seed, site):
        g = torch.Generator().manual_seed((int(seed[0]) * 1315423911 + int(site)) & 0x7FFFFFFF)
        return (torch.rand(n, generator=g) >= p).float() / (1.0 - p)

    def p16_decode(self, t):
        C = t.shape[-1]
        b = t.contiguous().view(torch.bfloat16).reshape(-1, C // 16, 2, 16).float()
        return (b[:, :, 0] + b[:, :, 1]).reshape(t.shape)

    def sync(self):
        pass

    def call(self, name, *a):
        return getattr(self, name)(*a)

    @staticmethod
    def _act(pre, act):
        return F.gelu(pre) if act == GELU else (torch.relu(pre) if act == RELU else pre)

    @staticmethod
    def _frame_stats(xf, raw_stats, eps, armed):
        """mean / rstd of the frames from their sums; where the header promises it (armed), a frame whose one-pass variance falls under
        VAR_GUARD x E[x^2] gets the statistics of a second pass over its elements"""
        n = xf.shape[1]
        m, e2 = raw_stats[:, 0].double() / n, raw_stats[:, 1].double() / n
        var = (e2 - m * m).clamp_min(0.0)
        if armed:
            redo = var < VAR_GUARD * e2
            m = torch.where(redo, xf.mean(1), m)
            var = torch.where(redo, xf.var(1, unbiased=False), var)
        return m, (var + eps).rsqrt()

    def norm_act_fwd(self, x, mean, rstd, w, b, y, rows, Fc, HW, per_col, act, p, seed, site, rowscale, rs_div, rs_mod, residual, p16, raw_stats,
                     eps):
        if raw_stats is not None and (per_col or mean is None or rstd is None):
            return -1
        if rows <= 0 or Fc <= 0 or Fc % 4 or HW < 1 or (not per_col and rows % HW):
            return -1
        if p16 and (Fc % 16 or y.data_ptr() % 64):
            return -1
        if p > 0 and (seed is None or p >= 1):
            return -1
        if rowscale is not None and (rs_div < 1 or rs_mod < 1):
            return -1
        xd = x.double().reshape(rows, Fc)
        if per_col:
            xh = (xd - mean.double()) * rstd.double()
            pre = xh * w.double() + b.double()
        else:
            frames, n = rows // HW, HW * Fc
            if raw_stats is not None:
                armed = (HW * (Fc // 4)) % 256 == 0 and (rows * (Fc // 4)) % 256 == 0
                m, r = self._frame_stats(xd.view(frames, n), raw_stats, eps, armed)
                mean.view(-1).copy_(m.float())
                rstd.view(-1).copy_(r.float())
            else:
                m, r = mean.double(), rstd.double()
            xh = (xd.view(frames, HW, Fc) - m[:, None, None]) * r[:, None, None]
            pre = (xh * w.double().view(HW, Fc) + b.double().view(HW, Fc)).reshape(rows, Fc)
        o = self._act(pre, act)
        if p > 0:
            o = o * self.dropout_mask(rows * Fc, p, seed, site).double().reshape(rows, Fc)
        if rowscale is not None:
            o = o * rowscale.double()[(torch.arange(rows) // rs_div) % rs_mod][:, None]
        if residual is not None:
            o = o + residual.double()
        y.copy_(p16_encode(o.float()) if p16 else o.float())
        return 0

    @staticmethod
    def _dw(a, w9, b9, frames, H, W, Fc):
        a4 = a.reshape(frames, H, W, Fc)
        pad = F.pad(a4, (0, 0, 1, 1, 1, 1))
        y = torch.zeros_like(a4) if b9 is None else b9.double().expand_as(a4).clone()
        for ky in range(3):
            for kx in range(3):
                y = y + pad[:, ky:ky + H, kx:kx + W, :] * w9.double()[ky * 3 + kx]
        return y.reshape(frames * H * W, Fc)

    @staticmethod
    def _add_stats(stats, y, frames):
        yf = y.reshape(frames, -1)
        stats[:, 0] += yf.sum(1).float()
        stats[:, 1] += (yf * yf).sum(1).float()

    def dwconv3x3_fwd(self, x, w9, b, y, frames, H, W, Fc, frame_stats):
        if min(frames, H, W, Fc) <= 0 or Fc % 4:
            return -1
        if frame_stats is not None and (W % 2 or ((W // 2) * (Fc // 4)) % 64):
            return -1
        o = self._dw(x.double(), w9, b, frames, H, W, Fc)
        y.copy_(o.float())
        if frame_stats is not None:
            self._add_stats(frame_stats, o, frames)
        return 0

    def dwconv3x3_norm_fwd(self, x, raw_stats, aw, ab, eps, act, w9, b, y, a_half, mean_out, rstd_out, frames, H, W, Fc, frame_stats):
        if any(t is None for t in (x, raw_stats, aw, ab, w9, y, mean_out, rstd_out)) or min(frames, H, W, Fc) <= 0 or Fc % 4:
            return -1
        W2 = W // 2
        if W % 2 or W2 < 1 or 16 % W2 or (W2 * (Fc // 4)) % 64:
            return -1
        if any(t is not None and t.data_ptr() % 16 for t in (x, y, aw, ab, w9, b)) or (a_half is not None and a_half.data_ptr() % 8):
            return -1
        n = H * W * Fc
        m, r = self._frame_stats(x.double().reshape(frames, n), raw_stats, eps, True)
        mean_out.view(-1).copy_(m.float())
        rstd_out.view(-1).copy_(r.float())
        xh = (x.double().reshape(frames, H * W, Fc) - m[:, None, None]) * r[:, None, None]
        a = self._act(xh * aw.double().view(H * W, Fc) + ab.double().view(H * W, Fc), act).reshape(frames * H * W, Fc)
        if a_half is not None:
            a_half.copy_(a.half())
        o = self._dw(a, w9, b, frames, H, W, Fc)
        y.copy_(o.float())
        if frame_stats is not None:
            self._add_stats(frame_stats, o, frames)
        return 0


# ----------------------------------------------------------------------------------------------------------- a. vptr_norm_act_fwd
# id -> (per_col, rows, HW, F); the float4 count is rows * F / 4.  What each one reaches (helpers.convffn_fwd_class, asserted in test_cpu.py):
#   bn_small       <true> kernel: 615 float4, the last of three workgroups partial; rowscale (row / 7) % 4
#   bn_stride      2 099 200 float4 > 8192 x 256: the grid-stride second trip covers the last 2048
#   ln_small       <false> kernel: a frame is 60 float4, so workgroups straddle frames
#   ln_armed       <false>: HW * F / 4 = 1024 and total % 256 == 0 -> the large-mean recompute is armed
#   ln_15          245 760 float4: one frame short of the position-major switch
#   ln_pos_min     exactly 2^18 float4: norm_act_fwd_pos_kernel, gridDim.y = 4
#   ln_pos_ragged  the pos kernel with P = 15 000: 152 live threads in the last x-workgroup, frames 16 / 17 on a fifth trip of y = 0, 1; not armed
NA_GEOMS = {
    "bn_small": (True, 123, 1, 20), "bn_stride": (True, 8200, 1, 1024), "ln_small": (False, 13 * 12, 12, 20), "ln_armed": (False, 4 * 64, 64, 64),
    "ln_15": (False, 15 * 64, 64, 1024), "ln_pos_min": (False, 16 * 64, 64, 1024), "ln_pos_ragged": (False, 18 * 60, 60, 1000),
}
NA_CLASSES = {      # id -> (kernel, grid, float4, trips, armed with raw_stats)
    "bn_small": ("col", (3, 1), 615, 1, False), "bn_stride": ("col", (8192, 1), 2099200, 2, False), "ln_small": ("row", (4, 1), 780, 1, False),
    "ln_armed": ("row", (16, 1), 4096, 1, True), "ln_15": ("row", (960, 1), 245760, 1, True), "ln_pos_min": ("pos", (64, 4), 1 << 18, 4, True),
    "ln_pos_ragged": ("pos", (59, 4), 270000, 5, False),
}
NA_VARIANTS = ("plain", "full", "raw", "p16")


def na_cases():
    """(geometry, variant) of test_norm_act_fwd: p16 only where F % 16 == 0, raw only in the LayerNorm mode, ReLU once"""
    out = []
    for gid, (per_col, _, _, Fc) in NA_GEOMS.items():
        out += [(gid, v) for v in NA_VARIANTS if not (v == "p16" and Fc % 16) and not (v == "raw" and per_col)]
        if gid == "ln_small":
            out.append((gid, "relu"))
    return out


def na_rs_mod(gid):
    return 4 if gid == "bn_small" else 5


@functools.lru_cache(maxsize=2)
def _na_base(gid):
    """seeded inputs of one geometry and the fp64 pre-activation / statistics every variant shares"""
    per_col, rows, HW, Fc = NA_GEOMS[gid]
    seed = 4000 + 10 * sorted(NA_GEOMS).index(gid)
    aff = (Fc,) if per_col else (HW, Fc)
    x, w, b = rn((rows, Fc), seed, 2.0) + 0.3, rn(aff, seed + 1).abs() + 0.5, rn(aff, seed + 2, 0.3)
    res = rn((rows, Fc), seed + 3)
    rs = rn((na_rs_mod(gid),), seed + 4).abs() + 0.5
    rs[1] = 0.0                                    # a dropped path
    base = norm_act_fwd_ref(x, w, b, HW, per_col, NONE)
    return {"x": x, "w": w, "b": b, "res": res, "rs": rs, "pre": base["pre"], "mean": base["mean"], "rstd": base["rstd"]}


def _finish(pre, act, mask=None, keep=1.0, rs=None, rs_div=1, rs_mod=1, res=None):
    y = F.gelu(pre) if act == GELU else (torch.relu(pre) if act == RELU else pre)
    if mask is not None:
        y = y * mask.double() / keep
    if rs is not None:
        y = y * rs.double()[(torch.arange(pre.shape[0]) // rs_div) % rs_mod][:, None]
    return y if res is None else y + res.double()


def run_norm_act(be, gid, variant):
    per_col, rows, HW, Fc = NA_GEOMS[gid]
    G, dev = _na_base(gid), be.dev
    act = {"plain": NONE, "relu": RELU}.get(variant, GELU)
    full, raw, p16 = variant == "full", variant == "raw", variant == "p16"
    nstat = Fc if per_col else rows // HW
    mask = seed = rs = res = None
    p, rs_div, rs_mod = 0.0, 1, 1
    if full:
        p, rs, rs_div, rs_mod, res = DROP_P, G["rs"], 7, na_rs_mod(gid), G["res"]
        seed = be.seed(97531)
        md = be.dropout_mask(rows * Fc, p, seed, SITE).reshape(rows, Fc).cpu()      # element index = row * F + col
        mask = (md != 0).float()
        assert 0.05 < float((mask == 0).double().mean()) < 0.15
        assert rel(md, mask.double() / (1.0 - p)) < 1e-6
    want = _finish(G["pre"], act, mask, 1.0 - p, rs, rs_div, rs_mod, res)
    y = Guarded(rows, Fc, dev)
    xd, wd, bd = G["x"].to(dev), G["w"].to(dev), G["b"].to(dev)
    rsd, resd = (rs.to(dev) if full else None), (res.to(dev) if full else None)
    rawh = rawd = None
    if raw:
        rawh = stats_rows(*ideal_sums(G["x"], nstat))
        rawd = rawh.clone().to(dev)
        mean, rstd = Guarded(nstat, 1, dev), Guarded(nstat, 1, dev)
        md_, rd_ = mean.out, rstd.out
    else:
        mh, rh = G["mean"].float(), G["rstd"].float()           # the fp64 statistics handed over as fp32
        md_, rd_ = mh.to(dev), rh.to(dev)
    rc = be.call("norm_act_fwd", xd, md_, rd_, wd, bd, y.out, rows, Fc, HW, int(per_col), act, p, seed, SITE, rsd, rs_div, rs_mod, resd, int(p16), rawd,
                 1e-5)
    assert rc == 0, rc
    be.sync()
    tag = "norm_act_fwd %s %s" % (gid, variant)
    if p16:
        v = rel(y.result(be.p16_decode), want)
        print("%s: y (P16) rel %.3e" % (tag, v))
        assert v < TOLP16, (tag, v)
    else:
        got = y.result()
        v = rel(got, want)
        print("%s: y rel %.3e" % (tag, v))
        assert v < TOLV, (tag, v)
        cls = convffn_fwd_class("norm_act", rows=rows, F=Fc, HW=HW, per_col=per_col, raw=raw)
        if cls["trips"] > 1 and cls["kernel"] != "pos":      # the rows of the grid-stride second trip on their own
            first = cls["grid"][0] * 256 * 4 // Fc
            assert 0 < first < rows
            vt = rel(got[first:], want[first:])
            assert vt < TOLV, (tag, "second trip", vt)
        if cls["kernel"] == "pos" and cls["trips"] * cls["grid"][1] != rows // HW:      # the frames of the ragged last trip
            first = (cls["trips"] - 1) * cls["grid"][1] * HW
            vt = rel(got[first:], want[first:])
            assert vt < TOLV, (tag, "last trip", vt)
    if raw:
        vm, vr = rel(mean.result(), G["mean"]), rel(rstd.result(), G["rstd"])
        print("%s: mean rel %.3e, rstd rel %.3e" % (tag, vm, vr))
        assert vm < TOLV and vr < TOLV, (tag, vm, vr)
        check_stats(rawd, rawh, None, None, tag)
    else:
        assert same_bits(md_, mh) and same_bits(rd_, rh), "%s: the statistics inputs changed" % tag


def run_norm_act_rejects(be):
    """raw_stats belong to the LayerNorm mode (per_col = 1 refused) and need the mean / rstd outputs; a P16 output needs F % 16 == 0: non-zero
    return code, nothing written"""
    dev = be.dev
    rows, HW, Fc = 24, 4, 20
    x, w, b = rn((rows, Fc), 1).to(dev), rn((Fc,), 2).to(dev), rn((Fc,), 3).to(dev)
    wl, bl = rn((HW, Fc), 4).to(dev), rn((HW, Fc), 5).to(dev)
    rawh = stats_rows(*ideal_sums(x.cpu(), rows // HW))
    rawd = rawh.clone().to(dev)
    for per_col, mean, rstd, wq, bq, p16, rq in ((1, Guarded(Fc, 1, dev), Guarded(Fc, 1, dev), w, b, 0, rawd),
                                                  (0, None, None, wl, bl, 0, rawd),
                                                  (0, Guarded(rows // HW, 1, dev), Guarded(rows // HW, 1, dev), wl, bl, 1, rawd)):
        y = Guarded(rows, Fc, dev)
        rc = be.call("norm_act_fwd", x, None if mean is None else mean.out, None if rstd is None else rstd.out, wq, bq, y.out, rows, Fc, HW, per_col, GELU,
                     0.0, None, 0, None, 1, 1, None, p16, rq, 1e-5)
        assert rc != 0
        be.sync()
        assert y.untouched() and (mean is None or (mean.untouched() and rstd.untouched()))
        check_stats(rawd, rawh, None, None, "norm_act_fwd reject")


# ------------------------------------------------------------------------------------------------------------- b. the large-mean guard
# the four places that hold the guard: (kind, frames, H, W, F)
GUARD_PLACES = {"ln_armed": ("na", 4, 8, 8, 64), "ln_pos_min": ("na", 16, 8, 8, 1024), "dwn_lds": ("dwn", 3, 8, 8, 64), "dwn_reg": ("dwn", 3, 4, 16, 32)}
GUARD_RATIOS = (9, 12, 25, 100)


@functools.lru_cache(maxsize=2)
def _guard_base(place, r):
    kind, frames, H, W, Fc = GUARD_PLACES[place]
    HW = H * W
    seed = 5000 + 100 * sorted(GUARD_PLACES).index(place) + r
    sign = torch.where(torch.arange(frames) % 2 == 1, -1.0, 1.0)
    x = (rn((frames, HW * Fc), seed) + float(r) * sign[:, None]).reshape(frames * HW, Fc)       # frame f: (-1)^f r + N(0, 1)
    aw, ab = rn((HW, Fc), seed + 1).abs() + 0.5, rn((HW, Fc), seed + 2, 0.3)
    w9, b9 = rn((9, Fc), seed + 3, 0.3), 1.0 + rn((Fc,), seed + 4, 0.3)
    ref = dwconv_norm_fwd_ref(x, aw, ab, w9, b9, frames, H, W, GELU)
    return {"x": x, "aw": aw, "ab": ab, "w9": w9, "b9": b9, "ref": ref}


def run_guard(be, place, r):
    """frames of mean +-r and unit variance, raw_stats from ideal sums, GELU: y, mean and rstd at TOLV"""
    kind, frames, H, W, Fc = GUARD_PLACES[place]
    G, dev, HW = _guard_base(place, r), be.dev, H * W
    rows, ref = frames * HW, G["ref"]
    rawh = stats_rows(*ideal_sums(G["x"], frames))
    rawd = rawh.clone().to(dev)
    y, mean, rstd = Guarded(rows, Fc, dev), Guarded(frames, 1, dev), Guarded(frames, 1, dev)
    xd, awd, abd = G["x"].to(dev), G["aw"].to(dev), G["ab"].to(dev)
    if kind == "na":
        cls = convffn_fwd_class("norm_act", rows=rows, F=Fc, HW=HW, per_col=False, raw=True)
        assert cls["armed"] and cls["kernel"] == ("pos" if place == "ln_pos_min" else "row")
        rc = be.call("norm_act_fwd", xd, mean.out, rstd.out, awd, abd, y.out, rows, Fc, HW, 0, GELU, 0.0, None, 0, None, 1, 1, None, 0, rawd, 1e-5)
        want = ref["a"]
    else:
        assert convffn_fwd_class("dwconv_norm", frames=frames, H=H, W=W, F=Fc)["kernel"] == place[4:]
        rc = be.call("dwconv3x3_norm_fwd", xd, rawd, awd, abd, 1e-5, GELU, G["w9"].to(dev), G["b9"].to(dev), y.out, None, mean.out, rstd.out, frames, H, W,
                     Fc, None)
        want = ref["y"]
    assert rc == 0, rc
    be.sync()
    vy, vm, vr = rel(y.result(), want), rel(mean.result(), ref["mean"]), rel(rstd.result(), ref["rstd"])
    print("guard %s r = %d: y rel %.3e, mean rel %.3e, rstd rel %.3e" % (place, r, vy, vm, vr))
    check_stats(rawd, rawh, None, None, "guard %s" % place)
    assert vy < TOLV and vm < TOLV and vr < TOLV, (place, r, vy, vm, vr)


# ------------------------------------------------------------------------------------------ c. vptr_dwconv3x3_fwd with frame_stats
# (frames, H, W, F) -> kernel
DW_STATS_GEOMS = {(5, 8, 8, 64): "fwd3", (3, 4, 2, 256): "fwd3", (2, 4, 32, 16): "fwd3", (3, 5, 6, 256): "fwd2", (2, 8, 12, 128): "fwd2"}
DW_STATS_REJECTS = [(2, 4, 5, 64), (2, 4, 4, 32)]          # odd W; (W / 2) * (F / 4) = 16


def _dw_inputs(geom, seed):
    frames, H, W, Fc = geom
    return rn((frames * H * W, Fc), seed, 2.0) + 0.3, rn((9, Fc), seed + 1, 0.3), 1.0 + rn((Fc,), seed + 2, 0.3)


def _stats_start(frames, seed):
    s = rn((frames, 2), seed, 0.5)
    return stats_rows(s[:, 0].double(), s[:, 1].double())


def run_dwconv_stats(be, geom):
    """y vs fp64 F.conv2d(groups = F); the statistics rows start from non-zero values: slots 0 / 1 vs start + sum(y_ref) / sum(y_ref^2)"""
    frames, H, W, Fc = geom
    assert convffn_fwd_class("dwconv", frames=frames, H=H, W=W, F=Fc, stats=True)["kernel"] == DW_STATS_GEOMS[geom]
    dev, seed = be.dev, 6000 + 10 * sorted(DW_STATS_GEOMS).index(geom)
    x, w9, b9 = _dw_inputs(geom, seed)
    want = dwconv3x3_fwd_ref(x, w9, b9, frames, H, W)
    wf = want.view(frames, -1)
    sth = _stats_start(frames, seed + 3)
    std, y = sth.clone().to(dev), Guarded(frames * H * W, Fc, dev)
    rc = be.call("dwconv3x3_fwd", x.to(dev), w9.to(dev), b9.to(dev), y.out, frames, H, W, Fc, std)
    assert rc == 0, rc
    be.sync()
    tag = "dwconv3x3_fwd %dx%dx%dx%d" % geom
    v = rel(y.result(), want)
    print("%s: y rel %.3e" % (tag, v))
    assert v < TOLV, (tag, v)
    check_stats(std, sth, sth[:, 0].double() + wf.sum(1), sth[:, 1].double() + (wf * wf).sum(1), tag)


def run_dwconv_stats_rejects(be):
    dev = be.dev
    for geom in DW_STATS_REJECTS:
        frames, H, W, Fc = geom
        assert convffn_fwd_class("dwconv", frames=frames, H=H, W=W, F=Fc, stats=True)["kernel"] == "reject"
        x, w9, b9 = _dw_inputs(geom, 6100)
        sth = _stats_start(frames, 6103)
        std, y = sth.clone().to(dev), Guarded(frames * H * W, Fc, dev)
        rc = be.call("dwconv3x3_fwd", x.to(dev), w9.to(dev), b9.to(dev), y.out, frames, H, W, Fc, std)
        assert rc != 0, geom
        be.sync()
        assert y.untouched(), geom
        check_stats(std, sth, None, None, "dwconv3x3_fwd reject %s" % (geom,))


# -------------------------------------------------------------------------------------------------- d. vptr_dwconv3x3_norm_fwd
# (frames, H, W, F) -> kernel.  LDS slab (F % 64 == 0 and H * W <= 256): the model's map; HW = 40, a single partial phase-1 trip with clamped
# loads; HW = 72, the second trip partial; W / 2 = 1; HW = 256, the largest slab (64 KB of dynamic LDS next to the kernel's static array).
# Register walk: F % 64 != 0; HW = 272
DWN_GEOMS = {(5, 8, 8, 64): "lds", (3, 5, 8, 128): "lds", (2, 9, 8, 64): "lds", (2, 3, 2, 256): "lds", (2, 16, 16, 64): "lds", (3, 4, 16, 32): "reg",
             (2, 17, 16, 64): "reg"}
DWN_VARIANTS = ("all", "none", "no_half", "no_stats", "no_bias")
DWN_REJECTS = {"odd_W": (2, 4, 5, 64), "W12": (2, 4, 12, 64), "W8_F32": (2, 4, 8, 32)}


def dwn_cases(half_only=False):
    """(geometry, variant): GELU with everything present on every geometry, the other variants on the model's map and on the F % 64 != 0 one;
    half_only: the cases that write the fp16 side copy"""
    return [(g, v) for g in DWN_GEOMS for v in DWN_VARIANTS if (v == "all" or g in ((5, 8, 8, 64), (3, 4, 16, 32))) and not (half_only and v == "no_half")]


@functools.lru_cache(maxsize=2)
def _dwn_base(geom):
    frames, H, W, Fc = geom
    HW, seed = H * W, 7000 + 10 * sorted(DWN_GEOMS).index(geom)
    x = rn((frames * HW, Fc), seed, 2.0) + 0.3
    aw, ab = rn((HW, Fc), seed + 1).abs() + 0.5, rn((HW, Fc), seed + 2, 0.3)
    w9, b9 = rn((9, Fc), seed + 3, 0.3), 1.0 + rn((Fc,), seed + 4, 0.3)
    return {"x": x, "aw": aw, "ab": ab, "w9": w9, "b9": b9, "seed": seed}


@functools.lru_cache(maxsize=4)
def _dwn_ref(geom, act, bias):
    G = _dwn_base(geom)
    frames, H, W, Fc = geom
    return dwconv_norm_fwd_ref(G["x"], G["aw"], G["ab"], G["w9"], G["b9"] if bias else None, frames, H, W, act)


def _dwn_call(be, geom, variant):
    frames, H, W, Fc = geom
    assert convffn_fwd_class("dwconv_norm", frames=frames, H=H, W=W, F=Fc)["kernel"] == DWN_GEOMS[geom]
    G, dev, rows = _dwn_base(geom), be.dev, frames * H * W
    act, bias = (NONE if variant == "none" else GELU), variant != "no_bias"
    ref = _dwn_ref(geom, act, bias)
    rawh = stats_rows(*ideal_sums(G["x"], frames))
    rawd = rawh.clone().to(dev)
    sth = _stats_start(frames, G["seed"] + 5)
    std = None if variant == "no_stats" else sth.clone().to(dev)
    y, mean, rstd = Guarded(rows, Fc, dev), Guarded(frames, 1, dev), Guarded(frames, 1, dev)
    ah = None if variant == "no_half" else Guarded(rows, Fc, dev, torch.float16)
    rc = be.call("dwconv3x3_norm_fwd", G["x"].to(dev), rawd, G["aw"].to(dev), G["ab"].to(dev), 1e-5, act, G["w9"].to(dev),
                 G["b9"].to(dev) if bias else None, y.out, None if ah is None else ah.out, mean.out, rstd.out, frames, H, W, Fc, std)
    tag = "dwconv3x3_norm_fwd %dx%dx%dx%d %s" % (geom + (variant,))
    assert rc == 0, (tag, rc)
    be.sync()
    return {"tag": tag, "ref": ref, "y": y, "mean": mean, "rstd": rstd, "ah": ah, "rawd": rawd, "rawh": rawh, "std": std, "sth": sth}


def run_dwn(be, geom, variant):
    """y, mean_out / rstd_out and the accumulated frame_stats vs fp64 conv2d(act(layer_norm(x))) at TOLV, the fp16 copy of the activated tensor
    at 2^-11 rel-L2 (its per-element bound: run_dwn_half_elements); raw_stats and the unused statistics slots bit-identical"""
    c = _dwn_call(be, geom, variant)
    tag, ref = c["tag"], c["ref"]
    vy, vm, vr = rel(c["y"].result(), ref["y"]), rel(c["mean"].result(), ref["mean"]), rel(c["rstd"].result(), ref["rstd"])
    print("%s: y rel %.3e, mean rel %.3e, rstd rel %.3e" % (tag, vy, vm, vr))
    check_stats(c["rawd"], c["rawh"], None, None, tag)
    assert vy < TOLV and vm < TOLV and vr < TOLV, (tag, vy, vm, vr)
    if c["ah"] is not None:
        r, _, _ = half_figures(c["ah"].result(), ref["a"], tag)
        assert r < TOLH, (tag, r)
    if c["std"] is not None:
        sth = c["sth"]
        check_stats(c["std"], sth, sth[:, 0].double() + ref["sum"], sth[:, 1].double() + ref["sumsq"], tag)


def run_dwn_half_elements(be, geom, variant):
    """every element of the fp16 side copy: |ah - ref| <= 2^-11 |ref| + 2^-24 (round-to-nearest of a correct value)"""
    c = _dwn_call(be, geom, variant)
    _, worst, over = half_figures(c["ah"].result(), c["ref"]["a"], c["tag"])
    assert over == 0, (c["tag"], over, worst)


def run_dwn_rejects(be):
    """odd W, W = 12 (W / 2 does not divide 16), W 8 with F 32 ((W/2)*(F/4) = 32) and x one float past a 16-byte boundary: non-zero return code,
    every output and the statistics rows untouched"""
    dev = be.dev
    cases = [(k, g, 0) for k, g in DWN_REJECTS.items()] + [("x_shifted", (5, 8, 8, 64), 1)]
    for name, geom, shift in cases:
        frames, H, W, Fc = geom
        rows = frames * H * W
        if not shift:
            assert convffn_fwd_class("dwconv_norm", frames=frames, H=H, W=W, F=Fc)["kernel"] == "reject", name
        xbuf = (rn((rows * Fc + 4,), 7100, 2.0) + 0.3).to(dev)
        x = xbuf[shift: shift + rows * Fc].view(rows, Fc)
        assert x.data_ptr() % 16 == 4 * shift
        aw, ab = (rn((H * W, Fc), 7101).abs() + 0.5).to(dev), rn((H * W, Fc), 7102, 0.3).to(dev)
        w9, b9 = rn((9, Fc), 7103, 0.3).to(dev), rn((Fc,), 7104, 0.3).to(dev)
        rawh, sth = stats_rows(*ideal_sums(x.cpu(), frames)), _stats_start(frames, 7105)
        rawd, std = rawh.clone().to(dev), sth.clone().to(dev)
        y, mean, rstd, ah = Guarded(rows, Fc, dev), Guarded(frames, 1, dev), Guarded(frames, 1, dev), Guarded(rows, Fc, dev, torch.float16)
        rc = be.call("dwconv3x3_norm_fwd", x, rawd, aw, ab, 1e-5, GELU, w9, b9, y.out, ah.out, mean.out, rstd.out, frames, H, W, Fc, std)
        assert rc != 0, name
        be.sync()
        assert y.untouched() and ah.untouched() and mean.untouched() and rstd.untouched(), name
        check_stats(std, sth, None, None, "dwconv3x3_norm_fwd reject " + name)
        check_stats(rawd, rawh, None, None, "dwconv3x3_norm_fwd reject " + name)


# --------------------------------------------------------------------------------------------------- e. chain with real producer sums
CHAIN_GEOMS = [(5, 8, 8, 64), (16, 8, 8, 1024)]      # the row-major kernel; 2^18 float4 on 16 frames: the position-major kernel


def run_chain(be, geom):
    """vptr_dwconv3x3_fwd(frame_stats) into a zeroed buffer, then vptr_norm_act_fwd(raw_stats = that buffer): the sums the normalisation reads
    are the producer's own fp32 atomics.  Against the fp64 composition GELU(LayerNorm(conv2d(x)))"""
    frames, H, W, Fc = geom
    dev, HW, rows, seed = be.dev, H * W, frames * H * W, 8000 + geom[3]
    x, w9, b9 = _dw_inputs(geom, seed)
    aw, ab = rn((HW, Fc), seed + 3).abs() + 0.5, rn((HW, Fc), seed + 4, 0.3)
    y1_ref = dwconv3x3_fwd_ref(x, w9, b9, frames, H, W)
    ref = norm_act_fwd_ref(y1_ref, aw, ab, HW, False, GELU)
    kernel = convffn_fwd_class("norm_act", rows=rows, F=Fc, HW=HW, per_col=False, raw=True)["kernel"]
    assert kernel == ("pos" if Fc == 1024 else "row")
    stats = torch.zeros((frames, STRIDE), device=dev)
    y1, y2, mean, rstd = Guarded(rows, Fc, dev), Guarded(rows, Fc, dev), Guarded(frames, 1, dev), Guarded(frames, 1, dev)
    assert be.call("dwconv3x3_fwd", x.to(dev), w9.to(dev), b9.to(dev), y1.out, frames, H, W, Fc, stats) == 0
    assert be.call("norm_act_fwd", y1.out, mean.out, rstd.out, aw.to(dev), ab.to(dev), y2.out, rows, Fc, HW, 0, GELU, 0.0, None, 0, None, 1, 1, None, 0, stats,
                   1e-5) == 0
    be.sync()
    assert float(stats[:, 2:].abs().max()) == 0.0
    v1, v2 = rel(y1.result(), y1_ref), rel(y2.result(), ref["y"])
    vm, vr = rel(mean.result(), ref["mean"]), rel(rstd.result(), ref["rstd"])
    print("chain %dx%dx%dx%d: conv rel %.3e, y rel %.3e, mean rel %.3e, rstd rel %.3e" % (geom + (v1, v2, vm, vr)))
    assert v1 < TOLV and v2 < TOLV and vm < TOLV and vr < TOLV, (geom, v1, v2, vm, vr)
