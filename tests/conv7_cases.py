"""Case runner of tests/test_09k_conv7_abi_gpu.py: the seven entry points of csrc/conv7.hip called through the C ABI (include/vptr_hip.h) in
every launch class of their launchers (helpers.conv7_class) and compared, element by element, with plain torch fp64 on the CPU
(F.pad(mode="reflect") + F.conv2d and autograd) from seeded oracle.fill inputs.

The runner talks to a BACKEND, as tests/convffn_fwd_cases.py does: `call(name, *args)` takes the arguments of `vptr_<name>` in the header's
order without the trailing stream (tensors for pointers, None for NULL) and returns the return code; `workspace_floats(B, Cimg)`,
`set_deterministic(on)` and `sync()` complete it.  The GPU file's backend hands the pointers to the library; `EmuBackend` below is a CPU
emulation written from the header (fp64 arithmetic, outputs rounded to fp32, planes encoded as [pixel][c / 32][hi 32 | lo 32] bf16, dw / db
accumulated, a non-zero code where the launchers' argument checks refuse), which tests/test_cpu.py runs the same cases against -- and named
MUTATIONS of it, each of which has to fail a case.

Guards: every output is a window of a larger buffer that holds a NaN canary of a known bit pattern everywhere else (`Guard`); the workspace has
its canary right behind vptr_conv7_out_bwd_weight_workspace floats, the plane buffer's extra last row has to stay zero, a refused call has to
leave every word as it was.

Backward calls get y = the fp32 rounding of the fp64 forward, and their reference is formed in fp64 from that same fp32 y, so only the call's
own arithmetic is judged; dw and db start from seeded non-zero values.

Per-element bars, u = 2^-23, S = the same operation on absolute values in fp64 (for a gradient: autograd of the absolute-valued forward with |g|
upstream, which carries the mirror folds of the reflection padding):
  conv7_in_fwd           (49 Cimg + 2) u S, S including |scale| and |shift|
  conv7_in_fwd_planes    the same + 2^-16 |ref|
  conv7_out_fwd          before the activation (49 + 6 + 1) u S: 49 FMAs per lane, six reduction levels, the bias; after it that bar times the
                         activation's gain (1 for tanh, 1 / 4 for sigmoid) + 2 ACT_ERR |ref|.  ACT_ERR is the worst relative error of tanhf /
                         the __expf sigmoid MEASURED on the MI355X against fp64 tanh / sigmoid of the same call's out_act = 0 output
                         (profiles/conv7_margins.md); comparing the two calls is sound because the kernels apply out_act to the finished
                         sum + bias only (conv7_out_fwd_kernel and conv7_out_fwd2_kernel: `v = ... + bias; if (out_act == 1) v = tanhf(v)`),
                         so the accumulation does not depend on it.  The test asserts that the error it measures stays within ACT_ERR
  conv7_out_bwd_data     (4 * 49 Cimg + 4) u S
  dw, db, conv7_in's dw  (B H W + 3) u S + u |start|: sound for any summation order
Rel-L2 at the project's bars as well (TOLV 2e-5 values, TOLG 5e-5 gradients): per output channel of every forward output, per input channel of
dx, per (co, ky) row of dw; a slice whose reference norm is below 1e-3 of the median is compared against the median.
ReLU kinks (conv7_in with a scale): elements with |pre_ref| <= bar are left out of the value check only; no case may leave out more than 1 %."""
import functools

import torch
import torch.nn.functional as F

from helpers import conv7_class, margin
from oracle import fill

U = 2.0 ** -23
TOLV, TOLG = 2e-5, 5e-5
TOLP = 2.0 ** -16                 # the bf16 hi + lo image of a value
KINK_SHARE = 0.01
CANARY = 0x7FC01234               # quiet NaN with a payload: everything a call may not write
SLACK = 64                        # words in front of and behind every guarded window
NONE, TANH, SIGMOID = 0, 1, 2
GAIN = {NONE: 1.0, TANH: 1.0, SIGMOID: 0.25}
# worst relative error of the device's tanhf / 1 / (1 + __expf(-v)) over every conv7_out_fwd case, measured (profiles/conv7_margins.md)
ACT_ERR = {TANH: 1.05e-7, SIGMOID: 2.12e-7}
SIGMOID_EXPECTED = lambda v: (v.abs() + 4.0) * 2.0 ** -24      # what a correctly rounded exp / reciprocal chain would give, relative


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Guard:
    """a window of n 32-bit words on a 128-byte boundary (+ shift words) inside a canary-filled buffer; zero_tail: words right behind the window
    that start as zero and have to stay zero (the plane buffer's last row); start: what the window holds before the call"""

    def __init__(self, be, n, start=None, zero_tail=0, shift=0):
        self.buf = torch.full((n + zero_tail + 2 * SLACK + 32 + shift,), CANARY, dtype=torch.int32).to(be.dev)
        self.o = SLACK + ((-(self.buf.data_ptr() + 4 * SLACK)) % 128) // 4 + shift
        self.n, self.started = n, start is not None
        if start is not None:
            self.buf[self.o: self.o + n].copy_(start.contiguous().reshape(-1).view(torch.int32))
        if zero_tail:
            self.buf[self.o + n: self.o + n + zero_tail].zero_()
        self.before = self.buf.cpu().clone()
        self.out = self.buf[self.o: self.o + n].view(torch.float32)
        assert self.out.data_ptr() % 128 == (4 * shift) % 128

    def intact(self):
        now = self.buf.cpu()
        return torch.equal(now[:self.o], self.before[:self.o]) and torch.equal(now[self.o + self.n:], self.before[self.o + self.n:])

    def untouched(self):
        return torch.equal(self.buf.cpu(), self.before)

    def words(self):
        assert self.intact(), "write outside the output window (or into the row that stays zero)"
        w = self.buf.cpu()[self.o: self.o + self.n].clone()
        assert self.started or not bool((w == CANARY).any()), "output not written everywhere"
        return w

    def result(self, shape):
        got = self.words().view(torch.float32).reshape(shape)
        assert bool(torch.isfinite(got).all()), "output not finite"
        return got


def planes_decode(words, npix):
    """[pixel][c / 32][hi 32 | lo 32] bf16 -> (hi + lo, hi) as fp32 [npix, 64]"""
    b = words.view(torch.bfloat16).reshape(npix, 2, 2, 32).float()
    out = (b[:, :, 0] + b[:, :, 1]).reshape(npix, 64)
    assert bool(torch.isfinite(out).all())
    return out, b[:, :, 0].reshape(npix, 64)


def planes_encode(v):
    g = v.float().reshape(-1, 2, 32)
    hi = g.to(torch.bfloat16)
    lo = (g - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], 2).contiguous().reshape(-1).view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def conv_ref(x, w, replicate=False):
    """ReflectionPad2d(3) + Conv7x7 in fp64: x [B, Ci, H, W], w [Co, Ci, 7, 7]"""
    return F.conv2d(F.pad(x.double(), (3, 3, 3, 3), mode="replicate" if replicate else "reflect"), w.double())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def act64(v, act):
    return torch.tanh(v) if act == TANH else (torch.sigmoid(v) if act == SIGMOID else v)


def act_grad64(dy, y, act):
    """the activation's gradient from its OUTPUT, as the kernels form it"""
    dy, y = dy.double(), y.double()
    return dy * (1.0 - y * y) if act == TANH else (dy * y * (1.0 - y) if act == SIGMOID else dy)


def conv_grads(x, w, g):
    """fp64 autograd of conv_ref under the upstream gradient g: (dx, dw)"""
    xr, wr = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    conv_ref(xr, wr).backward(g.double())
    return xr.grad, wr.grad


# ------------------------------------------------------------------------------------------------------------------------ checking
def slice_rel(got, ref, keep):
    """worst rel-L2 over the slices that keep the dimensions `keep`; a slice whose reference norm is below 1e-3 of the median counts against
    the median"""
    dims = [d for d in range(ref.dim()) if d not in keep]
    e = got.double() - ref
    en, rn_ = e.pow(2).sum(dims).sqrt().reshape(-1), ref.pow(2).sum(dims).sqrt().reshape(-1)
    med = float(rn_.median())
    den = torch.where(rn_ < 1e-3 * med, torch.full_like(rn_, med), rn_)
    return float((en / den.clamp_min(1e-300)).max())


def check(tag, got, ref, bar, keep, tol, skip=None):
    """every element within its bar (skip: the kink elements, at most KINK_SHARE of them) and every slice within tol (None: elements only); returns (worst element
    error / bar, worst slice rel-L2)"""
    assert got.shape == ref.shape == bar.shape, (tag, got.shape, ref.shape, bar.shape)
    ratio = (got.double() - ref).abs() / bar.clamp_min(1e-300)
    left_out = 0.0
    if skip is not None:
        left_out = float(skip.double().mean())
        ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
    worst, r = float(ratio.max()), slice_rel(got, ref, keep)
    margin("conv7 %s per-element" % tag, worst, 1.0)
    if tol is not None:
        margin("conv7 %s slices" % tag, r, tol)
    i = int(ratio.reshape(-1).argmax())
    print("conv7 %s: worst element error / bar %.4f (ref %.5e, got %.5e), worst slice rel-L2 %.3e (bar %s), %.3f %% left to the kink rule"
          % (tag, worst, float(ref.reshape(-1)[i]), float(got.reshape(-1)[i]), r, tol, 100.0 * left_out))
    assert left_out <= KINK_SHARE, (tag, left_out)
    assert worst <= 1.0, (tag, "element", worst)
    assert tol is None or r < tol, (tag, "slice", r)
    return worst, r


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
MUTATIONS = ("replicate", "dx_fold_dropped", "kykx_swapped", "sigmoid_grad_dy", "dw_overwritten", "planes_swapped", "chunk_off_by_quad")


class EmuBackend:
    """CPU emulation of the seven entry points from include/vptr_hip.h: fp64 F.pad(reflect) + F.conv2d and autograd on the fp32 inputs, outputs
    rounded to fp32, the argument checks of the launchers with a non-zero return code.  mut: one of MUTATIONS, a deliberate defect"""
    dev = "cpu"

    def __init__(self, mut=None):
        assert mut is None or mut in MUTATIONS, mut
        self.mut, self.det = mut, 0

    def call(self, name, *a):
        return getattr(self, name)(*a)

    def workspace_floats(self, B, Cimg):
        return B * 3 * Cimg * 49 * 64

    def set_deterministic(self, on):
        self.det = int(on)

    def sync(self):
        pass

    def _w(self, w, shape):
        w = w.double().reshape(shape)
        return w.transpose(2, 3) if self.mut == "kykx_swapped" else w

    def _conv(self, x, w):
        return conv_ref(x, w, self.mut == "replicate")

    def _in_fwd(self, x, w, scale, shift, B, Cimg, H, W, chunked):
        v = self._conv(x.reshape(B, Cimg, H, W), self._w(w, (64, Cimg, 7, 7)))
        if scale is not None:
            v = torch.relu(v * scale.double().view(1, 64, 1, 1) + shift.double().view(1, 64, 1, 1))
        if self.mut == "chunk_off_by_quad" and chunked and W >= 68:
            v = v.clone()
            v[..., 60:64] = v[..., 64:68]
        return nhwc(v)

    def conv7_in_fwd(self, x, w, scale, shift, y, B, Cimg, H, W, Cout):
        cls = conv7_class("in_fwd", B=B, Cimg=Cimg, H=H, W=W, Cout=Cout)["class"]
        if cls.endswith("reject"):
            return -1
        y.copy_(self._in_fwd(x, w, scale, shift, B, Cimg, H, W, "fwd2c" in cls).float().reshape(-1))
        return 0

    def conv7_in_fwd_planes(self, x, w, scale, shift, planes, B, Cimg, H, W, Cout):
        cls = conv7_class("in_fwd_planes", B=B, Cimg=Cimg, H=H, W=W, Cout=Cout, aligned=planes is not None and planes.data_ptr() % 128 == 0)["class"]
        if planes is None or cls.endswith("reject"):
            return -1
        v = self._in_fwd(x, w, scale, shift, B, Cimg, H, W, "fwd2c" in cls).float().reshape(-1, 64)
        enc = planes_encode(v).view(-1, 2, 2, 16)                       # [pixel, block][hi | lo][16 words]
        if self.mut == "planes_swapped":
            enc = enc.flip(2)
        planes.view(torch.int32)[: enc.numel()].copy_(enc.reshape(-1))
        return 0

    def conv7_out_fwd(self, x, w, bias, y, B, Cin, H, W, Cimg, out_act):
        if conv7_class("out_fwd", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"].endswith("reject"):
            return -1
        v = self._conv(nchw(x.reshape(B, H, W, 64)), self._w(w, (Cimg, 64, 7, 7))) + bias.double().view(1, Cimg, 1, 1)
        y.copy_(act64(v.float().double(), out_act).float().reshape(-1))      # the activation of the fp32 sum, as the kernels apply it
        return 0

    def _g(self, dy, y, B, Cimg, H, W, out_act):
        if self.mut == "sigmoid_grad_dy" and out_act == SIGMOID:
            return dy.double().reshape(B, Cimg, H, W)
        return act_grad64(dy, y, out_act).reshape(B, Cimg, H, W)

    def conv7_out_bwd_data(self, dy, y, w, dx, B, Cin, H, W, Cimg, out_act):
        if conv7_class("out_bwd_data", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"].endswith("reject"):
            return -1
        g, wd = self._g(dy, y, B, Cimg, H, W, out_act), self._w(w, (Cimg, Cin, 7, 7))
        if self.mut == "dx_fold_dropped":          # the gradient on the padded grid, folded without the mirror image of the top border
            from helpers import reflect_fold_ref
            xp = torch.zeros((B, Cin, H + 6, W + 6), dtype=torch.float64, requires_grad=True)
            F.conv2d(xp, wd).backward(g)
            gp = xp.grad.clone()
            gp[:, :, :3] = 0.0
            d = reflect_fold_ref(gp, 3)
        else:
            xr = torch.zeros((B, Cin, H, W), dtype=torch.float64, requires_grad=True)
            self._conv(xr, wd).backward(g)
            d = xr.grad
        dx.copy_(nhwc(d).float().reshape(-1))
        return 0

    def _out_dw(self, dy, y, x, dw, db, B, H, W, Cimg, out_act):
        g = self._g(dy, y, B, Cimg, H, W, out_act)
        wr = torch.zeros((Cimg, 64, 7, 7), dtype=torch.float64, requires_grad=True)
        self._conv(nchw(x.reshape(B, H, W, 64)).double(), wr).backward(g)
        gw = wr.grad.transpose(2, 3) if self.mut == "kykx_swapped" else wr.grad
        gw = gw.reshape(-1)
        dw.copy_((gw if self.mut == "dw_overwritten" else dw.double() + gw).float())
        if db is not None:
            db.copy_((db.double() + g.sum((0, 2, 3))).float())
        return 0

    def conv7_out_bwd_weight(self, dy, y, x, dw, db, B, Cin, H, W, Cimg, out_act):
        if conv7_class("out_bwd_weight", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"].endswith("reject"):
            return -1
        return self._out_dw(dy, y, x, dw, db, B, H, W, Cimg, out_act)

    def conv7_out_bwd_weight_ws(self, dy, y, x, dw, db, B, Cin, H, W, Cimg, out_act, workspace, workspace_floats):
        cls = conv7_class("out_bwd_weight_ws", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin, ws_floats=None if workspace is None else workspace_floats,
                          aligned=workspace is None or workspace.data_ptr() % 16 == 0)["class"]
        if cls.endswith("reject"):
            return -1
        return self._out_dw(dy, y, x, dw, db, B, H, W, Cimg, out_act)

    def conv7_in_bwd_weight(self, dy, x, dw, B, Cimg, H, W, Cout):
        if dy is None or x is None or dw is None or conv7_class("in_bwd_weight", B=B, Cimg=Cimg, H=H, W=W, Cout=Cout)["class"].endswith("reject"):
            return -1
        wr = torch.zeros((64, Cimg, 7, 7), dtype=torch.float64, requires_grad=True)
        self._conv(x.reshape(B, Cimg, H, W).double(), wr).backward(nchw(dy.reshape(B, H, W, 64)).double())
        gw = (wr.grad.transpose(2, 3) if self.mut == "kykx_swapped" else wr.grad).reshape(-1)
        dw.copy_((gw if self.mut == "dw_overwritten" else dw.double() + gw).float())
        return 0


# ------------------------------------------------------------------------------------------------------------ a. vptr_conv7_in_fwd
# (B, Cimg, H, W) -> class.  fwd2: every reflection inside one band; a second band of one row (three idle waves); W past one 64-column walk.
# fwd2c: Cimg 2 and 4; nq = 16; a second chunk of one quad; three chunks; more than 64 KB of LDS (the launcher raises the kernel's limit).
# gen1: odd sizes with a partial last workgroup; Cimg > 4
IN_FWD = {(2, 1, 4, 4): "fwd2", (1, 1, 9, 8): "fwd2", (1, 1, 20, 68): "fwd2",
          (1, 2, 4, 4): "fwd2c", (2, 3, 8, 64): "fwd2c", (1, 3, 8, 68): "fwd2c", (1, 3, 5, 132): "fwd2c", (1, 4, 4, 12): "fwd2c",
          (1, 3, 4, 384): "fwd2c_attr", (1, 4, 4, 288): "fwd2c_attr",
          (1, 1, 9, 11): "gen1", (3, 3, 5, 7): "gen1", (1, 5, 4, 8): "gen1"}
IN_FWD_REJECTS = {"H3": (1, 1, 3, 8, 64), "W3": (1, 1, 8, 3, 64), "Cout32": (1, 1, 8, 8, 32), "Cimg6": (1, 6, 8, 8, 64)}
IN_PLANES = {(2, 1, 4, 4): "fwd2", (1, 3, 8, 68): "fwd2c", (1, 4, 4, 12): "fwd2c", (1, 3, 4, 384): "fwd2c_attr"}
IN_PLANES_REJECTS = {"W6": (1, 1, 8, 6, 0), "Cimg5": (1, 5, 8, 8, 0), "off64": (1, 1, 8, 8, 16)}      # (B, Cimg, H, W, shift in words)


def _seed(table, geom, base):
    return base + 10 * sorted(table).index(geom)


@functools.lru_cache(maxsize=4)
def _in_base(geom):
    """seeded inputs of one conv7_in geometry, the fp64 convolution and the one on absolute values"""
    B, Cimg, H, W = geom
    seed = 11000 + 1000 * Cimg + 10 * H + W
    x, w = rn((B, Cimg, H, W), seed), rn((64, Cimg, 7, 7), seed + 1, 0.1)
    scale, shift = rn((64,), seed + 2).abs() + 0.5, rn((64,), seed + 3, 0.3)
    scale[1::2] *= -1.0
    return {"x": x, "w": w, "scale": scale, "shift": shift, "conv": nhwc(conv_ref(x, w)), "S": nhwc(conv_ref(x.abs(), w.abs()))}


def _in_want(G, with_scale, Cimg):
    """(ref, bar, kink elements) of conv7_in_fwd"""
    if not with_scale:
        return G["conv"], (49 * Cimg + 2) * U * G["S"], None
    pre = G["conv"] * G["scale"].double() + G["shift"].double()
    bar = (49 * Cimg + 2) * U * (G["S"] * G["scale"].double().abs() + G["shift"].double().abs())
    return torch.relu(pre), bar, pre.abs() <= bar


def run_in_fwd(be, geom, with_scale):
    B, Cimg, H, W = geom
    cls = conv7_class("in_fwd", B=B, Cimg=Cimg, H=H, W=W)
    assert cls["class"] == "in_fwd/" + IN_FWD[geom], cls
    G, dev = _in_base(geom), be.dev
    ref, bar, skip = _in_want(G, with_scale, Cimg)
    y = Guard(be, B * H * W * 64)
    rc = be.call("conv7_in_fwd", G["x"].to(dev), G["w"].to(dev), G["scale"].to(dev) if with_scale else None, G["shift"].to(dev) if with_scale else None,
                 y.out, B, Cimg, H, W, 64)
    assert rc == 0, (geom, rc)
    be.sync()
    tag = "in_fwd %s %dx%dx%dx%d %s" % ((IN_FWD[geom],) + geom + ("scale" if with_scale else "raw",))
    return check(tag, y.result((B, H, W, 64)), ref, bar, (3,), TOLV, skip)


def run_in_fwd_rejects(be):
    for name, (B, Cimg, H, W, Cout) in IN_FWD_REJECTS.items():
        assert conv7_class("in_fwd", B=B, Cimg=Cimg, H=H, W=W, Cout=Cout)["class"] == "in_fwd/reject", name
        x, w = rn((B, Cimg, H, W), 11900).to(be.dev), rn((64, Cimg, 7, 7), 11901, 0.1).to(be.dev)
        y = Guard(be, B * H * W * 64)
        rc = be.call("conv7_in_fwd", x, w, None, None, y.out, B, Cimg, H, W, Cout)
        assert rc != 0, name
        be.sync()
        assert y.untouched(), name


def run_in_planes(be, geom):
    """the folded BatchNorm + ReLU result as bf16 hi / lo planes; the buffer's extra last row stays zero"""
    B, Cimg, H, W = geom
    cls = conv7_class("in_fwd_planes", B=B, Cimg=Cimg, H=H, W=W)
    assert cls["class"] == "in_fwd_planes/" + IN_PLANES[geom], cls
    G, dev, npix = _in_base(geom), be.dev, B * H * W
    ref, bar, skip = _in_want(G, True, Cimg)
    p = Guard(be, npix * 64, zero_tail=64)
    rc = be.call("conv7_in_fwd_planes", G["x"].to(dev), G["w"].to(dev), G["scale"].to(dev), G["shift"].to(dev), p.out, B, Cimg, H, W, 64)
    assert rc == 0, (geom, rc)
    be.sync()
    tag = "in_fwd_planes %s %dx%dx%dx%d" % ((IN_PLANES[geom],) + geom)
    both, hi = planes_decode(p.words(), npix)
    # the hi half alone is the value to bf16 precision (8 significant bits, either rounding): the halves are where the consumer reads them
    assert bool(((hi.reshape(B, H, W, 64).double() - ref).abs() <= 2.0 ** -8 * ref.abs() + bar).all()), tag + ": the hi plane is not the bf16 image"
    return check(tag, both.reshape(B, H, W, 64), ref, bar + TOLP * ref.abs(), (3,), TOLV, skip)


def run_in_planes_rejects(be):
    for name, (B, Cimg, H, W, shift) in IN_PLANES_REJECTS.items():
        assert conv7_class("in_fwd_planes", B=B, Cimg=Cimg, H=H, W=W, aligned=shift == 0)["class"] == "in_fwd_planes/reject", name
        x, w = rn((B, Cimg, H, W), 11910).to(be.dev), rn((64, Cimg, 7, 7), 11911, 0.1).to(be.dev)
        sc, sh = (rn((64,), 11912).abs() + 0.5).to(be.dev), rn((64,), 11913, 0.3).to(be.dev)
        p = Guard(be, B * H * W * 64, zero_tail=64, shift=shift)
        rc = be.call("conv7_in_fwd_planes", x, w, sc, sh, p.out, B, Cimg, H, W, 64)
        assert rc != 0, name
        be.sync()
        assert p.untouched(), name


# ------------------------------------------------------------------------------------------------------ b. vptr_conv7_in_bwd_weight
# (B, H, W): 2047, 2048, 2050 and 4100 pixels around the 2048-pixel chunk (2049 = 3 x 683 has no factorisation with H, W > 3: 2050 is the
# smallest count past one chunk that the entry point accepts), each with Cimg 1 and 3 and in both determinism modes
IN_DW_GEOMS = [(1, 23, 89), (1, 32, 64), (1, 25, 82), (2, 25, 82)]


def in_dw_cases():
    return [(B, Cimg, H, W, det) for (B, H, W) in IN_DW_GEOMS for Cimg in (1, 3) for det in (0, 1)]


@functools.lru_cache(maxsize=2)
def _in_dw_base(B, Cimg, H, W):
    seed = 12000 + 100 * Cimg + H
    x, dy = rn((B, Cimg, H, W), seed), rn((B, H, W, 64), seed + 1)
    start = rn((64, Cimg, 7, 7), seed + 2)
    zero = torch.zeros((64, Cimg, 7, 7))
    _, dw = conv_grads(x, zero, nchw(dy))
    _, S = conv_grads(x.abs(), zero, nchw(dy).abs())
    return {"x": x, "dy": dy, "start": start, "dw": dw, "S": S}


def run_in_dw(be, B, Cimg, H, W, det):
    cls = conv7_class("in_bwd_weight", B=B, Cimg=Cimg, H=H, W=W, deterministic=bool(det))
    assert cls["class"] == "in_bwd_weight/" + ("one_wg" if det else "chunks"), cls
    G, dev = _in_dw_base(B, Cimg, H, W), be.dev
    ref = G["start"].double() + G["dw"]
    bar = (B * H * W + 3) * U * G["S"] + U * G["start"].double().abs()
    xd, dyd = G["x"].to(dev), G["dy"].to(dev)
    got = []
    be.set_deterministic(det)
    try:
        for _ in range(2 if det else 1):
            dw = Guard(be, 64 * Cimg * 49, start=G["start"])
            rc = be.call("conv7_in_bwd_weight", dyd, xd, dw.out, B, Cimg, H, W, 64)
            assert rc == 0, rc
            be.sync()
            got.append(dw.result((64, Cimg, 7, 7)))
    finally:
        be.set_deterministic(0)
    if det:
        assert torch.equal(bits(got[0]), bits(got[1])), "deterministic mode: two calls differ"
    tag = "in_bwd_weight %s %dx%dx%dx%d" % (("one_wg" if det else "chunks"), B, Cimg, H, W)
    return check(tag, got[0], ref, bar, (0, 2), TOLG)


def run_in_dw_rejects(be):
    """H = 3, Cout = 32, dw = NULL: refused, dw untouched"""
    for name, (H, Cout, null) in {"H3": (3, 64, False), "Cout32": (8, 32, False), "null": (8, 64, True)}.items():
        if not null:
            assert conv7_class("in_bwd_weight", B=1, Cimg=1, H=H, W=8, Cout=Cout)["class"] == "in_bwd_weight/reject"
        x, dy = rn((1, 1, H, 8), 12900).to(be.dev), rn((1, H, 8, 64), 12901).to(be.dev)
        dw = Guard(be, 64 * 49, start=rn((64 * 49,), 12902))
        rc = be.call("conv7_in_bwd_weight", dy, x, None if null else dw.out, 1, 1, H, 8, Cout)
        assert rc != 0, name
        be.sync()
        assert dw.untouched(), name


# ----------------------------------------------------------------------------------------------------------- c. vptr_conv7_out_fwd
# fwd2: one patch; three patches in a partial workgroup with gridDim.y = 3; 2 x 2 patches.  gen1: the smallest map; odd sizes; H % 4 != 0;
# W % 16 != 0; Cimg > 4
OUT_FWD = {(1, 1, 4, 16): "fwd2", (3, 3, 4, 16): "fwd2", (1, 1, 8, 32): "fwd2",
           (1, 1, 4, 4): "gen1", (2, 3, 9, 11): "gen1", (1, 1, 6, 16): "gen1", (1, 1, 4, 12): "gen1", (1, 5, 5, 8): "gen1"}
OUT_FWD_REJECTS = {"Cin32": (1, 1, 8, 8, 32), "Cimg6": (1, 6, 8, 8, 64), "H3": (1, 1, 3, 8, 64)}


@functools.lru_cache(maxsize=4)
def _out_base(geom, Cin=64):
    """seeded inputs of one conv7_out geometry: x NHWC, w [Cimg, Cin, 7, 7] (pre-activations of order 1), bias, the upstream gradient and
    the start values of dw / db; the fp64 pre-activation and its absolute-value companion"""
    B, Cimg, H, W = geom
    seed = 13000 + 1000 * Cimg + 10 * H + W + Cin
    x, w, bias = rn((B, H, W, Cin), seed), rn((Cimg, Cin, 7, 7), seed + 1, 0.02 * (64.0 / Cin) ** 0.5), rn((Cimg,), seed + 2, 0.3)
    pre = conv_ref(nchw(x), w) + bias.double().view(1, Cimg, 1, 1)
    S = conv_ref(nchw(x).abs(), w.abs()) + bias.double().abs().view(1, Cimg, 1, 1)
    return {"x": x, "w": w, "bias": bias, "pre": pre, "S": S, "dy": rn((B, Cimg, H, W), seed + 3),
            "dw0": rn((Cimg, Cin, 7, 7), seed + 4), "db0": rn((Cimg,), seed + 5)}


def run_out_fwd(be, geom):
    """out_act 0, 1 and 2 on one geometry: the pre-activation and both activations against fp64, and the activations' own error against fp64
    tanh / sigmoid of the out_act = 0 output of the same backend.  Returns {act: worst relative activation error}"""
    B, Cimg, H, W = geom
    cls = conv7_class("out_fwd", B=B, Cimg=Cimg, H=H, W=W)
    assert cls["class"] == "out_fwd/" + OUT_FWD[geom], cls
    G, dev = _out_base(geom), be.dev
    xd, wd, bd = G["x"].to(dev), G["w"].to(dev), G["bias"].to(dev)
    pre_bar = (49 + 6 + 1) * U * G["S"]
    got, measured = {}, {}
    for act in (NONE, TANH, SIGMOID):
        y = Guard(be, B * Cimg * H * W)
        rc = be.call("conv7_out_fwd", xd, wd, bd, y.out, B, 64, H, W, Cimg, act)
        assert rc == 0, (geom, act, rc)
        be.sync()
        got[act] = y.result((B, Cimg, H, W))
        ref = act64(G["pre"], act)
        bar = pre_bar * GAIN[act] + (2.0 * ACT_ERR[act] * ref.abs() if act else 0.0)
        tag = "out_fwd %s %dx%dx%dx%d act%d" % ((OUT_FWD[geom],) + geom + (act,))
        check(tag, got[act], ref, bar, (1,), TOLV)
        if act:
            own = act64(got[NONE].double(), act)
            relerr = (got[act].double() - own).abs() / own.abs()
            measured[act] = float(relerr.max())
            margin("conv7 %s activation error" % tag, measured[act], ACT_ERR[act])
            line = "conv7 %s: worst relative activation error %.3e (recorded %.3e)" % (tag, measured[act], ACT_ERR[act])
            if act == SIGMOID:
                line += ", worst error / ((|v| + 4) 2^-24) %.3f" % float((relerr / SIGMOID_EXPECTED(got[NONE].double())).max())
            print(line)
            assert measured[act] <= ACT_ERR[act], (tag, measured[act])
    return measured


def run_out_fwd_rejects(be):
    for name, (B, Cimg, H, W, Cin) in OUT_FWD_REJECTS.items():
        assert conv7_class("out_fwd", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"] == "out_fwd/reject", name
        x, w, b = rn((B, H, W, Cin), 13900).to(be.dev), rn((Cimg, Cin, 7, 7), 13901, 0.02).to(be.dev), rn((Cimg,), 13902).to(be.dev)
        y = Guard(be, B * Cimg * H * W)
        rc = be.call("conv7_out_fwd", x, w, b, y.out, B, Cin, H, W, Cimg, TANH)
        assert rc != 0, name
        be.sync()
        assert y.untouched(), name


# ------------------------------------------------------------------------------------------------------ d. vptr_conv7_out_bwd_data
# (B, Cimg, H, W, Cin) -> class.  data2 (W = 64): H = 7 (row 3 has both mirror images), one whole band, a second band of one row, a partial
# third band; Cimg = 3, and its LDS limit H = 73.  gen1: H = 74 just past that limit; both mirror images in both directions; odd sizes; W = 128;
# ngrp = 2 and 8
OUT_DX = {(1, 1, 7, 64, 64): "data2", (1, 1, 8, 64, 64): "data2", (1, 1, 9, 64, 64): "data2", (1, 1, 20, 64, 64): "data2", (1, 3, 9, 64, 64): "data2",
          (1, 3, 73, 64, 64): "data2", (1, 3, 74, 64, 64): "gen1", (2, 1, 7, 7, 64): "gen1", (1, 3, 9, 11, 64): "gen1", (1, 1, 8, 128, 64): "gen1",
          (1, 2, 8, 8, 32): "gen1", (1, 2, 8, 8, 128): "gen1"}
OUT_DX_REJECTS = {"H6": (1, 1, 6, 8, 64), "W6": (1, 1, 8, 6, 64), "Cin24": (1, 1, 8, 8, 24), "Cin48": (1, 1, 8, 8, 48)}
ACTS = (NONE, TANH, SIGMOID)


def _y32(G, act):
    """y as the backward calls receive it: the fp32 rounding of the fp64 forward"""
    return act64(G["pre"], act).float()


def run_out_dx(be, geom, act):
    B, Cimg, H, W, Cin = geom
    cls = conv7_class("out_bwd_data", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)
    assert cls["class"] == "out_bwd_data/" + OUT_DX[geom], cls
    G, dev = _out_base(geom[:4], Cin), be.dev
    y = _y32(G, act)
    g = act_grad64(G["dy"], y, act)
    zero = torch.zeros((B, Cin, H, W))
    ref, _ = conv_grads(zero, G["w"], g)
    S, _ = conv_grads(zero, G["w"].abs(), g.abs())
    dx = Guard(be, B * H * W * Cin)
    rc = be.call("conv7_out_bwd_data", G["dy"].to(dev), y.to(dev), G["w"].to(dev), dx.out, B, Cin, H, W, Cimg, act)
    assert rc == 0, (geom, rc)
    be.sync()
    tag = "out_bwd_data %s %dx%dx%dx%d Cin%d act%d" % ((OUT_DX[geom],) + geom + (act,))
    return check(tag, dx.result((B, H, W, Cin)), nhwc(ref), (4 * 49 * Cimg + 4) * U * nhwc(S), (3,), TOLG)


def run_out_dx_rejects(be):
    for name, (B, Cimg, H, W, Cin) in OUT_DX_REJECTS.items():
        assert conv7_class("out_bwd_data", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"] == "out_bwd_data/reject", name
        dy, y, w = rn((B, Cimg, H, W), 14900).to(be.dev), rn((B, Cimg, H, W), 14901, 0.3).to(be.dev), rn((Cimg, Cin, 7, 7), 14902, 0.02).to(be.dev)
        dx = Guard(be, B * H * W * Cin)
        rc = be.call("conv7_out_bwd_data", dy, y, w, dx.out, B, Cin, H, W, Cimg, TANH)
        assert rc != 0, name
        be.sync()
        assert dx.untouched(), name


# ------------------------------------------------------------------------------- e. vptr_conv7_out_bwd_weight and its _ws form
# plain: fpb = 4 with one frame and with a ragged second workgroup row; fpb = 16 whole and ragged
OUT_DW = {(1, 1, 8, 8): "fpb4", (5, 3, 8, 16): "fpb4", (64, 1, 8, 8): "fpb16", (65, 3, 8, 8): "fpb16"}
OUT_DW_REJECTS = {"H12": (1, 1, 12, 8), "Cimg4": (1, 4, 8, 8)}
# _ws: 3, 12, 15, 18 and 33 partials (the reduction's unrolled loop not at all, not at all, for three of the four thread groups, once with a tail,
# twice with a tail); sizes that are no multiple of 8; a tile above 64 KB
OUT_WS = {(1, 1, 8, 8): "ws", (4, 1, 8, 8): "ws", (5, 1, 8, 8): "ws", (6, 1, 8, 8): "ws", (11, 1, 8, 8): "ws", (2, 3, 9, 11): "ws", (1, 3, 10, 8): "ws",
          (2, 1, 16, 24): "ws", (1, 1, 8, 2048): "ws_attr"}
OUT_WS_FALLBACKS = {"null": (2, 3, 8, 16), "short": (2, 3, 8, 16), "lds": (1, 1, 8, 4096)}


@functools.lru_cache(maxsize=2)
def _out_dw_ref(geom, act):
    B, Cimg, H, W = geom
    G = _out_base(geom)
    y = _y32(G, act)
    g = act_grad64(G["dy"], y, act)
    zero = torch.zeros((Cimg, 64, 7, 7))
    _, dw = conv_grads(nchw(G["x"]), zero, g)
    _, Sw = conv_grads(nchw(G["x"]).abs(), zero, g.abs())
    n = B * H * W + 3
    return {"y": y, "dw": G["dw0"].double() + dw, "dw_bar": n * U * Sw + U * G["dw0"].double().abs(),
            "db": G["db0"].double() + g.sum((0, 2, 3)), "db_bar": n * U * g.abs().sum((0, 2, 3)) + U * G["db0"].double().abs()}


def _out_dw_call(be, geom, act, ws=None, with_db=True, ws_shift=0, ws_short=0):
    """one weight-gradient call from the seeded start values; ws: None = the plain entry point, "null" = the _ws entry point with a NULL
    workspace, True = with a guarded workspace (ws_short floats less declared and allocated).  Returns (rc, dw, db, workspace) guards"""
    B, Cimg, H, W = geom
    G, dev = _out_base(geom), be.dev
    R = _out_dw_ref(geom, act)
    dw, db = Guard(be, Cimg * 64 * 49, start=G["dw0"]), Guard(be, Cimg, start=G["db0"])
    args = [G["dy"].to(dev), R["y"].to(dev), G["x"].to(dev), dw.out, db.out if with_db else None, B, 64, H, W, Cimg, act]
    wsg = None
    if ws is None:
        rc = be.call("conv7_out_bwd_weight", *args)
    elif ws == "null":
        rc = be.call("conv7_out_bwd_weight_ws", *(args + [None, 0]))
    else:
        n = be.workspace_floats(B, Cimg) - ws_short
        wsg = Guard(be, n, shift=ws_shift)
        rc = be.call("conv7_out_bwd_weight_ws", *(args + [wsg.out, n]))
    be.sync()
    return rc, dw, db, wsg


def _out_dw_check(tag, geom, act, dw, db, with_db=True):
    B, Cimg, H, W = geom
    R = _out_dw_ref(geom, act)
    out = check(tag + " dw", dw.result((Cimg, 64, 7, 7)), R["dw"], R["dw_bar"], (0, 2), TOLG)
    if with_db:
        check(tag + " db", db.result((Cimg,)), R["db"], R["db_bar"], (0,), None)
    else:
        assert db.untouched(), tag
    return out


def run_out_dw(be, geom, act):
    B, Cimg, H, W = geom
    cls = conv7_class("out_bwd_weight", B=B, Cimg=Cimg, H=H, W=W)
    assert cls["class"] == "out_bwd_weight/" + OUT_DW[geom], cls
    rc, dw, db, _ = _out_dw_call(be, geom, act)
    assert rc == 0, (geom, rc)
    return _out_dw_check("out_bwd_weight %s %dx%dx%dx%d act%d" % ((OUT_DW[geom],) + geom + (act,)), geom, act, dw, db)


def run_out_dw_rejects(be):
    for name, geom in OUT_DW_REJECTS.items():
        B, Cimg, H, W = geom
        assert conv7_class("out_bwd_weight", B=B, Cimg=Cimg, H=H, W=W)["class"] == "out_bwd_weight/reject", name
        rc, dw, db, _ = _out_dw_call(be, geom, TANH)
        assert rc != 0, name
        assert dw.untouched() and db.untouched(), name


def run_out_ws(be, geom, act, det, with_db=True):
    """the workspace form, twice from the same start: dw within its bars and bit-identical across the two calls in either mode, db within its
    bars and bit-identical in deterministic mode; the canary behind the workspace intact"""
    B, Cimg, H, W = geom
    cls = conv7_class("out_bwd_weight_ws", B=B, Cimg=Cimg, H=H, W=W)
    assert cls["class"] == "out_bwd_weight_ws/" + OUT_WS[geom] and cls["partials"] == 3 * B, cls
    tag = "out_bwd_weight_ws %s %dx%dx%dx%d act%d %s%s" % ((OUT_WS[geom],) + geom + (act, "det" if det else "atomic", "" if with_db else " no db"))
    runs = []
    be.set_deterministic(det)
    try:
        for _ in range(2):
            rc, dw, db, wsg = _out_dw_call(be, geom, act, ws=True, with_db=with_db)
            assert rc == 0, (tag, rc)
            assert wsg.intact(), tag + ": write outside the workspace"
            runs.append((dw, db))
    finally:
        be.set_deterministic(0)
    out = _out_dw_check(tag, geom, act, runs[0][0], runs[0][1], with_db)
    _out_dw_check(tag + " (second call)", geom, act, runs[1][0], runs[1][1], with_db)
    assert torch.equal(runs[0][0].words(), runs[1][0].words()), tag + ": dw differs between two calls"
    if det and with_db:
        assert torch.equal(runs[0][1].words(), runs[1][1].words()), tag + ": db differs between two deterministic calls"
    return out


def run_out_ws_fallback(be, name):
    """NULL workspace, a workspace one float short, a tile above 150 KB: the plain entry point's result (within the same bars), the workspace
    untouched"""
    geom = OUT_WS_FALLBACKS[name]
    B, Cimg, H, W = geom
    nfl = be.workspace_floats(B, Cimg)
    cls = conv7_class("out_bwd_weight_ws", B=B, Cimg=Cimg, H=H, W=W, ws_floats={"null": None, "short": nfl - 1, "lds": nfl}[name])
    assert cls["class"] == "out_bwd_weight_ws/fallback" and cls["reason"] == name, cls
    rc, dw, db, wsg = _out_dw_call(be, geom, TANH, ws="null" if name == "null" else True, ws_short=1 if name == "short" else 0)
    assert rc == 0, (name, rc)
    assert wsg is None or wsg.untouched(), name
    out = _out_dw_check("out_bwd_weight_ws fallback %s %dx%dx%dx%d" % ((name,) + geom), geom, TANH, dw, db)
    rc, dwp, dbp, _ = _out_dw_call(be, geom, TANH)                 # the plain entry point itself: two results inside one bar are within two bars
    assert rc == 0, (name, rc)
    R = _out_dw_ref(geom, TANH)
    assert bool(((dw.result((Cimg, 64, 7, 7)).double() - dwp.result((Cimg, 64, 7, 7)).double()).abs() <= 2.0 * R["dw_bar"]).all()), name
    assert bool(((db.result((Cimg,)).double() - dbp.result((Cimg,)).double()).abs() <= 2.0 * R["db_bar"]).all()), name
    return out


def run_out_ws_rejects(be):
    """a workspace 4 bytes off a 16-byte boundary; Cimg = 4 (the fallback's own refusal included: H = 12 without a workspace)"""
    for name, geom, kw in (("off4", (1, 1, 8, 8), dict(ws=True, ws_shift=1)), ("Cimg4", (1, 4, 8, 8), dict(ws=True)), ("H12_null", (1, 1, 12, 8), dict(ws="null"))):
        B, Cimg, H, W = geom
        cls = conv7_class("out_bwd_weight_ws", B=B, Cimg=Cimg, H=H, W=W, aligned=name != "off4", **({"ws_floats": None} if kw["ws"] == "null" else {}))
        assert cls["class"] == "out_bwd_weight_ws/reject", (name, cls)
        rc, dw, db, wsg = _out_dw_call(be, geom, TANH, **kw)
        assert rc != 0, name
        assert dw.untouched() and db.untouched() and (wsg is None or wsg.untouched()), name


# ------------------------------------------------------------------------------------------------------------------------ census
def class_census():
    """class -> the cases that name it (tests/test_cpu.py: every class of helpers.CONV7_CLASSES is reached)"""
    out = {}

    def add(cls, case):
        out.setdefault(cls, []).append(case)
    for g, c in IN_FWD.items():
        add("in_fwd/" + c, g)
    for g, c in IN_PLANES.items():
        add("in_fwd_planes/" + c, g)
    for c in in_dw_cases():
        add("in_bwd_weight/" + ("one_wg" if c[4] else "chunks"), c)
    for g, c in OUT_FWD.items():
        add("out_fwd/" + c, g)
    for g, c in OUT_DX.items():
        add("out_bwd_data/" + c, g)
    for g, c in OUT_DW.items():
        add("out_bwd_weight/" + c, g)
    for g, c in OUT_WS.items():
        add("out_bwd_weight_ws/" + c, g)
    for k in OUT_WS_FALLBACKS:
        add("out_bwd_weight_ws/fallback", k)
    for op, table in (("in_fwd", IN_FWD_REJECTS), ("in_fwd_planes", IN_PLANES_REJECTS), ("out_fwd", OUT_FWD_REJECTS), ("out_bwd_data", OUT_DX_REJECTS),
                      ("out_bwd_weight", OUT_DW_REJECTS)):
        for k in table:
            add(op + "/reject", k)
    add("in_bwd_weight/reject", "H3")
    add("out_bwd_weight_ws/reject", "off4")
    return out
