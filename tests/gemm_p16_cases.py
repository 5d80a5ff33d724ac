"""Case runner of tests/test_01b_gemm_p16_abi_gpu.py: the nt P16 GEMM (vptr_gemm with a_mode = VPTR_A_P16, b_mode = VPTR_B_P16; csrc/gemm_p16.hip,
csrc/gemm_shared.h) called through the C ABI in each of its twelve launch classes -- EPI 1 .. 4 x NST 2 / 4 and EPI 0 x {batched-4, rows-halves-2,
serial-2, serial-4} -- and compared PER ELEMENT with the fp64 product of the decoded operands.

The runner talks to a BACKEND, as tests/convffn_fwd_cases.py does: `gemm(d)` takes a descriptor as a dict of vptr_gemm_desc members (tensors for
pointers: 1-D views that start at the address) and returns the return code, `last_error()` the library's message, `cus` the compute units of the
device (the launcher takes NST = 4 iff tiles <= cus), `mm64(a, b)` the fp64 pair (a . b^T, |a| . |b|^T).  The GPU file's backend fills a GemmDesc
and calls vptr_gemm; `EmuBackend` below emulates the call on the CPU (tests/test_cpu.py runs every case against it, and against named MUTATIONS
of it, each of which has to make a case fail).  Operands are encoded with helpers.p16_encode, never with vptr_to_p16.

Bars.  ref = fp64 product of the decoded operands, S_ij = sum_k |a_ik| |b_jk| over all segments, u = 2^-23.
  accumulator   (2^-18 + (32 + 3 nk nseg) u) S: 2^-18 for the dropped lo . lo term (|lo| <= 2^-9 |x|), the rest 3 nk nseg MFMA accumulations
                of at most 32 products each at one truncation each.
  epilogue      the accumulator bar times the first-order gains (|colscale|, |alpha|, 1.13 >= |GELU'|, |rowscale|, 1 / keep), plus u times the
                sum of the magnitudes of the epilogue's intermediate values.  u is twice the rounding of one fp32 operation, so the sum holds
                as long as the gain between an intermediate and the output stays below 2: the cases keep |rowscale| / keep < 1.7.
                GELU is evaluated by vptr_phi (csrc/common.h): eight intermediates of magnitude <= 1 on the way to Phi (|x| / sqrt 2 scaled,
                the reciprocal, the exponential and its squared argument, the polynomial, the product, the complement), then x Phi: 8 |x| + |g|
                join the sum; for GELU' = Phi + x phi the term is |v| (8 + 4 |x| + |x phi| + |g'|) with v the value it multiplies.
  P16 output    + 2^-16 |ref|.
  rows, columns rel-L2 of every row and of every column < TOL3 = 3e-5; one whose reference norm is below 1e-3 of the median is compared
                absolutely against the median.
Elements where ReLU, act_after or a ReLU / LeakyReLU gradient sees |pre| within its own bar (kinks) are left out of the value check only; no
case may leave out more than KINK_SHARE of its elements."""
import numpy as np
import torch

from helpers import drop_scale_emu, gemm_p16_class, margin, p16_encode
from oracle import fill

TOL3 = 3e-5
U = 2.0 ** -23
KINK_SHARE = 0.01
STRIDE = 32                      # VPTR_FRAME_STATS_STRIDE
OUT_CANARY = 0x7FC01234          # quiet NaN with a payload: everything a call may not write
IN_NAN = 0x7FC07FC0              # NaN as fp32 and as both bf16 halves: pitch gaps and slack of the inputs
SLACK = 64                       # floats in front of and behind every buffer
NONE, GELU, RELU, LRELU = 0, 1, 2, 3
DROP_P, SITE, SEED = 0.1, 11, 0x0123456789ABCDEF
EMU_CUS = 16                     # compute units of the emulated device

CLASSES = [(e, n, "batched") for e in (1, 2, 3, 4) for n in (2, 4)] + [(0, 4, "batched"), (0, 2, "rows_halves"), (0, 2, "serial"), (0, 4, "serial")]


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ geometries
def geom(gid, cus):
    """(M, N, K).  g*: at most `cus` tiles of 128 x 176 (NST = 4); n*: more (NST = 2)"""
    return {
        "g10": (10, 16, 16), "g129": (129, 192, 48), "g257": (257, 352, 80), "g200": (200, 100, 64), "g300": (300, 528, 144), "g128": (128, 176, 2112),
        "g64a": (64, 176, 32), "g64b": (64, 176, 96), "g64c": (64, 176, 128), "g192": (192, 192, 48), "g129n50": (129, 50, 48), "g129n48": (129, 48, 48),
        "n1": (128 * cus + 1, 16, 16), "n72": (128 * cus + 72, 176, 48), "n130": (64 * cus + 130, 192, 80), "n5": (32 * cus + 5, 544, 528),
        "n192": (128 * (cus // 2) + 64, 192, 48), "n1n50": (128 * cus + 1, 50, 48), "n1n48": (128 * cus + 1, 48, 48),
        "sb4": (10, 32, 48), "sb2": (10, 32, 48),
    }[gid]


# variant -> options.  epi / fn: the class the variant must reach (fn of EPI 0: "vec" = batched under NST 4, rows_halves under NST 2).
# Unless `tight`, every pitch is wider than its row: lda = K + 16, ldb = K + 32, ldd = N + 8 (N + 16 for a P16 output), ldr = N + 4.
V = {
    # EPI 1
    "e1_bias_alpha": dict(epi=1, alpha=0.75),
    "e1_tight": dict(epi=1, alpha=0.75, tight=True),
    "e1_res": dict(epi=1, alpha=0.75, res=True),
    "e1_alias": dict(epi=1, res=True, alias=True),
    "e1_p16": dict(epi=1, alpha=0.75, res=True, p16=True),
    "e1_batch2": dict(epi=1, batch=2, alphas=(1.5, -0.75, 0.5), nobias=(1,)),
    "e1_batch3": dict(epi=1, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(0,)),
    "e1_accum6": dict(epi=1, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(2,), accum=0b110),
    "e1_accum7": dict(epi=1, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(), accum=0b111),
    "e1_kseg2": dict(epi=1, ksegs=2, alpha=0.75, res=True),
    "e1_kseg3": dict(epi=1, ksegs=3, alpha=0.75, res=True),
    "e1_strided": dict(epi=1, strided=True, alpha=0.75),
    "e1_strided_p16": dict(epi=1, strided=True, alpha=0.75, p16=True),
    "e1_fs64": dict(epi=1, res=True, fs=64),
    "e1_fs192": dict(epi=1, alpha=0.75, fs=192),
    # EPI 3
    "e3_rs": dict(epi=3, bias=False, rs=True),
    "e3_drop": dict(epi=3, bias=False, drop=True),
    "e3_both": dict(epi=3, res=True, rs=True, drop=True),
    "e3_both_p16": dict(epi=3, res=True, rs=True, drop=True, p16=True),
    "e3_both_kseg3": dict(epi=3, res=True, rs=True, drop=True, ksegs=3),
    # EPI 4
    "e4_gelu": dict(epi=4, act=GELU, dpre=True, drop=True),
    "e4_relu": dict(epi=4, act=RELU, dpre=True, drop=True),
    "e4_lrelu": dict(epi=4, act=LRELU, dpre=True, drop=True),
    "e4_p16": dict(epi=4, act=GELU, dpre=True, drop=True, p16=True),
    "e4_nodpre": dict(epi=4, act=GELU),
    "e4_nobias": dict(epi=4, act=GELU, dpre=True, bias=False),
    # EPI 2
    "e2_gelu": dict(epi=2, bias=False, act=GELU, grad=True),
    "e2_relu": dict(epi=2, bias=False, act=RELU, grad=True),
    "e2_lrelu": dict(epi=2, bias=False, act=LRELU, grad=True),
    "e2_alpha": dict(epi=2, bias=False, act=GELU, grad=True, alpha=-0.5),
    "e2_drop": dict(epi=2, bias=False, act=GELU, grad=True, drop=True),
    "e2_p16": dict(epi=2, bias=False, act=GELU, grad=True, drop=True, p16=True),
    # EPI 0
    "e0_colscale": dict(epi=0, fn="vec", colscale=True, alpha=0.75),
    "e0_actafter": dict(epi=0, fn="vec", res=True, act_after=True),
    "e0_act_rs_res": dict(epi=0, fn="vec", act=GELU, rs=True, res=True),
    "e0_lrelu_rs_res": dict(epi=0, fn="vec", act=LRELU, rs=True, res=True, drop=True),
    "e0_batch3_act": dict(epi=0, fn="vec", act=GELU, batch=3, alphas=(1.5, -0.75, 0.5), nobias=(1,)),
    "e0_kseg_act": dict(epi=0, fn="vec", act=RELU, ksegs=3, res=True, rs=True),
    "e0_atomic": dict(epi=0, fn="serial", atomic=True, alpha=0.75),
    "e0_biasoff": dict(epi=0, fn="serial", biasoff=True, alpha=0.75, res=True),
    "e0_n50": dict(epi=0, fn="serial", res=True),              # alpha = 0 -> 1: the serial epilogue's plain branch
}
SWEEP4 = ("g10", "g129", "g257", "g200", "g300", "g128", "g64a", "g64b", "g64c")
SWEEP2 = ("n1", "n72", "n130", "n5")


def _cases():
    out = []
    for name, o in V.items():
        if name == "e1_bias_alpha":
            gs = SWEEP4 + SWEEP2
        elif name == "e1_tight":
            gs = ("g129", "g300", "n72")
        elif o.get("strided"):
            gs = ("sb4", "sb2")
        elif o.get("fs"):
            gs = ("g192", "n192")
        elif name == "e0_n50":
            gs = ("g129n50", "n1n50")
        elif name == "e0_biasoff":
            gs = ("g129n48", "n1n48")
        elif o.get("ksegs"):
            gs = ("g129", "n72", "n130")          # K % 32 == 16 in every segment
        else:
            gs = ("g129", "n130")
        out += ["%s-%s" % (name, g) for g in gs]
    return out


CASES = _cases()
REJECTS = list(range(1, 16))     # one per VPTR_CHECK of vptr_gemm_p16_launch, in source order


# ------------------------------------------------------------------------------------------------------------------ guarded buffers
class _Fake:
    """a pointer that is never dereferenced (class census without buffers)"""
    n = [0]

    def __init__(self, shift):
        _Fake.n[0] += 1
        self.addr = (_Fake.n[0] << 20) + 4 * (SLACK + shift)

    def data_ptr(self):
        return self.addr


class Buf:
    """[rows, cols] fp32 words at pitch ld inside a buffer that holds `canary` everywhere else: SLACK floats in front and behind, the pitch
    gaps, `extra` rows beyond the last and every row not in live_rows.  data: callable -> [len(live_rows), cols] or None (a pure output)"""

    def __init__(self, be, rows, cols, ld, canary, data=None, extra=2, shift=0, live_rows=None):
        self.rows, self.cols, self.ld, self.shift = rows, cols, ld, shift
        self.live_rows = live_rows
        if be.dry:
            self.ptr = _Fake(shift)
            return
        assert ld >= cols
        host = torch.full((2 * SLACK + (rows + extra) * ld + 4,), canary, dtype=torch.int32)
        self.mask = torch.zeros(host.shape, dtype=torch.bool)
        mm = self._mat(self.mask)
        if live_rows is None:
            mm[:] = True
        else:
            mm[live_rows] = True
        if data is not None:
            m = self._mat(host.view(torch.float32))
            val = data()
            if live_rows is None:
                m.copy_(val)
            else:
                m[live_rows] = val
        self.before = host
        self.buf = host.clone().to(be.dev)
        assert self.buf.data_ptr() % 64 == 0
        self.ptr = self.buf.view(torch.float32)[SLACK + shift:]

    def _mat(self, flat):
        return flat[SLACK + self.shift:].as_strided((self.rows, self.cols), (self.ld, 1))

    def live(self):
        m = self._mat(self.buf.cpu().view(torch.float32))
        return (m if self.live_rows is None else m[self.live_rows]).clone()

    def guards_intact(self):
        now = self.buf.cpu()
        return torch.equal(now[~self.mask], self.before[~self.mask])

    def unchanged(self):
        return torch.equal(self.buf.cpu(), self.before)


def p16_planes(t):
    """[rows, C] P16 words -> (hi, lo) as fp32 [rows, C]"""
    rows, C = t.shape
    b = t.contiguous().view(torch.bfloat16).view(rows, C // 16, 2, 16).float()
    return b[:, :, 0].reshape(rows, C), b[:, :, 1].reshape(rows, C)


def p16_decode(t):
    hi, lo = p16_planes(t)
    return hi + lo           # exact: two 8-bit significands at least 8 bits apart


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ activations
def act64(x, act):
    if act == GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == RELU:
        return torch.relu(x)
    if act == LRELU:
        return torch.where(x > 0, x, f32(0.2) * x)
    return x


def phi64(x):
    return torch.exp(-0.5 * x * x) * 0.3989422804014327


def act_grad64(h, act):
    if act == GELU:
        return 0.5 * (1.0 + torch.erf(h * 0.7071067811865476)) + h * phi64(h)
    if act == RELU:
        return (h > 0).to(h.dtype)
    if act == LRELU:
        return torch.where(h > 0, torch.ones_like(h), torch.full_like(h, f32(0.2)))
    return torch.ones_like(h)


# ------------------------------------------------------------------------------------------------------------------ CPU emulation
MUTATIONS = ("tail_not_zeroed", "seg3_reads_seg2", "col_plus4", "drop_index_ldd", "rs_div_ignored", "accum_ignored", "dpre_after_act",
             "grad_src_pitch_n", "p16_without_lo")


def fields_of(d):
    return {k: (v.data_ptr() if hasattr(v, "data_ptr") else v) for k, v in d.items() if v is not None}


class EmuBackend:
    """CPU emulation of vptr_gemm on P16 operands: the operands decoded into their bf16 planes, al . bh + ah . bl + ah . bh per 32-wide K-step in
    fp32 and in that order, steps and segments in order (the second granule of a tail step contributes nothing), the epilogue in fp32 in the
    order of include/vptr_hip.h, honouring M, N, the pitches, batch members, segments, batch_accum, the strided form, d_p16, frame_stats,
    act_grad_src and the launcher's refusals (helpers.gemm_p16_class).  mut: one of MUTATIONS"""
    dev, dry = "cpu", False

    def __init__(self, cus=EMU_CUS, mut=None):
        assert mut is None or mut in MUTATIONS
        self.cus, self.mut, self.err = cus, mut, ""

    def sync(self):
        pass

    def last_error(self):
        return self.err

    def mm64(self, a, b):
        a, b = a.double(), b.double()
        return a @ b.t(), a.abs() @ b.abs().t()

    def _acc(self, segs, M, N, K, lda, ldb):
        nk, acc = (K + 31) // 32, torch.zeros((M, N))
        for si, (Ap, Bp) in enumerate(segs):
            if self.mut == "seg3_reads_seg2" and si == 2:
                Ap, Bp = segs[1]
            ah, al = p16_planes(Ap.as_strided((M, K), (lda, 1)))
            bh, bl = p16_planes(Bp.as_strided((N, K), (ldb, 1)))
            for kt in range(nk):
                lo, hi = 32 * kt, min(32 * kt + 32, K)
                xs = [t[:, lo:hi] for t in (ah, al, bh, bl)]
                if hi - lo == 16 and self.mut == "tail_not_zeroed":       # the DMA's re-fetched first granule, left in the fragments
                    xs = [torch.cat((x, x), 1) for x in xs]
                acc = acc + xs[1] @ xs[2].t()
                acc = acc + xs[0] @ xs[3].t()
                acc = acc + xs[0] @ xs[2].t()
        return acc

    def gemm(self, d):
        g = lambda k, dflt=0: d[k] if d.get(k) is not None else dflt
        M, N, K = g("M"), g("N"), g("K")
        if min(M, N, K) <= 0 or d.get("A") is None or d.get("B") is None or d.get("D") is None or g("d_row_w"):
            self.err = "emulation: empty problem or null operand"
            return -1
        cls = gemm_p16_class(fields_of(d), self.cus)
        if cls[0] == "refuse":
            self.err = "emulation: refused by check %d" % cls[1]
            return -1
        lda, ldb, ldd, ldr = g("lda"), g("ldb"), g("ldd"), g("ldr")
        batch, ksegs, mut = max(g("batch"), 1), max(g("ksegs"), 1), self.mut
        strided, act, p = g("batch_stride_d") != 0, g("act"), f32(g("dropout_p"))
        rows, cols = torch.arange(M), torch.arange(N)
        vec = cls[2] != "serial"
        for m in range(batch):
            sfx = "" if m == 0 or strided else "_x%d" % m
            A, B, D = d["A" + sfx], d["B" + sfx], d["D" + sfx]
            bias, alpha = d.get("bias" + sfx), g("alpha" + sfx)
            if strided:
                A, B, D = A[m * d["batch_stride_a"]:], B[m * d["batch_stride_b"]:], D[m * d["batch_stride_d"]:]
            segs = [(d["A"], d["B"]), (d.get("A_x1"), d.get("B_x1")), (d.get("A_x2"), d.get("B_x2"))][:ksegs] if ksegs > 1 else [(A, B)]
            v = self._acc(segs, M, N, K, lda, ldb)
            if d.get("colscale") is not None:
                v = v * d["colscale"][:N]
            if bias is not None and d.get("act_grad_src") is None:
                v = v + bias[:N]
            v = v * torch.tensor(alpha if alpha != 0 else 1.0, dtype=torch.float32)
            Dm = D.as_strided((M, N), (ldd, 1))
            ok = ((cols - cols % 4 if vec else cols) + 4 <= N) if mut == "col_plus4" else torch.ones(N, dtype=torch.bool)
            if d.get("act_grad_src") is not None:
                h = d["act_grad_src"].as_strided((M, N), (N if mut == "grad_src_pitch_n" else ldd, 1))
                t = v * act_grad64(h, act).float()
            else:
                t = act64(v, act).float()
                if d.get("Dpre") is not None:
                    d["Dpre"].as_strided((M, N), (ldd, 1))[:, ok] = (t if mut == "dpre_after_act" else v)[:, ok]
                if d.get("rowscale") is not None:
                    t = t * d["rowscale"][((rows if mut == "rs_div_ignored" else rows // d["rs_div"]) % d["rs_mod"])][:, None]
            if p > 0:
                idx = rows[:, None] * (ldd if mut == "drop_index_ldd" else N) + cols[None, :]
                t = t * drop_scale_emu(int(d["seed_dev"][0]), g("site"), idx, p)
            res = None
            if m == 0 and d.get("residual") is not None:
                res = d["residual"].as_strided((M, N), (ldr, 1))
            if (g("batch_accum") >> m) & 1 and mut != "accum_ignored":
                res = Dm
            t = t + (res.clone() if res is not None else 0.0)
            if g("act_after"):
                t = torch.relu(t)
            if g("atomic"):
                t = Dm + t
            if g("d_p16"):
                enc = p16_encode(t.contiguous())
                if mut == "p16_without_lo":
                    e = enc.view(torch.bfloat16).view(M, N // 16, 2, 16).clone()
                    e[:, :, 1] = 0
                    enc = e.view(M, 2 * N).view(torch.float32)
                Dm.copy_(enc)
            else:
                Dm[:, ok] = t[:, ok]
            if d.get("frame_stats") is not None:
                fr, td = g("frame_rows"), t.double()
                for f in range(-(-M // fr)):
                    blk = td[f * fr:(f + 1) * fr]
                    d["frame_stats"][STRIDE * f] += float(blk.sum())
                    d["frame_stats"][STRIDE * f + 1] += float((blk * blk).sum())
        return 0


class DryBackend:
    """no buffers at all: descriptors with made-up addresses of the right alignment, for the class census"""
    dev, dry = "cpu", True

    def __init__(self, cus):
        self.cus = cus


# ------------------------------------------------------------------------------------------------------------------ operands
_PAIRS = {}


def _pair(be, M, N, K, seed, scale):
    """one seeded operand pair: the P16 words of A [M, K] and B [N, K] and the fp64 product / absolute product of the DECODED operands"""
    key = (type(be).__name__, M, N, K, seed, scale)
    if key not in _PAIRS:
        while len(_PAIRS) >= 6:
            _PAIRS.pop(next(iter(_PAIRS)))
        Ae, Be = p16_encode(rn((M, K), seed)), p16_encode(rn((N, K), seed + 1, scale))
        acc, S = be.mm64(p16_decode(Ae), p16_decode(Be))
        _PAIRS[key] = (Ae, Be, acc, S)
    return _PAIRS[key]


# ------------------------------------------------------------------------------------------------------------------ building a call
def build(be, cid):
    """the descriptor of a case with all its buffers.  Returns a dict: d (the descriptor), cls (the class it must reach), outs (one entry per
    output matrix with what its reference needs), inputs (buffers the call must not write)"""
    name, gid = cid.rsplit("-", 1)
    o, cus, dry = V[name], be.cus, be.dry
    M, N, K = geom(gid, cus)
    nst = 4 if gid[0] in "gs" and gid != "sb2" else 2
    tight, p16 = o.get("tight", False), o.get("p16", False)
    lda, ldb = (K, K) if tight else (K + 16, K + 32)
    ldd = N if tight else N + (16 if p16 else 8)
    ldr = ldd if o.get("alias") else (N if tight else N + 4)
    batch, ksegs, strided = o.get("batch", 1), o.get("ksegs", 1), o.get("strided", False)
    seed0 = 100 * (sorted(V).index(name) + 1)
    d = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldd=ldd, a_mode=5, b_mode=3, precision=3, split_k=1, alpha=o.get("alpha", 0.0), act=o.get("act", NONE))
    inputs, outs = [], []

    def inp(rows, cols, ld, data, **kw):
        b = Buf(be, rows, cols, ld, IN_NAN, data, **kw)
        inputs.append(b)
        return b

    if strided:
        nb = 3 if gid == "sb4" else cus + 1
        Mpad = 16
        lr = torch.cat([torch.arange(M) + i * Mpad for i in range(nb)])
        if not dry:
            Ae = p16_encode(rn((nb * M, K), seed0))
            Be = p16_encode(rn((nb * N, K), seed0 + 1, K ** -0.5))
            Ad, Bd = p16_decode(Ae).double().view(nb, M, K), p16_decode(Be).double().view(nb, N, K)
            acc = torch.bmm(Ad, Bd.transpose(1, 2)).reshape(nb * M, N)
            S = torch.bmm(Ad.abs(), Bd.abs().transpose(1, 2)).reshape(nb * M, N)
        Ab = inp(nb * Mpad, K, lda, None if dry else (lambda: Ae), live_rows=lr)
        Bb = inp(nb * N, K, ldb, None if dry else (lambda: Be))
        Db = Buf(be, nb * Mpad, N, ldd, OUT_CANARY, live_rows=lr)
        biasb = inp(1, N, N, lambda: rn((1, N), seed0 + 2))
        d.update(A=Ab.ptr, B=Bb.ptr, D=Db.ptr, bias=biasb.ptr, batch=nb, batch_stride_a=Mpad * lda, batch_stride_b=N * ldb, batch_stride_d=Mpad * ldd,
                 d_p16=int(p16))
        outs.append(dict(D=Db, acc=None if dry else acc, S=None if dry else S, alpha=o["alpha"], bias=biasb, rows=nb * M, nseg=1))
        tiles = nb
    else:
        count = max(batch, ksegs)
        scale = (ksegs * K) ** -0.5
        prs = [None if dry else _pair(be, M, N, K, seed0 + 10 * i, scale) for i in range(count)]
        Abs = [inp(M, K, lda, None if dry else (lambda i=i: prs[i][0])) for i in range(count)]
        Bbs = [inp(N, K, ldb, None if dry else (lambda i=i: prs[i][1])) for i in range(count)]
        for i in range(count):
            sfx = "" if i == 0 else "_x%d" % i
            d["A" + sfx], d["B" + sfx] = Abs[i].ptr, Bbs[i].ptr
        d.update(batch=batch if batch > 1 else 0, ksegs=ksegs if ksegs > 1 else 0, d_p16=int(p16))
        tiles = -(-M // 128) * -(-N // 176) * batch
        alphas = o.get("alphas", (o.get("alpha", 0.0),))
        for m in range(batch):
            sfx = "" if m == 0 else "_x%d" % m
            has_bias = o.get("bias", True) and m not in o.get("nobias", ())
            biasb = None
            if has_bias:
                sh = 1 if o.get("biasoff") else 0
                biasb = inp(1, N, N, lambda m=m: rn((1, N), seed0 + 3 + m), shift=sh)
                d["bias" + sfx] = biasb.ptr
            if m > 0:
                d["alpha" + sfx] = alphas[m]
            elif batch > 1:
                d["alpha"] = alphas[0]
            pre_fill = None
            if o.get("atomic") or (o.get("accum", 0) >> m) & 1 or (o.get("alias") and m == 0):
                pre_fill = rn((M, N), seed0 + 40 + m) if not dry else None
                Db = Buf(be, M, N, ldd, OUT_CANARY, None if dry else (lambda pf=pre_fill: pf))
            else:
                Db = Buf(be, M, N, ldd, OUT_CANARY)
            d["D" + sfx] = Db.ptr
            if dry:
                acc = S = None
            elif ksegs > 1:
                acc, S = sum(pr[2] for pr in prs), sum(pr[3] for pr in prs)
            else:
                acc, S = prs[m][2], prs[m][3]
            outs.append(dict(D=Db, acc=acc, S=S, alpha=alphas[m] if batch > 1 else o.get("alpha", 0.0), bias=biasb, rows=M, nseg=ksegs, prefill=pre_fill,
                             accum=bool((o.get("accum", 0) >> m) & 1)))
        o0 = outs[0]
        if o.get("accum"):
            d["batch_accum"] = o["accum"]
        if o.get("res"):
            if o.get("alias"):
                o0["res"], d["residual"] = o0["prefill"], o0["D"].ptr
            else:
                o0["res"] = None if dry else rn((M, N), seed0 + 50)
                rb = inp(M, N, ldr, None if dry else (lambda: o0["res"]))
                d["residual"] = rb.ptr
            d["ldr"] = ldr
        if o.get("colscale"):
            o0["cs"] = inp(1, N, N, lambda: rn((1, N), seed0 + 51).abs() * 0.5 + 0.5)
            d["colscale"] = o0["cs"].ptr
        if o.get("rs"):
            rsv = rn((1, 5), seed0 + 52).abs() * 0.3 + 0.6
            rsv[0, 1] = 0.0                                   # a dropped path
            rsv = rsv.clamp(max=1.5)
            o0["rs"] = inp(1, 5, 5, lambda: rsv)
            d.update(rowscale=o0["rs"].ptr, rs_div=7, rs_mod=5)
        if o.get("drop"):
            sd = torch.tensor([SEED], dtype=torch.int64)
            d.update(dropout_p=DROP_P, site=SITE, seed_dev=sd if dry else sd.to(be.dev))
        if o.get("dpre"):
            o0["Dpre"] = Buf(be, M, N, ldd, OUT_CANARY)
            d["Dpre"] = o0["Dpre"].ptr
        if o.get("grad"):
            o0["h"] = None if dry else rn((M, N), seed0 + 53)
            if not dry and o["act"] != GELU:
                o0["h"].view(-1)[::211] = 0.0                 # exact zeros: the only kinks a gradient of exact inputs has
            d["act_grad_src"] = inp(M, N, ldd, None if dry else (lambda: o0["h"])).ptr
        if o.get("act_after"):
            d["act_after"] = 1
        if o.get("atomic"):
            d["atomic"] = 1
        if o.get("fs"):
            frames = -(-M // o["fs"])
            o0["fs"] = Buf(be, frames, 2, STRIDE, OUT_CANARY, lambda: torch.zeros((frames, 2)), extra=1)
            d.update(frame_stats=o0["fs"].ptr, frame_rows=o["fs"])
    assert (tiles <= cus) == (nst == 4), "%s: %d tiles on %d compute units do not make an NST = %d launch" % (cid, tiles, cus, nst)
    fn = o.get("fn", "batched")
    cls = (o["epi"], nst, ("batched" if nst == 4 else "rows_halves") if fn == "vec" else fn)
    got = gemm_p16_class(fields_of(d), cus)
    assert got == cls, "%s reaches %s, not %s" % (cid, got, cls)
    return dict(d=d, cls=cls, outs=outs, inputs=inputs, o=o, geom=(M, N, K), cid=cid)


def class_census(cus):
    """class -> cases that run it on a device of `cus` compute units"""
    be, out = DryBackend(cus), {c: [] for c in CLASSES}
    for cid in CASES:
        out[build(be, cid)["cls"]].append(cid)
    return out


# ------------------------------------------------------------------------------------------------------------------ reference and bars
def reference(c, out, first):
    """fp64 reference of one output matrix with its per-element bar: dict ref, bar, kink, pre, bar_pre, dropped (bool or None), res"""
    o, d = c["o"], c["d"]
    M, N, K = c["geom"]
    R = out["rows"]
    nk = (K + 31) // 32
    acc, S = out["acc"], out["S"]
    bar = (2.0 ** -18 + (32 + 3 * nk * out["nseg"]) * U) * S
    v, mags = acc, torch.zeros_like(acc)
    if first and "cs" in out:
        cs = out["cs"].live().double()
        v, bar = v * cs, bar * cs.abs()
        mags = mags + v.abs()
    if out["bias"] is not None:
        v = v + out["bias"].live().double()
        mags = mags + v.abs()
    alpha = f32(out["alpha"]) or 1.0
    v, bar = v * alpha, bar * abs(alpha)
    mags = mags + v.abs()
    pre, bar_pre = v, bar + U * mags
    kink = torch.zeros(v.shape, dtype=torch.bool)
    act = o.get("act", NONE)
    if o.get("grad"):
        h = out["h"].double()
        gp = act_grad64(h, act)
        t = v * gp
        if act == GELU:
            bar = bar * 1.13
            mags = mags + v.abs() * (8 + 4 * h.abs() + (h * phi64(h)).abs() + gp.abs())
        else:
            bar = bar * gp.abs()
            kink |= h == 0
        mags = mags + t.abs()
    else:
        t = act64(v, act)
        if act == GELU:
            bar = bar * 1.13
            mags = mags + 8 * v.abs() + t.abs()
        elif act in (RELU, LRELU):
            kink |= pre.abs() <= bar_pre
            mags = mags + t.abs()
        if first and "rs" in out:
            rs = out["rs"].live().double().view(-1)[(torch.arange(R) // 7) % 5][:, None]
            t, bar = t * rs, bar * rs.abs()
            mags = mags + t.abs()
    dropped = None
    if o.get("drop"):
        keep = drop_scale_emu(SEED, SITE, torch.arange(R)[:, None] * N + torch.arange(N)[None, :], DROP_P).double()
        dropped = keep == 0
        share = float(dropped.double().mean())
        assert 0.05 < share < 0.15, share
        t, bar = t * keep, bar * keep
        mags = mags + t.abs()
    res = out.get("res") if first else None
    if out.get("accum"):
        res = out["prefill"]
    if res is not None:
        t = t + res.double()
        mags = mags + t.abs()
    if o.get("act_after"):
        kink |= t.abs() <= bar + U * mags
        t = torch.relu(t)
    if o.get("atomic"):
        t = t + out["prefill"].double()
        mags = mags + t.abs()
    bar = bar + U * mags
    if o.get("p16"):
        bar = bar + 2.0 ** -16 * t.abs()
    return dict(ref=t, bar=bar, kink=kink, pre=pre, bar_pre=bar_pre, dropped=dropped, res=res)


def rowcol(got, ref):
    """worst rel-L2 over the rows and over the columns; a row / column whose reference norm is below 1e-3 of the median counts absolutely
    against the median"""
    worst = 0.0
    e, r = got.double() - ref, ref
    for dim in (1, 0):
        en, rn_ = e.norm(dim=dim), r.norm(dim=dim)
        med = float(rn_.median())
        den = torch.where(rn_ < 1e-3 * med, torch.full_like(rn_, med), rn_)
        worst = max(worst, float((en / den.clamp_min(1e-300)).max()))
    return worst


def check_matrix(tag, cls, got, ref, bar, kink):
    assert bool(torch.isfinite(got).all()), "%s: NaN or Inf in the output (an element that was never written keeps the canary)" % tag
    err = (got.double() - ref).abs()
    ratio = torch.where(kink, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    worst = float(ratio.max())
    i = int(ratio.reshape(-1).argmax())
    rc = rowcol(got, ref)
    share = float(kink.double().mean())
    print("%s %s: worst element error / bar %.3f at (%d, %d) (ref %.6e, got %.6e, bar %.3e); worst row / column rel-L2 %.3e; kinks %.2e"
          % (tag, cls, worst, i // ref.shape[1], i % ref.shape[1], float(ref.reshape(-1)[i]), float(got.reshape(-1)[i]), float(bar.reshape(-1)[i]), rc,
             share))
    margin("gemm_p16 %s element %s" % (cls, tag), worst, 1.0)
    margin("gemm_p16 %s rowcol %s" % (cls, tag), rc, TOL3)
    assert share <= KINK_SHARE, (tag, "kinks", share)
    assert worst <= 1.0, (tag, "element over its bar", worst, i // ref.shape[1], i % ref.shape[1])
    assert rc < TOL3, (tag, "row / column rel-L2", rc)
    return worst, rc


def run_case(be, cid):
    c = build(be, cid)
    d, o = c["d"], c["o"]
    rc = be.gemm(d)
    assert rc == 0, (cid, rc, be.last_error())
    be.sync()
    M, N, K = c["geom"]
    figures = []
    for m, out in enumerate(c["outs"]):
        tag = cid if len(c["outs"]) == 1 else "%s[%d]" % (cid, m)
        R = reference(c, out, m == 0)
        assert out["D"].guards_intact(), "%s: D written outside its %d x %d elements" % (tag, out["rows"], N)
        raw = out["D"].live()
        got = p16_decode(raw) if o.get("p16") else raw
        if R["dropped"] is not None:          # exactly the emulated pattern: a dropped element is its residual bit for bit, +0 without one
            want = R["res"].float() if R["res"] is not None else torch.zeros_like(got)
            dm = R["dropped"]
            if o.get("p16"):
                want = p16_decode(p16_encode(want.contiguous()))
            bad = int((got[dm].view(torch.int32) != want[dm].view(torch.int32)).sum())
            assert bad == 0, "%s: %d of %d dropped elements are not their residual / +0 bit for bit" % (tag, bad, int(dm.sum()))
        figures.append(check_matrix(tag, c["cls"], got, R["ref"], R["bar"], R["kink"]))
        if "Dpre" in out:
            assert out["Dpre"].guards_intact(), "%s: Dpre written outside its elements" % tag
            figures.append(check_matrix(tag + " Dpre", c["cls"], out["Dpre"].live(), R["pre"], R["bar_pre"], torch.zeros_like(R["kink"])))
        if "fs" in out:
            assert out["fs"].guards_intact(), "%s: a statistics slot beyond [frame][0 .. 1] changed" % tag
            st, fr = out["fs"].live().double(), o["fs"]
            yd = got.double()
            s0 = torch.stack([yd[f * fr:(f + 1) * fr].sum() for f in range(st.shape[0])])
            s1 = torch.stack([(yd[f * fr:(f + 1) * fr] ** 2).sum() for f in range(st.shape[0])])
            sa = max(float(yd[f * fr:(f + 1) * fr].abs().sum()) for f in range(st.shape[0]))
            v1, v0 = float(((st[:, 1] - s1).abs() / s1).max()), float((st[:, 0] - s0).abs().max()) / sa
            print("%s: frame sums |err| / max sum|y| %.3e, sums of squares rel %.3e" % (tag, v0, v1))
            assert v1 < 1e-6 and v0 < 1e-6, (tag, v0, v1)       # the bounds of test_01::test_frame_stats_from_producers
    for b in c["inputs"]:
        assert b.unchanged(), "%s: an input of the call changed" % cid
    if o.get("drop"):
        assert int(d["seed_dev"].cpu()[0]) == SEED, "%s: the seed word changed" % cid
    return c["cls"], figures


# ------------------------------------------------------------------------------------------------------------------ rejections
def run_reject(be, k):
    """a valid EPI 1 descriptor at 129 x 192 x 48 bent so that the k-th VPTR_CHECK of vptr_gemm_p16_launch refuses it: negative return code,
    a message, every output canary intact, and the mirror refuses at the same check"""
    c = build(be, "e1_res-g129")
    d, outs = dict(c["d"]), list(c["outs"])
    M, N, K = c["geom"]
    extra_out = []

    def out_buf():
        b = Buf(be, M, N, d["ldd"], OUT_CANARY)
        extra_out.append(b)
        return b.ptr

    if k == 1:
        d["b_mode"] = 0
    elif k == 2:
        d["K"] = 40
    elif k == 3:
        d["split_k"] = 2
    elif k == 4:
        d.update(batch=2, batch_stride_a=16 * d["lda"], batch_stride_b=0, batch_stride_d=16 * d["ldd"], M=16)
    elif k == 5:
        d.update(ksegs=4, A_x1=d["A"], B_x1=d["B"], A_x2=d["A"], B_x2=d["B"])
    elif k == 6:
        d.update(batch=2, residual=None, D_x1=out_buf())
    elif k == 7:
        d.update(ksegs=3, A_x1=d["A"], B_x1=d["B"])
    elif k == 8:
        d["A"] = d["A"][4:]
    elif k == 9:
        d.update(batch=2, residual=None, A_x1=d["A"], B_x1=d["B"])
    elif k == 10:
        d.update(rowscale=d["bias"], rs_div=0, rs_mod=5)
    elif k == 11:
        d["dropout_p"] = 0.1
    elif k == 12:
        d["d_p16"] = 1                      # ldd = N + 8 is no multiple of 16
    elif k == 13:
        d.update(frame_stats=out_buf(), frame_rows=32, M=128)
    elif k == 14:
        d.update(act_grad_src=d["residual"], residual=None, act=GELU)        # bias is still there
    elif k == 15:
        d["batch_accum"] = 1
    got = gemm_p16_class(fields_of(d), be.cus)
    assert got == ("refuse", k), (k, got)
    rc = be.gemm(d)
    be.sync()
    assert rc < 0, (k, rc)
    assert len(be.last_error()) > 0, k
    for out in outs:
        assert out["D"].unchanged(), "check %d: D was written" % k
    for b in extra_out + c["inputs"]:
        assert b.unchanged(), "check %d: a buffer changed" % k
