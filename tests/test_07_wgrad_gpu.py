"""Every launch geometry of the grouped weight-gradient GEMM (vptr_gemm_grouped with token-major P16 operands, gemm_p16.hip).  The
launcher picks one of five kernels, named here by the codes of vptr_wgrad_kernel_counts:

    A  plain, 128 x 176 tiles, atomic adds                     D  plain, 256 x 176 tiles
    B  plain, 128-row tiles, plain stores (token ranges)       E  persistent panel-synchronous, 256-row tiles
    C  persistent panel-synchronous, 128-row tiles

They are driven by hand-built descriptor tables, through the planner (defer_wgrad / flush_wgrads, chunked flushes) and through
ops.convt_weight_grads.  The reference is fp64 on the GPU applied to the P16-DECODED operands, so the only error left is the kernel's own:
rel-L2 < 3e-5 per destination, and |D - ref| <= 1e-4 (|A|^T |B|) per element -- a dropped or doubled tile, row or token shows there even
where a norm would dilute it.  Every test reads the launch counters and asserts that the kernels it is about actually ran: the persistent
kernels fall back to the plain ones without a message (thresholds, occupancy, CU count)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import margin, rel

pytestmark = pytest.mark.gpu
TOL3 = 3e-5
ELEM = 1e-4
SENTINEL = 0x7FA5A5A5      # a NaN bit pattern no kernel writes: padding and gaps between destinations must keep it bit for bit
CODES = "ABCDE"
WIDE = 2368                # token-major operand tensors: problems read column slices of them (lda, ldb > the problem's width)
MIXED_T = (1, 31, 100, 545, 1000, 2081)   # plain launches mix token counts; 545 / 1000 / 2081: arrival only / one wait / three waits


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


@pytest.fixture(autouse=True)
def _restore(ops, monkeypatch):
    """every test leaves ops.config, the tuner table and the record queues as it found them"""
    monkeypatch.setattr(ops.wgrad, "_wgrad_tune", {})
    monkeypatch.setattr(ops.config, "wgrad_rows", ops.config.wgrad_rows)
    try:
        yield
    finally:
        ops.discard_wgrads()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def launch_counts(ops):
    out = (ctypes.c_int * 5)()
    ops.wgrad.check(ops.lib.vptr_wgrad_kernel_counts(out, 5), "vptr_wgrad_kernel_counts")
    return dict(zip(CODES, out))


def sync_timeouts(ops):
    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    ops.wgrad.check(ops.lib.vptr_wgrad_sync_stats(ops.wgrad.ptr(buf), ops.wgrad.stream()), "vptr_wgrad_sync_stats")
    return int(buf.sum())


class Launches:
    """launch-counter deltas of the five kernels across a block (`ran`); the bounded-wait time-outs of the persistent kernels are logged
    (helpers.margin), not asserted: a displaced workgroup costs time, not correctness"""

    def __init__(self, ops, name):
        self.ops, self.name = ops, name

    def __enter__(self):
        self.c0, self.t0 = launch_counts(self.ops), sync_timeouts(self.ops)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        c1 = launch_counts(self.ops)
        self.ran = {k: c1[k] - self.c0[k] for k in CODES if c1[k] != self.c0[k]}
        margin(self.name + ":sync_timeouts", sync_timeouts(self.ops) - self.t0, 0)
        return False


def assert_ran(L, want):
    assert L.ran == want, "asked for kernel(s) %s, the launcher ran %s (a persistent kernel that fell back to a plain one?)" % (want, L.ran)


def check_close(name, got, d0, alpha, prod, absprod):
    """got - d0 (the destination's change) against alpha * prod (fp64): rel-L2 and the element-wise bound.  The 2^-22 |got| term is the
    rounding of the fp32 destination itself (D0 + v).  A destination whose exact value cancels (||ref|| < 1e-3 || |A|^T|B| ||: the
    k-projection biases of the model, zero in exact arithmetic) is held to the element-wise bound only -- a relative error between two
    round-offs means nothing; random operands sit at 1.2 / sqrt(T) and above."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), "%s: non-finite values (an element no tile wrote?)" % name
    inc = got - (d0.double() if d0 is not None else 0.0)
    ref = alpha * prod
    r = rel(inc, ref)
    if float(ref.norm()) >= 1e-3 * abs(alpha) * float(absprod.norm()):
        assert r < TOL3, (name, r)
    err = (inc - ref).abs()
    ratio = err / (ELEM * abs(alpha) * absprod + 2.0 ** -22 * got.abs() + 1e-300)
    worst = float(ratio.max())
    if worst > 1.0:
        idx = [int(i) for i in torch.nonzero(ratio > 1.0)[:8].flatten()] if ratio.dim() == 1 else \
            [tuple(int(v) for v in i) for i in torch.nonzero(ratio > 1.0)[:8]]
        raise AssertionError("%s: %d elements beyond 1e-4 |A|^T|B| (worst ratio %.3g), first at %s" % (name, int((ratio > 1.0).sum()), worst, idx))
    margin(name + ":elem", worst, 1.0)


# ---- hand-built descriptor tables ---------------------------------------------------------------------------------------------------
class Operands:
    """per token count: A and B operands [T, WIDE] as P16 tensors, and their decoded fp64 values (what the kernel is given)"""

    def __init__(self, ops, dev):
        self.ops, self.dev, self.cache = ops, dev, {}

    def get(self, T):
        if T not in self.cache:
            gen = torch.Generator(device=self.dev).manual_seed(1000 + T)
            a = self.ops.to_p16(torch.randn((T, WIDE), device=self.dev, generator=gen))
            b = self.ops.to_p16(torch.randn((T, WIDE), device=self.dev, generator=gen))
            self.cache[T] = (a, b, self.ops.p16_decode(a).double(), self.ops.p16_decode(b).double())
        return self.cache[T]


@pytest.fixture(scope="module")
def opnds(ops):
    o = Operands(ops, torch.device("cuda:0"))
    yield o
    o.cache.clear()
    torch.cuda.empty_cache()


class Prob:
    """D[M, N] (+)= alpha * A[T, M]^T . B[T, N]; flip: stored transposed (D[n * ldd + m]) and the bias vector gets the column sums of B"""

    def __init__(self, i, M, N, T, flip, bias, alpha):
        assert M % 16 == 0 and N % 16 == 0, "P16 problems are whole 16-channel granules"
        self.M, self.N, self.T, self.flip, self.bias, self.alpha = M, N, T, flip, bias, alpha
        self.oa, self.ob = 16 * (i % 5), 16 * ((i + 2) % 5)      # column offsets into the wide operands (whole granules)
        assert self.oa + M <= WIDE and self.ob + N <= WIDE

    def tiles(self, tr):
        return -(-self.M // tr) * -(-self.N // 176)

    def ref(self, opnds):
        _, _, a64, b64 = opnds.get(self.T)
        A, B = a64[:, self.oa:self.oa + self.M], b64[:, self.ob:self.ob + self.N]
        prod, absprod = A.t() @ B, A.abs().t() @ B.abs()
        if self.flip:
            prod, absprod = prod.t(), absprod.t()
        S = B if self.flip else A
        return prod, absprod, S.sum(0), S.abs().sum(0)


# (M, N, flipped, bias, alpha).  P16 problems have M, N % 16 == 0, so the row remainders are multiples of 16.
# 128-row tiles: M % 128 in {0, 16, 32, 64, 80, 112}, N % 176 in {0, 16, 64, 160}; flipped problems with a bias have a free 16-row
# fragment in their last row tile (f0 = ceil((M % 128) / 16) < 8), at ones-fragment index cmi = f0 % 2 in {0, 1}; 1136 leaves exactly 16.
# 1029 tiles: above the persistent threshold (1024), not a multiple of 8.
P128 = [(2048, 2112, False, True, 1.0), (1040, 1600, False, True, 0.5), (2080, 528, True, True, 2.0), (1136, 1920, True, True, 1.0),
        (1104, 1472, True, True, 0.5), (656, 336, True, True, 2.0), (2112, 2112, False, True, 1.0), (2048, 2112, True, False, 1.0),
        (1152, 2112, False, False, 2.0)]
# 256-row tiles: M % 256 in {0, 16, 64, 96, 208, 240}; the flipped problems with a bias put the ones-fragment at cmi = 1, 0, 2, 1, 3
# (1264 leaves exactly 16 free rows).  517 tiles: above the persistent threshold (512), not a multiple of 8.
P256 = [(2048, 2112, False, True, 1.0), (2064, 1600, True, True, 0.5), (1856, 1472, True, True, 2.0), (1120, 2096, True, True, 1.0),
        (2000, 528, True, True, 1.0), (1264, 2112, True, True, 0.5), (2288, 1936, False, True, 2.0), (528, 336, False, False, 1.0),
        (352, 880, False, True, 0.5)]
# code -> (split_k of the prototype, atomic, problem list, tile rows, tile threshold of the persistent kernel)
KERNELS = {"A": (1, 1, P128, 128), "B": (1, 0, P128, 128), "C": (-1, 1, P128, 128), "D": (-3, 1, P256, 256), "E": (-2, 1, P256, 256)}


def layout(probs):
    """one slab for all destinations: problem i's D is [h, ldd] with h x w used (ldd padded), then a gap, then its bias vector, a gap"""
    off, lay = 0, []
    for i, p in enumerate(probs):
        h, w = (p.N, p.M) if p.flip else (p.M, p.N)
        ldd = w + 3 + 16 * (i % 3)
        d_off = off
        off += h * ldd + 37 + i
        r_off = None
        if p.bias:
            r_off = off
            off += (p.N if p.flip else p.M) + 19
        lay.append((d_off, h, w, ldd, r_off))
    return lay, off


def dest(slab, lay_i):
    d_off, h, w, ldd, _ = lay_i
    return slab[d_off:d_off + h * ldd].view(h, ldd)[:, :w]


def bias_of(slab, lay_i, p):
    r_off = lay_i[4]
    return slab[r_off:r_off + (p.N if p.flip else p.M)]


def launch_direct(ops, probs, opnds, slab, lay, split_k, atomic, tr):
    """one vptr_gemm_grouped launch built the way ops._launch_wgrad_group builds it; returns what must outlive the launch"""
    GemmDesc = ops.wgrad.GemmDesc
    n = len(probs)
    descs = (GemmDesc * n)()
    starts, total = [], 0
    base = slab.data_ptr()
    for i, (p, (d_off, h, w, ldd, r_off)) in enumerate(zip(probs, lay)):
        a, b, _, _ = opnds.get(p.T)
        d = descs[i]
        d.precision, d.split_k, d.atomic, d.alpha = 3, 1, atomic, p.alpha
        d.A, d.B, d.D = a.data_ptr() + 4 * p.oa, b.data_ptr() + 4 * p.ob, base + 4 * d_off
        d.a_rowsum = (base + 4 * r_off) if r_off is not None else None
        d.lda, d.ldb, d.ldd = WIDE, WIDE, ldd
        d.M, d.N, d.K = p.M, p.N, p.T
        d.d_transposed = int(p.flip)
        d.a_mode, d.b_mode = ops.A_P16T, ops.B_P16T
        starts.append(total)
        total += p.tiles(tr)
    descs[0].split_k = split_k
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(slab.device)
    st = torch.tensor(starts, dtype=torch.int32, device=slab.device)
    ops.wgrad.check(ops.lib.vptr_gemm_grouped(ctypes.byref(descs[0]), ops.wgrad.ptr(raw), ops.wgrad.ptr(st), n, total, ops.wgrad.stream()),
                    "vptr_gemm_grouped")
    return total, (raw, st)


def check_direct(tag, probs, lay, slab, d0s, r0s, opnds):
    for i, p in enumerate(probs):
        prod, absprod, s, abss = p.ref(opnds)
        name = "%s:p%d(M=%d,N=%d,T=%d,flip=%d,alpha=%g)" % (tag, i, p.M, p.N, p.T, p.flip, p.alpha)
        check_close(name, dest(slab, lay[i]), d0s[i], p.alpha, prod, absprod)
        if p.bias:
            check_close(name + ":bias", bias_of(slab, lay[i], p), r0s[i], p.alpha, s, abss)


@pytest.mark.parametrize("code,T", [("A", None), ("B", None), ("C", 545), ("C", 2081), ("D", None), ("E", 1000), ("E", 2081)])
def test_direct_descriptor_matrix(ops, dev, opnds, code, T):
    """one launch per kernel of mixed shapes (binary search over tile_start), row remainders that leave every ones-fragment position,
    column remainders, operand slices of wider tensors, alpha 0.5 / 1 / 2, problems with and without a bias.  Destinations are views of
    one sentinel-filled slab with padded rows and gaps: atomic launches accumulate into random values, the store launch (B) overwrites
    NaN.  The persistent launches walk one token count (their contract) over a tile count that leaves some XCD a partial last round."""
    split_k, atomic, spec, tr = KERNELS[code]
    probs = [Prob(i, M, N, T or MIXED_T[i % len(MIXED_T)], fl, bi, al) for i, (M, N, fl, bi, al) in enumerate(spec)]
    if code in "CE":
        total = sum(p.tiles(tr) for p in probs)
        assert total >= (1024 if code == "C" else 512) and total % 8 != 0
    lay, n = layout(probs)
    slab = torch.empty(n, device=dev)
    slab.view(torch.int32).fill_(SENTINEL)
    gen = torch.Generator(device=dev).manual_seed(7)
    d0s, r0s = [], []
    for i, p in enumerate(probs):
        D = dest(slab, lay[i])
        if atomic:
            D.copy_(torch.randn(D.shape, device=dev, generator=gen))
            d0s.append(D.clone())
        else:
            D.fill_(float("nan"))
            d0s.append(None)
        if p.bias:
            b = bias_of(slab, lay[i], p)
            b.copy_(torch.randn(b.shape, device=dev, generator=gen))
            r0s.append(b.clone())
        else:
            r0s.append(None)
    with Launches(ops, "direct_%s_T%s" % (code, T)) as L:
        keep = launch_direct(ops, probs, opnds, slab, lay, split_k, atomic, tr)
    assert_ran(L, {code: 1})
    check_direct(code, probs, lay, slab, d0s, r0s, opnds)
    used = torch.zeros(n, dtype=torch.bool, device=dev)
    for i, p in enumerate(probs):
        dest(used, lay[i]).fill_(True)
        if p.bias:
            bias_of(used, lay[i], p).fill_(True)
    bits = slab.view(torch.int32)[~used]
    assert bool((bits == SENTINEL).all()), "%d padding / gap elements were written" % int((bits != SENTINEL).sum())
    del keep, slab, used


def test_geometries_agree_bit_for_bit(ops, dev, opnds):
    """one problem set, zeroed destinations, no token split, through A, C, D, E and B: every output element comes from exactly one tile,
    which runs the same K loop and the same three MFMAs per K-step in every geometry, and lands once -- the results are identical"""
    T = 1000
    spec = P256 + [(1024, 528, False, False, 1.0), (512, 880, False, True, 2.0)]   # valid in both geometries, >= 1024 / 512 tiles
    probs = [Prob(i, M, N, T, fl, bi, al) for i, (M, N, fl, bi, al) in enumerate(spec)]
    lay, n = layout(probs)
    outs = {}
    for code in "ACDEB":
        split_k, atomic, _, tr = KERNELS[code]
        slab = torch.zeros(n, device=dev)
        with Launches(ops, "agree_" + code) as L:
            keep = launch_direct(ops, probs, opnds, slab, lay, split_k, atomic, tr)
        assert_ran(L, {code: 1})
        outs[code] = slab
        del keep
    check_direct("agree_A", probs, lay, outs["A"], [None] * len(probs), [None] * len(probs), opnds)
    for code in "CDEB":
        if torch.equal(outs[code], outs["A"]):
            continue
        diff = []
        for i, p in enumerate(probs):
            nd = int((dest(outs[code], lay[i]) != dest(outs["A"], lay[i])).sum())
            nb = int((bias_of(outs[code], lay[i], p) != bias_of(outs["A"], lay[i], p)).sum()) if p.bias else 0
            if nd or nb:
                diff.append((i, p.M, p.N, p.flip, nd, nb))
        raise AssertionError("kernel %s differs from A: (problem, M, N, flip, differing D elements, differing bias elements) %s" % (code, diff))


# ---- through the planner ------------------------------------------------------------------------------------------------------------
C_, F_ = 528, 2112


class Layers:
    """weight gradients of K64-like transformer layers in a FlatAdamW-style slab (every weight followed by its bias): packed in_proj
    [1584, 528] deferred as three row slices, out_proj [528, 528], fc1 [2112, 528], fc2 [528, 2112] (flipped by the planner).  Operand
    tensors are shared between the layers of one token count.  classes: [(tokens, layers)]."""

    SHAPES = (("in_proj", 3 * C_, C_), ("out_proj", C_, C_), ("fc1", F_, C_), ("fc2", C_, F_))

    def __init__(self, ops, dev, classes, seed=0):
        self.ops, self.dev = ops, dev
        self.tok, self.refs = {}, {}
        self.params = []                  # (tokens, name, weight offset, bias offset, alpha)
        off = 0
        for ci, (T, nl) in enumerate(classes):
            if T not in self.tok:
                gen = torch.Generator(device=dev).manual_seed(500 + T + seed)
                t = {}
                for nm, c in (("x528", C_), ("x2112", F_), ("g528", C_), ("g2112", F_), ("g1584", 3 * C_)):
                    p = ops.to_p16(torch.randn((T, c), device=dev, generator=gen))
                    t[nm] = (p, ops.p16_decode(p).double())
                self.tok[T] = t
            for li in range(nl):
                alpha = (1.0, 0.5, 2.0)[(li + ci) % 3]
                for name, N, K in self.SHAPES:
                    self.params.append((T, name, off, off + N * K, alpha))
                    off += N * K + N
        self.n = off
        self.slab = torch.empty(off, device=dev)
        self.slab.copy_(torch.randn(off, device=dev, generator=torch.Generator(device=dev).manual_seed(900 + seed)))
        self.slab0 = self.slab.clone()

    def views(self, name, w_off, b_off):
        N, K = {n: (a, b) for n, a, b in self.SHAPES}[name]
        return self.slab[w_off:w_off + N * K].view(N, K), self.slab[b_off:b_off + N]

    def records(self):
        """(g, x, dW, db, N, K, tokens, alpha) in the order the model's backward pass would record them"""
        out = []
        for (T, name, w_off, b_off, alpha) in self.params:
            t = self.tok[T]
            W, b = self.views(name, w_off, b_off)
            if name == "in_proj":
                for k in range(3):
                    out.append((t["g1584"][0][:, k * C_:(k + 1) * C_], t["x528"][0], W[k * C_:(k + 1) * C_], b[k * C_:(k + 1) * C_], C_, C_, T, alpha))
            else:
                g, x = {"out_proj": ("g528", "x528"), "fc1": ("g2112", "x528"), "fc2": ("g528", "x2112")}[name]
                out.append((t[g][0], t[x][0], W, b, W.shape[0], W.shape[1], T, alpha))
        return out

    def defer(self):
        for (g, x, dW, db, N, K, T, alpha) in self.records():
            self.ops.defer_wgrad(g, x, dW, N, K, T, db=db, alpha=alpha, p16=True)

    def ref(self, T, name):
        key = (T, name)
        if key not in self.refs:
            t = self.tok[T]
            g, x = {"in_proj": ("g1584", "x528"), "out_proj": ("g528", "x528"), "fc1": ("g2112", "x528"), "fc2": ("g528", "x2112")}[name]
            G, X = t[g][1], t[x][1]
            self.refs[key] = (G.t() @ X, G.abs().t() @ X.abs(), G.sum(0), G.abs().sum(0))
        return self.refs[key]

    def check(self, tag, slab=None):
        slab = self.slab if slab is None else slab
        for i, (T, name, w_off, b_off, alpha) in enumerate(self.params):
            N, K = {n: (a, b) for n, a, b in self.SHAPES}[name]
            prod, absprod, s, abss = self.ref(T, name)
            nm = "%s:%d:%s(T=%d)" % (tag, i, name, T)
            check_close(nm, slab[w_off:w_off + N * K].view(N, K), self.slab0[w_off:w_off + N * K].view(N, K), alpha, prod, absprod)
            check_close(nm + ":bias", slab[b_off:b_off + N], self.slab0[b_off:b_off + N], alpha, s, abss)

    def reset(self):
        self.slab.copy_(self.slab0)

    def free(self):
        self.tok.clear()
        self.refs.clear()
        del self.slab, self.slab0


@pytest.mark.parametrize("rows,want", [(128, {"C": 1}), (256, {"E": 1, "A": 1})])
def test_planner_k64_layers(ops, dev, monkeypatch, rows, want):
    """eleven K64-like layers at one token count through defer_wgrad / flush_wgrads: 1782 tiles of 128 rows (one persistent launch), or
    528 tiles of 256 rows (persistent) + 726 tiles of the 128-row remainders and small problems (plain: below the threshold)"""
    monkeypatch.setattr(ops.config, "wgrad_rows", rows)
    L = Layers(ops, dev, [(1000, 11)])
    L.defer()
    with Launches(ops, "planner_k64_%d" % rows) as n:
        ops.flush_wgrads()
    assert_ran(n, want)
    L.check("planner_k64_%d" % rows)
    L.free()


@pytest.mark.parametrize("rows,want", [(128, {"C": 2, "A": 1}), (256, {"D": 3, "A": 1})])
def test_planner_two_token_classes(ops, dev, monkeypatch, rows, want):
    """two token classes as in KTH128 (encoder / decoder layers) of >= 1024 tiles each get a persistent launch each; a third, small class
    goes to one plain launch.  With 256-row tiles every token count's tall part gets a 256-row launch of its own (all three below the
    512-tile threshold: plain), and the 128-row remainders of all classes (each < 1024 tiles) share one plain launch."""
    monkeypatch.setattr(ops.config, "wgrad_rows", rows)
    L = Layers(ops, dev, [(1000, 7), (545, 7), (100, 1)])
    L.defer()
    with Launches(ops, "planner_classes_%d" % rows) as n:
        ops.flush_wgrads()
    assert_ran(n, want)
    L.check("planner_classes_%d" % rows)
    L.free()


@pytest.mark.parametrize("rows", [128, 256])
def test_planner_small_group_token_ranges(ops, dev, monkeypatch, rows):
    """a group of <= 3 problems is cut into token ranges (the last one shorter, with a token tail) that accumulate into the same
    destinations: one plain 128-row launch whatever the tile-row setting"""
    monkeypatch.setattr(ops.config, "wgrad_rows", rows)
    L = Layers(ops, dev, [(5000, 1)])
    recs = [r for r in L.records() if r[4] != C_ or r[5] != C_]        # fc1 and fc2: two problems
    for (g, x, dW, db, N, K, T, alpha) in recs:
        ops.defer_wgrad(g, x, dW, N, K, T, db=db, alpha=alpha, p16=True)
    with Launches(ops, "planner_small_%d" % rows) as n:
        ops.flush_wgrads()
    assert_ran(n, {"A": 1})
    for i, (T, name, w_off, b_off, alpha) in enumerate(L.params):
        if name in ("fc1", "fc2"):
            N, K = {nm: (a, b) for nm, a, b in L.SHAPES}[name]
            prod, absprod, s, abss = L.ref(T, name)
            check_close("small:" + name, L.slab[w_off:w_off + N * K].view(N, K), L.slab0[w_off:w_off + N * K].view(N, K), alpha, prod, absprod)
            check_close("small:" + name + ":bias", L.slab[b_off:b_off + N], L.slab0[b_off:b_off + N], alpha, s, abss)
    L.free()


def test_planner_auto_mode_samples_both_geometries(ops, dev, monkeypatch):
    """VPTR_WGRAD_ROWS=auto: 2 * _TUNE_SAMPLES + 2 flushes of one problem set (each booked: synchronize after every flush) time both tile-row
    settings, every flush matches fp64, all flushes are bit-identical (one adder per element in every geometry), and the choice settles"""
    monkeypatch.setattr(ops.config, "wgrad_rows", "auto")
    L = Layers(ops, dev, [(1000, 11)])
    results = []
    with Launches(ops, "planner_auto") as n:
        for _ in range(2 * ops.wgrad._TUNE_SAMPLES + 2):
            L.slab.zero_()
            L.defer()
            ops.flush_wgrads()
            torch.cuda.synchronize()
            results.append(L.slab.clone())
    tune = list(ops.wgrad._wgrad_tune.values())
    assert len(tune) == 1
    tune = tune[0]
    assert len(tune["samples"][128]) >= 1 and len(tune["samples"][256]) >= 1, tune["samples"]
    assert "C" in n.ran and "E" in n.ran, n.ran
    ops.wgrad_tune_settle()
    assert tune["choice"] in (128, 256)
    L.slab0.zero_()
    for k, r in enumerate(results):
        L.check("auto:%d" % k, r)
        assert torch.equal(r, results[0]), "flush %d differs from flush 0" % k
    del results
    L.free()


@pytest.mark.parametrize("rows", [128, 256])
def test_chunked_flush_contract(ops, dev, monkeypatch, rows):
    """flush_wgrads(chunks=4, on_chunk=cb): when cb(p) runs, everything in the slab below p is final (the data-parallel trainer starts
    all-reduces on it).  A clone taken at that point on the current stream equals the final slab; the pointers increase and end with None;
    chunks use plain launches only (they run beside the all-reduce kernels)"""
    monkeypatch.setattr(ops.config, "wgrad_rows", rows)
    L = Layers(ops, dev, [(1000, 3)])
    L.defer()
    seen = []

    def cb(p):
        off = L.n if p is None else (p - L.slab.data_ptr()) // 4
        seen.append((p, L.slab[:off].clone()))
    with Launches(ops, "chunks_%d" % rows) as n:
        ops.flush_wgrads(chunks=4, on_chunk=cb)
    assert n.ran and set(n.ran) <= {"A", "D"}, n.ran
    ps = [p for p, _ in seen]
    assert 2 <= len(ps) <= 4 and ps[-1] is None, ps
    offs = [(p - L.slab.data_ptr()) // 4 for p in ps[:-1]]
    assert offs[0] > 0 and all(a < b for a, b in zip(offs, offs[1:] + [L.n])), offs
    for k, (p, c) in enumerate(seen):
        assert torch.equal(c, L.slab[:c.numel()]), "chunk %d: the range below its pointer changed after on_chunk" % k
    L.check("chunks_%d" % rows)
    del seen
    L.free()


# ---- the real problem set at bench size ----------------------------------------------------------------------------------------------
def test_k64_bench_size_problem_set(ops, dev, monkeypatch):
    """the launch the timed step makes: the K64 NAR transformer at batch 16 (10 240 tokens), one forward + backward with the weight
    gradients held, then the recorded problems flushed from the same gradient slab with 128- and with 256-row tiles.  Each destination's
    change is compared with the fp64 sum of the records that target it (the NCE projector receives two)."""
    import vptr_amd.model as pkg
    from helpers import build_transformer, jload, load
    from oracle import fill
    from vptr_amd.train import NARTrainer
    ops.unregister_flat_slabs()
    z = load("step_k64_n16_digest")
    cfg, meta = jload(z, "cfg"), jload(z, "meta")
    enc = pkg.VPTREnc(1, meta["feat"], 3, "reflect")
    dec = pkg.VPTRDec(1, meta["feat"], 3, "Tanh", "reflect")
    T = build_transformer(pkg, cfg, False)
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 10)
    fill.apply_fill(T, meta["seed"] + 20)
    tr = NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=meta["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1)
    past = ((fill.rand_input((meta["N"], cfg["Tp"], 1, meta["HW"], meta["HW"]), meta["seed"] + 100) - 0.6013795) / 2.7570653).to(dev)
    fut = ((fill.rand_input((meta["N"], cfg["Tf"], 1, meta["HW"], meta["HW"]), meta["seed"] + 200) - 0.6013795) / 2.7570653).to(dev)
    try:
        tr._front_impl(past, fut)           # forward + backward: weight gradients recorded (ops.hold_wgrads), not launched
        recs = ops.take_wgrads()
        torch.cuda.synchronize()
        grad = tr.opt.grad
        g0, g1 = grad.data_ptr(), grad.data_ptr() + 4 * grad.numel()
        assert len(recs) > 100 and all(r[9] for r in recs), "expected the P16 records of the K64 step"
        refs = {}                           # (data_ptr, shape, stride) -> [sum of alpha * product, sum of |alpha| * |product|] in fp64
        for (g, x, dW, N, K, M, _, db, alpha, _p) in recs:
            G, X = ops.p16_decode(g).double(), ops.p16_decode(x).double()
            for dst, v, a in ((dW, G.t() @ X, G.abs().t() @ X.abs()), (db, G.sum(0), G.abs().sum(0))):
                if dst is None:
                    continue
                assert g0 <= dst.data_ptr() < g1, "a destination outside the gradient slab"
                acc = refs.setdefault((dst.data_ptr(), tuple(dst.shape), tuple(dst.stride())), [torch.zeros_like(v), torch.zeros_like(a)])
                acc[0] += alpha * v
                acc[1] += abs(alpha) * a
            del G, X
        snap = grad.clone()
        for rows, code in ((128, "C"), (256, "E")):
            monkeypatch.setattr(ops.config, "wgrad_rows", rows)
            grad.copy_(snap)
            ops.requeue_wgrads(recs)
            with Launches(ops, "k64_bench_%d" % rows) as n:
                ops.flush_wgrads()
            assert code in n.ran and set(n.ran) <= {"A", "C", code}, n.ran   # (256: the 128-row remainders are a launch of their own)
            for (p, shape, stride), (prod, absprod) in refs.items():
                off = (p - g0) // 4
                got, before = grad.as_strided(shape, stride, off), snap.as_strided(shape, stride, off)
                check_close("k64_bench_%d:%d:%s" % (rows, off, shape), got, before, 1.0, prod, absprod)
    finally:
        ops.discard_wgrads()
        del tr, enc, dec, T
        ops.unregister_flat_slabs()
        torch.cuda.empty_cache()


# ---- ConvTranspose2d weight gradients (launch B + vptr_partial_reduce) ---------------------------------------------------------------
@pytest.mark.parametrize("geoms,tps", [([(4, 16, 16, 528, 128), (4, 32, 32, 128, 64)], 300), ([(3, 5, 7, 48, 32)], 40)],
                         ids=["k64_decoder", "short_last_range"])
def test_convt_weight_grads(ops, dev, geoms, tps):
    """ops.convt_weight_grads vs torch.autograd.grad of conv_transpose2d(3x3, s2, p1, op1) in fp64 on the P16-decoded operands, reshaped as
    the decoder does; the K64 decoder's two layers in one call, and a pixel count that is no multiple of 32 with a short last range"""
    layers, refs = [], []
    for li, (B, ih, iw, ci, co) in enumerate(geoms):
        oh, ow = 2 * ih, 2 * iw
        gen = torch.Generator(device=dev).manual_seed(40 + li)
        x = torch.randn((B * ih * iw, ci), device=dev, generator=gen)
        g = torch.randn((B * oh * ow, co), device=dev, generator=gen)
        layers.append((x, g, B, ih, iw, ci, oh, ow, co))
        x64 = ops.p16_decode(ops.to_p16(x)).double().view(B, ih, iw, ci).permute(0, 3, 1, 2)
        g64 = ops.p16_decode(ops.to_p16(g)).double().view(B, oh, ow, co).permute(0, 3, 1, 2)
        rr = []
        for xs, gs in ((x64, g64), (x64.abs(), g64.abs())):
            w = torch.zeros((ci, co, 3, 3), device=dev, dtype=torch.float64, requires_grad=True)
            y = F.conv_transpose2d(xs, w, stride=2, padding=1, output_padding=1)
            rr.append(torch.autograd.grad((y * gs).sum(), w)[0])
        refs.append(rr)
    with Launches(ops, "convt") as n:
        outs = ops.convt_weight_grads(layers, tokens_per_split=tps)
    assert_ran(n, {"B": 1})
    for (B, ih, iw, ci, co), D, (ref, absref) in zip(geoms, outs, refs):
        got = D.view(ci, 3, 3, co).permute(0, 3, 1, 2)
        check_close("convt(%d,%d,%d,%d,%d)" % (B, ih, iw, ci, co), got, None, 1.0, ref, absref)
