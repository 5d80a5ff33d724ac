"""Cases, fp64 references, bars and a CPU emulation of vptr_tensor_stats (include/vptr_hip_diag.h, csrc/tensor_stats.hip), shared by
tests/test_09l_tensor_stats_gpu.py (the library through the C ABI) and tests/test_tensor_stats_cpu.py (the emulation and its mutations).

A backend offers `dev` (where the tensors live), `call(p, g, m, v, seg_off, item_first, S, scale, state, ctl, table, ws, ws_bytes,
grid_cap) -> rc` on tensors of that device (None = NULL) and `sync()`.

The bars.
  * Norms (GRAD_NORM, WEIGHT_NORM): 2^-23 relative.  (double)x * x is exact (48 significant bits); an fp64 sum of at most 2^27
    non-negative terms is off by at most 2^27 * 2^-53 = 2^-26 relative in any order, the square root halves that, the product with the
    scale and the fp64 square root add 2^-52 each, and the one rounding to fp32 adds 2^-24: below 2^-23.
  * Maxima, counts, NUMEL: equal to the reference's fp32, bit for bit (a maximum is one of the inputs, times a scale in fp64 where the
    product of two fp32 values is exact; counts are whole numbers).
  * DIR_RMS: d = m / fmaf(sqrtf(v), isb, eps) in fp32 against the same expression in fp64 on the same fp32 inputs.  The library is built
    without fast-math, so sqrtf, the fma and the division each round correctly: relative error at most u = 2^-24 each.  To first order
    the denominator is off by at most 2u (the error of sqrtf enters through a non-negative term of a non-negative sum, so it is at most
    u of the whole; the fma rounds once), d by 3u, d^2 by 6u, a sum of non-negative d^2 by 6u + 2^-26, its square root by 3u + 2^-27,
    and the rounding of the result to fp32 adds u: 4u + 2^-27 < DIR_RTOL = 2^-22 + 2^-26.  A denormal d carries an absolute error of
    half the smallest denormal instead, which the rms cannot amplify: DIR_ATOL = 2^-149.
"""
import numpy as np
import torch

from vptr_amd import diagnostics as D

NORM_RTOL = 2.0 ** -23
DIR_RTOL = 2.0 ** -22 + 2.0 ** -26
DIR_ATOL = 2.0 ** -149
S_SKIP_NOW, S_INV_SQRT_BC2, S_EPS = 2, 7, 13          # include/vptr_hip_optim.h
ISB = float(np.float32(1.0 / np.sqrt(1.0 - 0.999 ** 3)))   # the bias correction of the third step: far from 1
EPS = float(np.float32(1e-8))
SCALE = 0.25
SENTINEL = -3.0                                       # the words of ctl neither side owns
TABLE_GUARD, WS_GUARD = 64, 20                        # fp32 words (256 bytes: keeps the table on the 64-byte grid) / doubles

MIXED = [1, 4097, 5, 4, 3, 4095, 4096, 8195]
GEOS = {
    # name: (sizes, leading floats of (p, g, m, v) in front of the slab, pad elements behind seg_off[S], grid_cap)
    "one": ([1], (4, 4, 4, 4), 0, 0),
    "mixed": (MIXED, (4, 4, 4, 4), 0, 0),
    "offgrid": (MIXED, (1, 1, 1, 1), 0, 0),
    "skewed": ([5, 4097, 3], (4, 5, 6, 7), 0, 0),
    "many": ([(i * 7) % 9 + 1 for i in range(700)], (4, 4, 4, 4), 0, 3),
    "big": ([70001], (4, 4, 4, 4), 0, 0),
    "pad": ([5, 4096, 2], (4, 4, 4, 4), 3, 0),
}
assert {o % 4 for o in np.cumsum([0] + MIXED[:-1])} == {0, 1, 2, 3}
assert sorted(set(GEOS["many"][0])) == list(range(1, 10))


def bits(t):
    """the bit patterns as integers, always a copy (on the CPU `.cpu()` alone would alias the tensor)"""
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).clone()


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def rn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------
def ref_table(p, g, m, v, sizes, scale=1.0, isb=ISB, eps=EPS, moments=True):
    """the [S + 1, 8] table in fp64 from the slabs (1-D CPU tensors of any float dtype, read as fp64), plain torch, tensor by tensor"""
    off, rows = 0, []
    p, g = p.double(), g.double()
    if moments:
        d_all = m.double() / (v.double().sqrt() * float(isb) + float(eps))

    def row(a, b):
        gi, pi = g[a:b], p[a:b]

        def mx(x):
            x = x[~torch.isnan(x)]
            return float(x.abs().max()) if x.numel() else 0.0
        n = b - a
        return [float(gi.pow(2).sum().sqrt()) * scale, float(pi.pow(2).sum().sqrt()), mx(gi) * scale, mx(pi),
                float((d_all[a:b].pow(2).sum() / n).sqrt()) if moments else 0.0,
                float((~torch.isfinite(gi)).sum()), float((~torch.isfinite(pi)).sum()), float(n)]
    for n in sizes:
        rows.append(row(off, off + n))
        off += n
    rows.append(row(0, off))
    return torch.tensor(rows, dtype=torch.float64)


def check_table(got, ref, moments, what=""):
    """got: fp32 [S + 1, 8]; ref: fp64 [S + 1, 8].  Every word inside its bar; -> the worst distance of each kind (in units of its bar)"""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref.shape, (got.shape, ref.shape)
    worst = {"norm": 0.0, "dir": 0.0}
    for r in range(ref.shape[0]):
        for c in (D.GRAD_NORM, D.WEIGHT_NORM, D.DIR_RMS):
            x, y = float(got[r, c]), float(ref[r, c])
            where = "%s row %d %s: got %r, reference %r" % (what, r, D.COLUMNS[c], x, y)
            if c == D.DIR_RMS and not moments:
                assert same_bits(got[r, c], torch.zeros((), dtype=torch.float32)), where
            elif y != y:
                assert x != x, where
            elif y in (float("inf"), float("-inf")) or float(np.float32(y)) == float("inf"):
                assert x == float("inf"), where
            else:
                bar = NORM_RTOL * abs(y) if c != D.DIR_RMS else DIR_RTOL * abs(y) + DIR_ATOL
                assert abs(x - y) <= bar, where + " (%.3f of the bar)" % (abs(x - y) / bar if bar else float("inf"))
                if bar:
                    k = "dir" if c == D.DIR_RMS else "norm"
                    worst[k] = max(worst[k], abs(x - y) / bar)
        for c in (D.GRAD_MAXABS, D.WEIGHT_MAXABS, D.GRAD_NONFINITE, D.WEIGHT_NONFINITE, D.NUMEL):
            assert same_bits(got[r, c], ref[r, c].float()), "%s row %d %s: got %r, reference %r" % (what, r, D.COLUMNS[c], float(got[r, c]), float(ref[r, c]))
    return worst


# ---- a call's buffers ----------------------------------------------------------------------------------------------------------------
class World:
    """the slabs of a geometry inside NaN surroundings, the plan, and NaN-filled table and workspace inside NaN guards"""

    def __init__(self, be, geo, moments=True, scaled=False, seed=0, every=1, on_skip=0, skip_now=0.0, ws_items=None):
        self.be, self.geo, self.moments, self.scaled = be, geo, moments, scaled
        self.sizes, leads, pad, self.grid_cap = GEOS[geo]
        self.total = sum(self.sizes)
        self.S = len(self.sizes)
        self.seg_off_h, self.item_first_h = D.plan(self.sizes)
        self.items = int(self.item_first_h[-1])
        self.host = {"p": rn(self.total, 100 + seed), "g": rn(self.total, 200 + seed, 0.3), "m": rn(self.total, 300 + seed, 0.1),
                     "v": rn(self.total, 400 + seed, 0.1).pow(2) + 1e-6}
        self.leads, self.pad = dict(zip("pgmv", leads)), pad
        self.scale_h = SCALE if scaled else 1.0
        state = torch.zeros(16)
        state[S_SKIP_NOW], state[S_INV_SQRT_BC2], state[S_EPS] = skip_now, ISB, EPS
        ctl = torch.full((16,), SENTINEL)
        ctl[D.C_EVERY], ctl[D.C_ON_SKIP], ctl[D.C_PHASE], ctl[D.C_COMPUTED], ctl[D.C_AGE] = float(every), float(on_skip), 0.0, 0.0, 0.0
        dev = be.dev
        self.state, self.ctl = state.to(dev), ctl.to(dev)
        self.scale = torch.tensor([SCALE], dtype=torch.float32).to(dev) if scaled else None
        self.seg_off, self.item_first = self.seg_off_h.to(dev), self.item_first_h.to(dev)
        self.tbuf = torch.full((2 * TABLE_GUARD + (self.S + 1) * 8,), float("nan")).to(dev)
        self.table = self.tbuf[TABLE_GUARD:TABLE_GUARD + (self.S + 1) * 8]
        self.ws_items = self.items if ws_items is None else ws_items
        self.wbuf = torch.full((2 * WS_GUARD + self.ws_items * 5,), float("nan"), dtype=torch.float64).to(dev)
        self.ws = self.wbuf[WS_GUARD:WS_GUARD + self.ws_items * 5]
        self._tfill, self._wfill = bits(self.tbuf), bits(self.wbuf)
        self.upload()

    def upload(self):
        """(re)build the device slabs from `host`: NaN in front of the slab, behind it and in its pad"""
        self.bufs, self.slab = {}, {}
        for k in "pgmv":
            lead = self.leads[k]
            buf = torch.full((lead + self.total + self.pad + 5,), float("nan"))
            buf[lead:lead + self.total] = self.host[k]
            self.bufs[k] = buf.to(self.be.dev)
            self.slab[k] = self.bufs[k][lead:lead + self.total + self.pad]
        self._in = {k: bits(b) for k, b in self.bufs.items()}

    def call(self, grid_cap=None, ws_bytes=None):
        mom = self.moments
        rc = self.be.call(self.slab["p"], self.slab["g"], self.slab["m"] if mom else None, self.slab["v"] if mom else None, self.seg_off,
                          self.item_first, self.S, self.scale, self.state if mom else None, self.ctl, self.table, self.ws,
                          self.ws_items * D.PART_BYTES if ws_bytes is None else ws_bytes, self.grid_cap if grid_cap is None else grid_cap)
        self.be.sync()
        return rc

    def ref(self):
        return ref_table(self.host["p"], self.host["g"], self.host["m"], self.host["v"], self.sizes, self.scale_h, ISB, EPS, self.moments)

    def rows(self):
        return self.table.detach().cpu().view(self.S + 1, 8).clone()

    def ctl_words(self):
        c = self.ctl.detach().cpu()
        return float(c[D.C_PHASE]), float(c[D.C_COMPUTED]), float(c[D.C_AGE])

    def guards_intact(self):
        t, w = bits(self.tbuf), bits(self.wbuf)
        n, k = (self.S + 1) * 8, self.ws_items * 5
        ok = bool((t[:TABLE_GUARD] == self._tfill[:TABLE_GUARD]).all() and (t[TABLE_GUARD + n:] == self._tfill[TABLE_GUARD + n:]).all())
        ok = ok and bool((w[:WS_GUARD] == self._wfill[:WS_GUARD]).all() and (w[WS_GUARD + k:] == self._wfill[WS_GUARD + k:]).all())
        c = self.ctl.detach().cpu()
        own = [D.C_EVERY, D.C_ON_SKIP, D.C_PHASE, D.C_COMPUTED, D.C_AGE]
        ok = ok and all(float(c[i]) == SENTINEL for i in range(16) if i not in own)
        return ok and all(bool((bits(b) == self._in[k]).all()) for k, b in self.bufs.items())

    def untouched(self):
        """table and workspace hold what they were filled with"""
        return bool((bits(self.tbuf) == self._tfill).all() and (bits(self.wbuf) == self._wfill).all())

    def snapshot(self):
        return bits(self.tbuf).clone(), bits(self.wbuf).clone()

    def put_ctl(self, idx, value):
        self.ctl[idx:idx + 1].fill_(float(value))

    def put_state(self, idx, value):
        self.state[idx:idx + 1].fill_(float(value))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
GEO_CASES = [(geo, mom, sc) for geo in GEOS for mom in (1, 0) for sc in (0, 1)]


def run_geometry(be, geo, moments, scaled):
    w = World(be, geo, bool(moments), bool(scaled), seed=len(geo))
    assert w.call() == 0
    assert w.ctl_words() == (0.0, 1.0, 0.0)
    worst = check_table(w.rows(), w.ref(), w.moments, geo)
    assert w.guards_intact(), "%s: a guard, an input or a foreign word of ctl changed" % geo
    assert not bool(torch.isnan(w.ws).any()), "a partial record was left unwritten"
    return worst


BITEQ_CASES = ["mixed", "offgrid", "many", "big"]


def run_bit_equal(be, geo):
    """the same table, bit for bit, with 1, 3 and the default number of workgroups, and from a second call"""
    w = World(be, geo, True, True, seed=5)
    tabs = []
    for cap in (1, 3, 0, 0):
        w.table.fill_(float("nan"))
        w.ws.fill_(float("nan"))
        assert w.call(grid_cap=cap) == 0
        tabs.append((w.rows(), bits(w.ws).clone()))
    check_table(tabs[0][0], w.ref(), True, geo)
    for t, s in tabs[1:]:
        assert same_bits(t, tabs[0][0]) and bool((s == tabs[0][1]).all()), "%s: the table depends on the grid or the run" % geo
    assert w.guards_intact()


NONFINITE_CASES = ["nan", "+inf", "-inf"]


def run_nonfinite(be, kind):
    """a NaN / Inf in the LAST element of tensor i and the FIRST of tensor i + 2: tensor i + 1 between them stays finite"""
    val = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[kind]
    for geo, i in (("mixed", 0), ("mixed", 4), ("offgrid", 5), ("many", 350)):
        w = World(be, geo, True, True, seed=9)
        off = w.seg_off_h.tolist()
        w.host["g"][off[i + 1] - 1] = val
        w.host["g"][off[i + 2]] = val
        w.host["p"][off[i + 2]] = val
        w.upload()
        assert w.call() == 0
        rows, ref = w.rows(), w.ref()
        check_table(rows, ref, True, "%s %s" % (geo, kind))
        hit = {i, i + 2, w.S}
        for r in range(w.S + 1):
            bad = not bool(torch.isfinite(rows[r, D.GRAD_NORM])) or float(rows[r, D.GRAD_NONFINITE]) != 0.0
            assert bad == (r in hit), (geo, kind, r)
        assert [float(rows[r, D.GRAD_NONFINITE]) for r in (i, i + 1, i + 2, w.S)] == [1.0, 0.0, 1.0, 2.0]
        assert [float(rows[r, D.WEIGHT_NONFINITE]) for r in (i, i + 1, i + 2, w.S)] == [0.0, 0.0, 1.0, 1.0]
        if kind == "nan":    # the maxima skip it
            assert all(bool(torch.isfinite(rows[r, c])) for r in hit for c in (D.GRAD_MAXABS, D.WEIGHT_MAXABS))
        else:
            assert float(rows[i, D.GRAD_MAXABS]) == float("inf") and float(rows[i + 2, D.WEIGHT_MAXABS]) == float("inf")
        assert w.guards_intact()


def run_only_nan(be):
    """a tensor that holds nothing but NaN: its maxima are 0"""
    w = World(be, "mixed", True, False, seed=3)
    off = w.seg_off_h.tolist()
    for i in (0, 4):    # 1 and 3 elements
        w.host["g"][off[i]:off[i + 1]] = float("nan")
    w.upload()
    assert w.call() == 0
    rows = w.rows()
    check_table(rows, w.ref(), True, "only NaN")
    assert float(rows[0, D.GRAD_MAXABS]) == 0.0 and float(rows[4, D.GRAD_MAXABS]) == 0.0 and float(rows[4, D.GRAD_NONFINITE]) == 3.0


def run_extremes(be):
    """-0, a denormal, 1e25 and 3e-30 in gradients and weights (squares far outside fp32), v = 0"""
    w = World(be, "mixed", True, True, seed=11)
    off = w.seg_off_h.tolist()
    for k in "gp":
        h = w.host[k]
        h[off[1]:off[2]] = 3e-30              # a tensor of 4097 tiny values: every fp32 square underflows to 0
        h[off[2]] = -0.0
        h[off[2] + 1] = 1e-40                 # denormal
        h[off[5] + 7] = 1e25                  # its fp32 square is Inf
        h[off[6]:off[7]] = 1e25
        h[off[3]:off[4]] = -0.0               # a tensor of nothing but -0: norm 0, maximum +0
    w.host["v"][off[5]:off[5] + 100] = 0.0
    w.host["v"][off[0]] = 0.0
    w.host["m"][off[0]] = 0.0
    w.upload()
    assert w.call() == 0
    rows, ref = w.rows(), w.ref()
    check_table(rows, ref, True, "extremes")
    assert bool(torch.isfinite(rows).all()) and float(rows[1, D.GRAD_NORM]) > 0.0 and float(rows[6, D.WEIGHT_NORM]) > 1e26
    assert same_bits(rows[3, :4], torch.zeros(4)), "a tensor of -0 must give +0 norms and maxima"
    assert w.guards_intact()


def run_due(be):
    """EVERY = 3 over 7 calls: calls 3 and 6 compute; the others leave table and workspace bit for bit and advance PHASE and AGE"""
    w = World(be, "mixed", True, False, seed=13, every=3)
    expect = [(1.0, 0.0, 1.0), (2.0, 0.0, 2.0), (0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (2.0, 0.0, 2.0), (0.0, 1.0, 0.0), (1.0, 0.0, 1.0)]
    for n, exp in enumerate(expect):
        w.host["g"] = rn(w.total, 700 + n, 0.3)      # a new gradient every call
        w.upload()
        before = w.snapshot()
        assert w.call() == 0
        assert w.ctl_words() == exp, "call %d: (PHASE, COMPUTED, AGE) = %r, expected %r" % (n + 1, w.ctl_words(), exp)
        after = w.snapshot()
        if exp[1] == 0.0:
            assert bool((after[0] == before[0]).all() and (after[1] == before[1]).all()), "call %d is not due and wrote" % (n + 1)
            if n < 2:
                assert w.untouched()
        else:
            check_table(w.rows(), w.ref(), True, "call %d" % (n + 1))
        assert w.guards_intact()


SKIP_CASES = [(1, 0.0), (1, 1.0), (1, 2.0), (0, 1.0)]


def run_on_skip(be, on_skip, skip_now):
    """EVERY = 5: the phase rule is silent; only ON_SKIP with SKIP_NOW == 1 computes (2 is a hold), and PHASE keeps counting"""
    w = World(be, "mixed", True, True, seed=17, every=5, on_skip=on_skip, skip_now=skip_now)
    due = on_skip == 1 and skip_now == 1.0
    for n in range(2):
        assert w.call() == 0
        assert w.ctl_words() == (float(n + 1), 1.0 if due else 0.0, 0.0 if due else float(n + 1))
    if due:
        check_table(w.rows(), w.ref(), True, "on skip")
    else:
        assert w.untouched()
    assert w.guards_intact()


def run_on_skip_without_state(be):
    """without moments there is no state record: ON_SKIP cannot fire"""
    w = World(be, "mixed", False, False, seed=17, every=5, on_skip=1, skip_now=1.0)
    assert w.call() == 0
    assert w.ctl_words() == (1.0, 0.0, 1.0) and w.untouched()


def run_every_lowered(be):
    """EVERY = 10 for four calls, then EVERY = 2 with PHASE = 4: the next call is due and PHASE starts again"""
    w = World(be, "mixed", True, False, seed=19, every=10)
    for n in range(4):
        assert w.call() == 0
    assert w.ctl_words() == (4.0, 0.0, 4.0) and w.untouched()
    w.put_ctl(D.C_EVERY, 2)
    assert w.call() == 0
    assert w.ctl_words() == (0.0, 1.0, 0.0)
    check_table(w.rows(), w.ref(), True, "EVERY lowered")
    assert w.call() == 0
    assert w.ctl_words() == (1.0, 0.0, 1.0)
    assert w.call() == 0
    assert w.ctl_words() == (0.0, 1.0, 0.0)


def run_age_saturates(be):
    w = World(be, "one", True, False, every=D.MAX_EVERY - 1)
    w.put_ctl(D.C_AGE, D.AGE_MAX - 1)
    for _ in range(2):
        assert w.call() == 0
        assert w.ctl_words()[2] == float(D.AGE_MAX)
    assert w.untouched()


def run_small_workspace(be):
    """a workspace that passes the launcher's check (one record per tensor) but not the plan's item count: nothing is computed and
    nothing outside it is written"""
    w = World(be, "mixed", True, False, seed=23, ws_items=len(MIXED))
    assert w.items > w.ws_items
    assert w.call() == 0
    assert w.ctl_words() == (0.0, 0.0, 1.0) and w.untouched() and w.guards_intact()


def all_cases():
    out = [("run_geometry", c) for c in GEO_CASES] + [("run_bit_equal", (g,)) for g in BITEQ_CASES] + [("run_nonfinite", (k,)) for k in NONFINITE_CASES]
    out += [("run_only_nan", ()), ("run_extremes", ()), ("run_due", ())] + [("run_on_skip", c) for c in SKIP_CASES]
    out += [("run_on_skip_without_state", ()), ("run_every_lowered", ()), ("run_age_saturates", ()), ("run_small_workspace", ())]
    return out


def case_id(case):
    return case[0][4:] + "".join("-%s" % (a,) for a in case[1])


# ---- the CPU emulation -----------------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "segment_end_off_by_one": [("run_geometry", ("one", 1, 0)), ("run_geometry", ("mixed", 1, 0)), ("run_geometry", ("many", 0, 1))],
    "short_last_chunk_dropped": [("run_geometry", ("mixed", 1, 0)), ("run_geometry", ("big", 0, 0)), ("run_geometry", ("pad", 1, 1))],
    "squares_in_fp32": [("run_extremes", ())],
    "nan_enters_the_maximum": [("run_nonfinite", ("nan",)), ("run_only_nan", ())],
    "scale_omitted": [("run_geometry", ("mixed", 1, 1)), ("run_geometry", ("one", 0, 1)), ("run_extremes", ())],
    "row_S_misses_the_last_tensor": [("run_geometry", ("one", 1, 0)), ("run_geometry", ("mixed", 0, 0)), ("run_geometry", ("many", 1, 1))],
    "direction_without_inv_sqrt_bc2": [("run_geometry", ("mixed", 1, 0)), ("run_geometry", ("big", 1, 1))],
    "phase_rule_fires_at_phase_0": [("run_due", ()), ("run_on_skip", (1, 2.0)), ("run_every_lowered", ())],
    "hold_treated_as_skip": [("run_on_skip", (1, 2.0))],
}


def _f32(x):
    return np.float32(x)


class TsEmu:
    """vptr_tensor_stats on CPU tensors: the plan's items, one partial per item, the tensors' sums in item order, row S in tensor order,
    the due rule and the record updates.  The Adam direction is formed in fp32 (the fma as one rounding of the exact fp64 value).
    `mutation`: one of MUTATIONS, a named defect."""

    dev = "cpu"

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS, mutation
        self.mut = mutation

    def sync(self):
        pass

    def call(self, p, g, m, v, seg_off, item_first, S, scale, state, ctl, table, ws, ws_bytes, grid_cap):
        mut = self.mut
        if any(t is None for t in (p, g, seg_off, item_first, ctl, table, ws)) or not 1 <= S <= D.MAX_TENSORS or grid_cap < 0:
            return -1
        if ws_bytes < S * D.PART_BYTES or not ((m is None) == (v is None) == (state is None)):
            return -1
        mom = m is not None
        c = ctl.numpy()
        phase, every, age = c[D.C_PHASE], c[D.C_EVERY], c[D.C_AGE]
        fire = bool(phase + _f32(1) >= every) or (mut == "phase_rule_fires_at_phase_0" and phase == 0)
        skip_now = float(state[S_SKIP_NOW]) if state is not None else 0.0
        skip = c[D.C_ON_SKIP] != 0 and state is not None and (skip_now == 1.0 or (mut == "hold_treated_as_skip" and skip_now != 0.0))
        so, it = seg_off.tolist(), item_first.tolist()
        computed = (fire or skip) and it[S] <= ws_bytes // D.PART_BYTES
        if computed:
            P, G = p.numpy(), g.numpy()
            if mom:
                isb, eps = _f32(state[S_INV_SQRT_BC2]), _f32(state[S_EPS])
                if mut == "direction_without_inv_sqrt_bc2":
                    isb = _f32(1)
            parts = ws.numpy().reshape(-1, 5)
            # stage 1: one partial per item
            for item, (i, a, b) in enumerate(D.items_of(seg_off, item_first)):
                if mut == "segment_end_off_by_one":
                    b = min(b, so[i + 1] - 1)
                if mut == "short_last_chunk_dropped" and b - a < D.CHUNK:
                    b = a
                gi, pi = G[a:b], P[a:b]
                with np.errstate(all="ignore"):
                    if mut == "squares_in_fp32":
                        sg, sp = float((gi * gi).astype(np.float64).sum()), float((pi * pi).astype(np.float64).sum())
                    else:
                        sg, sp = float((gi.astype(np.float64) ** 2).sum()), float((pi.astype(np.float64) ** 2).sum())
                    sd = 0.0
                    if mom:
                        den = (np.sqrt(v.numpy()[a:b]).astype(np.float64) * np.float64(isb) + np.float64(eps)).astype(np.float32)   # fmaf
                        d = m.numpy()[a:b] / den
                        sd = float((d.astype(np.float64) ** 2).sum())

                    def mx(x):
                        if mut == "nan_enters_the_maximum":
                            return float(np.abs(x).max()) if x.size else 0.0
                        x = x[~np.isnan(x)]
                        return float(np.abs(x).max()) if x.size else 0.0
                    rec = np.array([sg, sp, sd, 0.0, 0.0])
                    rec[3:4].view(np.float32)[:] = [mx(gi), mx(pi)]
                    rec[4:5].view(np.uint32)[:] = [int((~np.isfinite(gi)).sum()), int((~np.isfinite(pi)).sum())]
                parts[item] = rec
            # stage 2: the tensors in item order, row S in tensor order
            s = np.float64(1.0 if scale is None or mut == "scale_omitted" else float(scale[0]))
            tab = table.numpy().reshape(S + 1, 8)

            def write(r, tot, n):
                with np.errstate(all="ignore"):
                    tab[r] = [_f32(np.sqrt(tot[0]) * s), _f32(np.sqrt(tot[1])), _f32(np.float64(tot[5]) * s), _f32(tot[6]),
                              _f32(np.sqrt(tot[2] / np.float64(n))) if mom else _f32(0), _f32(tot[3]), _f32(tot[4]), _f32(np.float64(n))]
            whole = [np.float64(0)] * 5 + [_f32(0), _f32(0)]
            fmax = np.maximum if mut == "nan_enters_the_maximum" else np.fmax
            with np.errstate(all="ignore"):
                for i in range(S):
                    tot = [np.float64(0)] * 5 + [_f32(0), _f32(0)]     # sum g^2, p^2, d^2, count g, count p, max g, max p
                    for item in range(it[i], it[i + 1]):
                        rec = parts[item]
                        mg, mp = rec[3:4].view(np.float32)
                        ng, np_ = rec[4:5].view(np.uint32)
                        tot = [tot[0] + rec[0], tot[1] + rec[1], tot[2] + rec[2], tot[3] + np.float64(ng), tot[4] + np.float64(np_),
                               fmax(tot[5], mg), fmax(tot[6], mp)]
                    write(i, tot, so[i + 1] - so[i])
                    if not (mut == "row_S_misses_the_last_tensor" and i == S - 1):
                        whole = [whole[k] + tot[k] for k in range(5)] + [fmax(whole[5], tot[5]), fmax(whole[6], tot[6])]
                write(S, whole, so[S])
        c[D.C_PHASE] = 0.0 if fire else phase + _f32(1)
        c[D.C_COMPUTED] = 1.0 if computed else 0.0
        c[D.C_AGE] = 0.0 if computed else min(age + _f32(1), _f32(D.AGE_MAX))
        return 0
