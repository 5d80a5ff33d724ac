"""Per-tensor statistics of the optimizer's slabs (csrc/tensor_stats.hip) through the C ABI (include/vptr_hip_diag.h): every geometry
(one element, tensors of 1 .. 8195 elements whose starts hit all four residues of the 16-byte grid, the slabs one float off that grid and
in four different phases of it, 700 tiny tensors on three workgroups, one tensor of 70 001 elements, NaN pad elements) with and without
moments and with and without a scale, against the fp64 builder inside the derived bars; NaN, +Inf and -Inf at tensor boundaries; -0, a
denormal, 1e25, 3e-30 and v = 0; bit equality across grids and calls; the due rule, ON_SKIP, EVERY lowered, the saturating AGE and a
workspace too small for the plan; every reject; and the call captured into a graph and replayed.

The cases, guarded buffers, references and bars live in tests/tensor_stats_cases.py, which tests/test_tensor_stats_cpu.py also runs against
a CPU emulation and its mutations; this file supplies the backend that hands the pointers to the library.  Every slab is at most 70 k
floats.  Measured distances: profiles/tensor_stats.md."""
import pytest
import torch

import tensor_stats_cases as T
from vptr_amd import diagnostics as D

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: tensors become raw device pointers, the current stream is appended, the return code comes back"""

    def __init__(self, dev):
        from vptr_amd import _lib
        self.dev, self.lib = dev, _lib

    def call(self, *args):
        L = self.lib
        for a in args:
            assert not isinstance(a, torch.Tensor) or (a.is_cuda and a.is_contiguous())
        raw = [L.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
        return L.lib.vptr_tensor_stats(*raw, L.stream())

    def last_error(self):
        return self.lib.lib.vptr_last_error().decode()

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a tensor-statistics call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.mark.parametrize("geo,moments,scaled", T.GEO_CASES, ids=lambda x: str(x))
def test_geometry_against_fp64(be, geo, moments, scaled):
    worst = T.run_geometry(be, geo, moments, scaled)
    print("%s moments %d scaled %d: worst norm %.3f, worst dir_rms %.3f of their bars" % (geo, moments, scaled, worst["norm"], worst["dir"]))


@pytest.mark.parametrize("geo", T.BITEQ_CASES)
def test_table_is_bit_identical_across_grids_and_calls(be, geo):
    T.run_bit_equal(be, geo)


@pytest.mark.parametrize("kind", T.NONFINITE_CASES)
def test_nonfinite_stays_in_its_tensor(be, kind):
    T.run_nonfinite(be, kind)


def test_tensor_of_nothing_but_nan(be):
    T.run_only_nan(be)


def test_extreme_values_and_v_zero(be):
    T.run_extremes(be)


def test_due_rule_over_seven_calls(be):
    T.run_due(be)


@pytest.mark.parametrize("on_skip,skip_now", T.SKIP_CASES, ids=lambda x: str(x))
def test_on_skip(be, on_skip, skip_now):
    T.run_on_skip(be, on_skip, skip_now)


def test_on_skip_without_a_state_record(be):
    T.run_on_skip_without_state(be)


def test_every_lowered_below_phase(be):
    T.run_every_lowered(be)


def test_age_saturates(be):
    T.run_age_saturates(be)


def test_workspace_smaller_than_the_plan(be):
    T.run_small_workspace(be)


def test_rejects_write_and_launch_nothing(be):
    w = T.World(be, "mixed", True, True, seed=1)
    names = ["p", "g", "m", "v", "seg_off", "item_first", "S", "scale", "state", "ctl", "table", "ws", "ws_bytes", "grid_cap"]
    good = [w.slab["p"], w.slab["g"], w.slab["m"], w.slab["v"], w.seg_off, w.item_first, w.S, w.scale, w.state, w.ctl, w.table, w.ws,
            w.items * D.PART_BYTES, 0]

    def bad(**kw):
        assert be.call(*[kw.get(n, a) for n, a in zip(names, good)]) != 0, kw
        assert be.last_error().startswith("tensor_stats"), be.last_error()

    for name in ("p", "g", "seg_off", "item_first", "ctl", "table", "ws"):
        bad(**{name: None})
    for S in (0, -1, 65536):
        bad(S=S)
    bad(ctl=w.ctl[1:])
    bad(table=w.table[1:])
    bad(table=w.table[8:])          # a row further: 32 bytes
    bad(ws=w.ws.view(torch.float32)[1:])
    bad(ws_bytes=w.S * D.PART_BYTES - 1)
    bad(ws_bytes=-1)
    for absent in (("m",), ("v",), ("state",), ("m", "v"), ("m", "state"), ("v", "state")):
        bad(**{n: None for n in absent})
    bad(state=w.state[4:])
    bad(grid_cap=-1)
    be.sync()
    assert w.untouched() and w.guards_intact() and w.ctl_words() == (0.0, 0.0, 0.0)
    assert be.call(*good) == 0
    be.sync()
    T.check_table(w.rows(), w.ref(), True, "after the rejects")


def test_captured_call_follows_gradient_and_control_record(be, dev):
    """captured once (two kernel nodes, nothing else), replayed four times at EVERY = 2 with the gradient rewritten before every replay:
    replays 2 and 4 compute, from the gradient of their own replay; 1 and 3 leave the table bit for bit"""
    from vptr_amd.train import graph_node_census
    w = T.World(be, "mixed", True, True, seed=29, every=2)
    mom = (w.slab["m"], w.slab["v"])
    args = (w.slab["p"], w.slab["g"], *mom, w.seg_off, w.item_first, w.S, w.scale, w.state, w.ctl, w.table, w.ws, w.items * D.PART_BYTES, 0)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        assert be.call(*args) == 0
    census = graph_node_census(graph)
    assert census == {"kernel": 2}, census
    graph.instantiate()
    be.sync()
    assert w.untouched() and w.ctl_words() == (0.0, 0.0, 0.0), "capturing ran the kernels"
    lead = w.leads["g"]
    for n in range(4):
        w.host["g"] = T.rn(w.total, 900 + n, 0.3)
        w.bufs["g"][lead:lead + w.total].copy_(w.host["g"].to(dev))      # in place: the graph holds the address
        before = w.snapshot()
        graph.replay()
        be.sync()
        if n % 2 == 0:
            assert w.ctl_words() == (1.0, 0.0, 1.0), (n, w.ctl_words())
            after = w.snapshot()
            assert bool((after[0] == before[0]).all() and (after[1] == before[1]).all()), "replay %d is not due and wrote" % (n + 1)
        else:
            assert w.ctl_words() == (0.0, 1.0, 0.0), (n, w.ctl_words())
            T.check_table(w.rows(), w.ref(), True, "replay %d" % (n + 1))
    w._in["g"] = T.bits(w.bufs["g"])
    assert w.guards_intact()
