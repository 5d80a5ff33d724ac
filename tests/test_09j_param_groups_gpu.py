"""Parameter groups of the device-resident optimizer controls (csrc/optim.hip) through the C ABI (include/vptr_hip_groups.h):
vptr_optim_group_scalars (the per-group rate, step size and decay against their definitions, bit identity with the state record at
lr_scale 1, skip and hold) and vptr_adamw_groups in both forms (every size and launch class, each pointer off its grid, group boundaries
inside a float4 / at a multiple of 1024 / at the last element, an empty group, 1 / 2 / 16 groups, a map byte out of range, bit identity
with vptr_adamw_ctl and vptr_adamw_ctl_ema for any map, scales 0 / 0.1 / 1 / 2.5 and decays 0 / 0.01 at steps 1, 2, 10, 1000 against
fp64 torch.optim.AdamW semantics, a group at lr_scale 0, skip and hold), the rejects of both, and the five launches of a grouped step
captured into one graph and replayed with one group's record rewritten in between.

The cases, guarded buffers, references and bars live in tests/param_groups_cases.py, which tests/test_param_groups_cpu.py also runs against
a CPU emulation and its mutations; this file supplies the backend that hands the pointers to the library.  Measured distances:
profiles/param_groups.md."""
import pytest
import torch

import optim_ctl_cases as C
import param_groups_cases as G

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: tensors become raw device pointers, the current stream is appended, the return code comes back"""

    def __init__(self, dev):
        from vptr_amd import _lib
        self.dev, self.lib = dev, _lib

    def call(self, name, *args):
        L = self.lib
        for a in args:
            assert not isinstance(a, torch.Tensor) or (a.is_cuda and a.is_contiguous())
        raw = [L.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
        return getattr(L.lib, "vptr_" + name)(*raw, L.stream())

    def last_error(self):
        return self.lib.lib.vptr_last_error().decode()

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a parameter-group call: %s" % e, returncode=3)

    def group_map(self, layout, group_of, numel):
        from vptr_amd.optim import group_map
        return group_map(layout, group_of, numel)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.mark.parametrize("size,ema", G.SIZE_CASES, ids=lambda x: str(x))
def test_sizes(be, size, ema):
    """n = 1, 3, 4, 5, 1027, 4 195 507 with three groups mixed element by element, against the ungrouped kernel run once per group"""
    G.run_sizes(be, size, ema)


@pytest.mark.parametrize("size,shift,ema", G.SHIFT_CASES, ids=lambda x: str(x))
def test_one_pointer_off_its_grid(be, size, shift, ema):
    G.run_shift(be, size, shift, ema)


@pytest.mark.parametrize("where,ema", G.BOUND_CASES, ids=lambda x: str(x))
def test_group_boundary(be, where, ema):
    G.run_boundary(be, where, ema)


@pytest.mark.parametrize("ngroups,kind,ema", G.NGROUPS_CASES, ids=lambda x: str(x))
def test_group_counts(be, ngroups, kind, ema):
    G.run_ngroups(be, ngroups, kind, ema)


@pytest.mark.parametrize("ema", [0, 1])
def test_group_without_elements(be, ema):
    G.run_empty_group(be, ema)


@pytest.mark.parametrize("ema", [0, 1])
def test_map_byte_out_of_range_stays_inside_the_table(be, ema):
    G.run_byte_out_of_range(be, ema)


def test_pad_elements_belong_to_group_0(be):
    G.run_pad_group(be)


@pytest.mark.parametrize("size,ngroups,ema", G.IDENT_CASES, ids=lambda x: str(x))
def test_default_groups_are_bit_identical_to_the_ungrouped_kernels(be, size, ngroups, ema):
    G.run_identity(be, size, ngroups, ema)


def test_group_scalars(be):
    G.run_scalars(be)


@pytest.mark.parametrize("k,ema", G.REF_CASES, ids=lambda x: str(x))
def test_against_fp64_adamw_with_param_groups(be, k, ema):
    G.run_fp64(be, k, ema)


def test_lr_scale_0_keeps_special_values(be):
    G.run_scale0_special_values(be)


@pytest.mark.parametrize("size,skip_now,ema", G.SKIP_CASES, ids=lambda x: str(x))
def test_skip_and_hold_write_nothing(be, size, skip_now, ema):
    G.run_skip(be, size, skip_now, ema)


def test_group_scalars_rejects(be):
    G.run_scalars_rejects(be)


def test_adamw_groups_rejects(be):
    G.run_groups_rejects(be)


# ------------------------------------------------------------------------------------------------------------------ under a graph
def _grouped_step(be, r, gh, gs, grad, p, m, v, gid, sumsq, ws, n, const):
    """the launches of one grouped step behind a stand-in for the backward pass: sumsq -> prepare -> group scalars -> update"""
    grad.add_(const)
    assert be.call("sumsq_ws", grad, n, sumsq, ws, ws.numel()) == 0
    assert be.call("optim_prepare", r.hr.out, r.sr.out, r.st.out, sumsq) == 0
    assert be.call("optim_group_scalars", r.sr.out, gh.out, gs.out, 3) == 0
    assert be.call("adamw_groups", p, grad, m, v, None, gid, n, r.sr.out, None, gs.out, 3) == 0


def test_captured_step_follows_the_group_records(be, dev):
    """captured once, replayed 4 times; between replays 2 and 3 group 1's lr_scale goes 0 -> 0.5 and its weight_decay 0 -> 0.2 by the
    host's one-word fills: group 1's parameters stand still for two replays and move afterwards, and every buffer and record is
    torch.equal to the same calls issued eagerly"""
    from vptr_amd.optim import LRSchedule
    from vptr_amd.train import graph_node_census
    n = 1027
    sched = LRSchedule("cosine", warmup_steps=1, total_steps=4, min_ratio=0.1)
    hyper, p0 = C.hyper_words(max_norm=1.0, sched=sched), C.adamw_inputs(n, 1, C.HYPER["b1"], C.HYPER["b2"])[0]
    gid = G.make_map(n, 3, seed=2)
    specs = [(1.0, G.WD), (0.0, 0.0), (2.5, 0.05)]

    def world():
        r = G.Recs(be, 0, hyper)
        gh, gs = G.Tab(dev, G.ghyper_words(specs)), G.Tab(dev, G.fresh_gstate())
        bufs = [C.Guard(n, dev, start=t) for t in (G.rn((n,), 9700, 0.3), p0, torch.zeros(n), torch.zeros(n))]      # grad, p, m, v
        return r, gh, gs, bufs, G.ByteGuard(gid, dev), torch.zeros(1, device=dev), torch.empty(1024, device=dev)

    def run(step_fn, gh, bufs):
        ps = []
        for i in range(4):
            if i == 2:
                gh.out[G.G_WORDS + G.GH["LR_SCALE"]:G.G_WORDS + G.GH["LR_SCALE"] + 1].fill_(0.5)
                gh.out[G.G_WORDS + G.GH["WEIGHT_DECAY"]:G.G_WORDS + G.GH["WEIGHT_DECAY"] + 1].fill_(0.2)
            step_fn()
            be.sync()
            ps.append(bufs[1].out.cpu().clone())
        return ps

    re_, ghe, gse, be_, mpe, sse, wse = world()
    eager = run(lambda: _grouped_step(be, re_, ghe, gse, *[b.out for b in be_], mpe.out, sse, wse, n, 0.25), ghe, be_)
    g1 = gid == 1
    assert G.same_bits(eager[1][g1], p0[g1]) and not bool((G.bits(eager[2][g1]) == G.bits(eager[1][g1])).any())
    assert not bool((G.bits(eager[0][~g1]) == G.bits(p0[~g1])).any())
    rg, ghg, gsg, bg, mpg, ssg, wsg = world()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        _grouped_step(be, rg, ghg, gsg, *[b.out for b in bg], mpg.out, ssg, wsg, n, 0.25)
    census = graph_node_census(graph)
    assert set(census) == {"kernel"} and census["kernel"] >= 5, census
    graph.instantiate()
    be.sync()
    assert all(b.untouched() for b in bg) and gsg.untouched() and float(rg.st.out) == 0.0, "capturing ran the kernels"
    replayed = run(graph.replay, ghg, bg)
    for i, (x, y) in enumerate(zip(replayed, eager)):
        assert G.same_bits(x, y), "p after replay %d differs from the eager calls" % i
    for name, x, y in zip(("grad", "p", "m", "v"), bg, be_):
        assert x.guards_intact() and G.same_bits(x.out.cpu(), y.out.cpu()), "%s differs between the replays and the eager calls" % name
    assert G.same_bits(rg.sr.words(), re_.sr.words()) and G.same_bits(gsg.words(), gse.words()) and mpg.untouched()
    lr_now = float(rg.sr.words()[C.S["LR_NOW"]])
    assert float(gsg.words()[G.G_WORDS + G.GS["LR"]]) == G.f32(G.F(lr_now) * G.F(0.5)) and float(rg.st.out) == 4.0
