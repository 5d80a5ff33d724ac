"""Gradient accumulation and EMA weights of the device-resident optimizer controls (csrc/optim.hip) through the C ABI
(include/vptr_hip_accum.h): vptr_accum_begin (zero-fill at a window start, the partial sum left alone otherwise, every launch class),
vptr_optim_prepare_accum (bit identity with vptr_optim_prepare at k = 1, the window sequences at k = 3, non-finite sums on a hold and on a
close, k lowered inside a window, the EMA coefficient against its fp64 mirror), vptr_adamw_ctl_ema (p / m / v bit-identical to
vptr_adamw_ctl, the EMA within two roundings, skip and hold, a 12-step trajectory against torch.optim.AdamW in fp64 with the EMA of its
parameters), vptr_slab_swap, the rejects of all four, and the five launches of a micro-step captured into one graph.

The cases, guarded records, references and bars live in tests/accum_cases.py, which tests/test_accum_cpu.py also runs against a CPU
emulation and its mutations; this file supplies the backend that hands the pointers to the library (test_09e's).  Measured distances:
profiles/accum_ema.md."""
import pytest
import torch

import accum_cases as A
import optim_ctl_cases as C

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
            pytest.exit("GPU error after an accumulation / EMA call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


# -------------------------------------------------------------------------------------------------------------- 1. vptr_accum_begin
@pytest.mark.parametrize("size,shift,micro", A.BEGIN, ids=lambda x: str(x))
def test_accum_begin(be, size, shift, micro):
    """n = 1, 3, 4, 1027, 4 195 507; the pointer aligned and one float in; MICRO = 0 zeroes, MICRO = 1 and 2 leave seeded content (NaNs
    included) bit for bit"""
    A.run_begin(be, size, shift, micro)


def test_accum_begin_rejects(be):
    A.run_begin_rejects(be)


# ------------------------------------------------------------------------------------------------------ 2. vptr_optim_prepare_accum
def test_prepare_accum_k1_is_bit_identical_to_prepare(be):
    A.run_prepare_k1(be)


def test_prepare_accum_k3_sequences_and_rates(be):
    A.run_prepare_k3(be)


def test_prepare_accum_ignores_a_nonfinite_sum_on_a_hold(be):
    A.run_prepare_nonfinite_hold(be)


@pytest.mark.parametrize("skip", [0, 1])
def test_prepare_accum_nonfinite_sum_on_the_close(be, skip):
    A.run_prepare_nonfinite_close(be, skip)


def test_prepare_accum_k_lowered_inside_a_window(be):
    A.run_prepare_lower_k(be)


@pytest.mark.parametrize("warm,d", A.OMD)
def test_prepare_accum_ema_coefficient(be, warm, d):
    A.run_ema_omd(be, warm, d)


def test_prepare_accum_rejects(be):
    A.run_prepare_accum_rejects(be)


# ------------------------------------------------------------------------------------------------------------ 3. vptr_adamw_ctl_ema
@pytest.mark.parametrize("size,shift", A.EMA_LAUNCH, ids=lambda x: str(x))
def test_adamw_ctl_ema_matches_adamw_ctl_and_the_ema_bound(be, size, shift):
    A.run_ema_same_bits(be, size, shift)


@pytest.mark.parametrize("size,skip_now", A.EMA_SKIP, ids=lambda x: str(x))
def test_adamw_ctl_ema_returns_on_skip_and_hold(be, size, skip_now):
    A.run_ema_skip(be, size, skip_now)


def test_adamw_ctl_ema_rejects(be):
    A.run_ema_rejects(be)


def test_adamw_ctl_ema_trajectory_vs_torch_adamw_and_its_ema(be):
    A.run_ema_trajectory(be)


# ---------------------------------------------------------------------------------------------------------------- 4. vptr_slab_swap
@pytest.mark.parametrize("size,shift", A.SWAP, ids=lambda x: str(x))
def test_slab_swap(be, size, shift):
    A.run_swap(be, size, shift)


def test_slab_swap_rejects(be):
    A.run_swap_rejects(be)


# ------------------------------------------------------------------------------------------------------------------ 5. under a graph
def _micro_step(be, r, grad, p, m, v, ema, sumsq, ws, n, const):
    """the launches of one micro-step: begin -> a stand-in for the backward pass (adds a constant to the slab) -> sumsq -> prepare -> update"""
    assert be.call("accum_begin", grad, n, r.wr.out) == 0
    grad.add_(const)
    assert be.call("sumsq_ws", grad, n, sumsq, ws, ws.numel()) == 0
    assert be.call("optim_prepare_accum", r.hr.out, r.sr.out, r.wr.out, r.st.out, sumsq) == 0
    assert be.call("adamw_ctl_ema", p, grad, m, v, ema, n, r.sr.out, r.wr.out) == 0


def test_captured_micro_step_follows_the_window_record(be, dev):
    """the five launches captured once and replayed 6 times at k = 3, ACCUM_STEPS rewritten to 2 between replays 3 and 4 (a window
    boundary): closes at replays 3 and 5, and every buffer and record torch.equal to the same calls issued eagerly"""
    from vptr_amd.optim import LRSchedule
    from vptr_amd.train import graph_node_census
    n = 1027
    sched = LRSchedule("cosine", warmup_steps=1, total_steps=4, min_ratio=0.1)
    hyper, p0 = C.hyper_words(max_norm=1.0, grad_scale=1.0 / 3.0, sched=sched), C.adamw_inputs(n, 1, C.HYPER["b1"], C.HYPER["b2"])[0]

    def world():
        r = A.Records(be, hyper, A.window_words(k=3, d=0.9, warm=1))
        bufs = [C.Guard(n, dev, start=t) for t in (A.seeded(n, 8700), p0, torch.zeros(n), torch.zeros(n), p0)]      # grad, p, m, v, ema
        return r, bufs, torch.zeros(1, device=dev), torch.empty(1024, device=dev)

    def run(step_fn, r):
        seq = []
        for i in range(6):
            if i == 3:
                r.host_write(A.W["ACCUM_STEPS"], 2.0)
            step_fn()
            be.sync()
            seq.append((float(r.wr.out[A.W["MICRO"]]), float(r.wr.out[A.W["APPLY_NOW"]]), float(r.st.out)))
        return seq

    re_, be_, sse, wse = world()
    eager = run(lambda: _micro_step(be, re_, *[b.out for b in be_], sse, wse, n, 0.25), re_)
    assert eager == [(1.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (0.0, 1.0, 2.0), (1.0, 0.0, 2.0)], eager
    rg, bg, ssg, wsg = world()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        _micro_step(be, rg, *[b.out for b in bg], ssg, wsg, n, 0.25)
    census = graph_node_census(graph)
    assert set(census) == {"kernel"} and census["kernel"] >= 5, census
    graph.instantiate()
    be.sync()
    assert all(b.untouched() for b in bg) and float(rg.st.out) == 0.0, "capturing ran the kernels"
    assert run(graph.replay, rg) == eager
    for name, x, y in zip(("grad", "p", "m", "v", "ema"), bg, be_):
        assert x.guards_intact() and A.same_bits(x.out.cpu(), y.out.cpu()), "%s differs between the replays and the eager calls" % name
    assert A.same_bits(rg.sr.words(), re_.sr.words()) and A.same_bits(rg.wr.words(), re_.wr.words())
    assert not A.same_bits(bg[1].out.cpu(), p0) and not A.same_bits(bg[4].out.cpu(), bg[1].out.cpu())
    # the slab holds one micro-step of the open third window: 0.25 everywhere, the seeded content (a NaN included) long gone
    assert A.same_bits(bg[0].out.cpu(), torch.full((n,), 0.25))
