"""The device-resident optimizer controls of csrc/optim.hip through the C ABI (include/vptr_hip_optim.h): vptr_optim_prepare alone (step and
lr_now over 41 steps of the three schedule kinds against the host mirror, the schedule's edges, the update scalars per step count and beta
pair, the clip coefficient with grad_scale, the non-finite decision word by word, the counters over good / bad / bad / good) and
vptr_adamw_ctl (bit identity with vptr_adamw in every launch class, under a cosine schedule step by step, a 12-step trajectory against
torch.optim.AdamW + LambdaLR + clip_grad_norm_ in fp64, the skipped step, the rejects), then both captured into one graph and replayed.

The cases, the guarded records, the references and the bars live in tests/optim_ctl_cases.py, which tests/test_optim_ctl_cpu.py also runs
against a CPU emulation and its mutations; this file supplies the backend that hands the pointers to the library.  Measured distances:
profiles/optim_ctl.md."""
import pytest
import torch

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
            pytest.exit("GPU error after an optimizer-control call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


# ------------------------------------------------------------------------------------------------------------ 1. vptr_optim_prepare
@pytest.mark.parametrize("kind", C.KINDS)
def test_prepare_schedule(be, kind):
    """k = 0 .. 40 with W = 5, S = 30, r = 0.1: step_dev counts, lr_now within one fp32 ulp of base_lr * LRSchedule.factor(k)"""
    C.run_prepare_schedule(be, kind)


@pytest.mark.parametrize("edge", sorted(C.SCHED_EDGES))
def test_prepare_schedule_edges(be, edge):
    """W = 0, S = W, W = 1, each of the three kinds, run past S where the factor stays at r"""
    C.run_prepare_schedule_edges(be, edge)


@pytest.mark.parametrize("betas", C.ADAMW_BETAS, ids=lambda b: "%g_%g" % b)
@pytest.mark.parametrize("k", C.ADAMW_STEPS)
def test_prepare_update_scalars(be, k, betas):
    """the update scalars of step k at 4 ulp of a numpy fp32 evaluation of adamw_kernel's expressions, and the update they give (p0 = 0)
    against fp64 at test_09d's bar"""
    C.run_prepare_scalars(be, k, betas)


@pytest.mark.parametrize("case", sorted(C.CLIP))
def test_prepare_clip(be, case):
    """max_norm 0 and -1 (no clipping), the clip active and inactive, grad_scale 0.25 with each"""
    C.run_prepare_clip(be, case)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("which", sorted(C.NONFINITE))
def test_prepare_nonfinite(be, which, skip):
    C.run_prepare_nonfinite(be, which, skip)


def test_prepare_counters_over_good_bad_bad_good(be):
    C.run_prepare_sequence(be)


# ---------------------------------------------------------------------------------------------------------------- 2. vptr_adamw_ctl
@pytest.mark.parametrize("case", sorted(C.CTL_LAUNCH))
def test_adamw_ctl_is_bit_identical_to_adamw(be, case):
    """n = 1, 3, 4, 1027 and 4 195 507 (second grid-stride trip plus scalar tail), p / g / m / v in turn one float in (all-scalar path)"""
    C.run_ctl_same_bits_launch(be, case)


@pytest.mark.parametrize("wd", C.CTL_WD)
@pytest.mark.parametrize("clip", sorted(C.CTL_CLIP))
def test_adamw_ctl_is_bit_identical_clip_and_decay(be, clip, wd):
    C.run_ctl_same_bits_clip(be, clip, wd)


def test_adamw_ctl_is_bit_identical_with_the_stage1_settings(be):
    C.run_ctl_same_bits_stage1(be)


def test_adamw_ctl_cosine_steps_are_bit_identical_to_adamw_with_lr_now(be):
    C.run_ctl_cosine_same_bits(be)


def test_adamw_ctl_trajectory_vs_torch_adamw_lambda_lr(be):
    C.run_ctl_trajectory(be)


@pytest.mark.parametrize("case", sorted(C.CTL_SKIP_N))
def test_adamw_ctl_skip(be, case):
    C.run_ctl_skip(be, case)


def test_rejects(be):
    C.run_rejects(be)


# ------------------------------------------------------------------------------------------------------------------ 3. under a graph
def test_captured_prepare_and_update_follow_the_hyper_record(be, dev):
    """prepare + adamw_ctl as two kernel nodes of one graph, replayed 5 times: step and lr_now advance per replay; base_lr written between
    replays 2 and 3 shows in lr_now and in p (against vptr_adamw called eagerly with the expected rate, bit for bit)"""
    from vptr_amd.optim import LRSchedule
    n, sched = 1027, LRSchedule("linear", warmup_steps=2, total_steps=10, min_ratio=0.1)
    hyper = C.hyper_words(max_norm=1.0, sched=sched)
    hr, sr, st = C.Rec(dev, hyper), C.Rec(dev, C.fresh_state()), C.Guard(1, dev, start=torch.tensor([0.0]))
    p0, g, _, _ = C.adamw_inputs(n, 1, C.HYPER["b1"], C.HYPER["b2"])
    sumsq = C._sumsq_of(g)
    ss = C.scalar(sumsq, dev)
    pg, gd_, mg, vg = C._slabs(be, (p0, g, torch.zeros(n), torch.zeros(n)))
    C._ctl_step(be, (p0, g, torch.zeros(n), torch.zeros(n)), hyper, 0, sumsq)       # both kernels have run once before the capture (on other buffers)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert be.call("optim_prepare", hr.out, sr.out, st.out, ss) == 0
        assert be.call("adamw_ctl", pg.out, gd_, mg.out, vg.out, n, sr.out) == 0
    be.sync()
    assert pg.untouched() and float(st.out.cpu()) == 0.0, "capturing ran the kernels"
    base, cur = C.BASE_LR, (p0, torch.zeros(n), torch.zeros(n))
    for i in range(5):
        if i == 2:
            base = 4e-3
            hr.out[C.H["BASE_LR"]:C.H["BASE_LR"] + 1].fill_(base)          # a stream-ordered write, as FlatAdamW.set_lr issues it
        graph.replay()
        be.sync()
        words = sr.words()
        want_lr = C.f32(base) * sched.factor(i)
        assert float(st.out.cpu()) == i + 1
        assert abs(float(words[C.S["LR_NOW"]]) - want_lr) <= want_lr * C.ULP, (i, float(words[C.S["LR_NOW"]]), want_lr)
        cur = C._adamw_step(be, (cur[0], g, cur[1], cur[2]), dict(C.HYPER, lr=float(words[C.S["LR_NOW"]])), i + 1, sumsq, 1.0)
        got = C._slab_result((pg, mg, vg))
        C._assert_same("replay %d" % (i + 1), got, cur)
    assert float(words[C.S["LR_NOW"]]) > 2.0 * C.f32(C.BASE_LR)              # the new base rate, not the captured one
