"""Op-level fp64 parity of the tail of the train step through the C ABI: the fused losses of csrc/losses.hip (vptr_mse_gdl_fwd / _bwd with
more partials than one trip of the final kernel, one-row last bands, the minimum plane, W above the workgroup, either upstream scalar NULL,
exact ties; vptr_nce_fwd / _bwd in every NV class of the backward and on both sides of every class boundary, dead rows with partial token
chunks, channel widths that are no multiple of 16, both temperatures, gout present and NULL, the scratch's score / log-sum-exp sections, the
documented rejects), the optimizer of csrc/optim.hip (vptr_sumsq with its unrolled loop, unaligned branch and accumulate contract,
vptr_sumsq_ws, vptr_adamw in every launch class, with the clip active / inactive / absent, grad_scale, and the applied update at full fp32
resolution per step count), and the counter-based RNG of csrc/common.h bit for bit (vptr_dropout, vptr_droppath_scales).

The cases, the guarded buffers, the references and the bars live in tests/step_tail_cases.py, which tests/test_cpu.py also runs against a CPU
emulation of the calls; this file supplies the backend that hands the pointers to the library.  Measured distances:
profiles/step_tail_margins.md."""
import pytest
import torch

import step_tail_cases as C

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

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a step-tail call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


def _id(g):
    return "x".join("%g" % v for v in g)


# ------------------------------------------------------------------------------------- 1. vptr_mse_gdl_fwd / vptr_mse_gdl_bwd
@pytest.mark.parametrize("variant", sorted(C.MSE_VARIANTS))
@pytest.mark.parametrize("geom", sorted(C.MSE_GEOMS), ids=_id)
def test_mse_gdl(be, geom, variant):
    """mse, gdl (1e-6) and dpred (2e-6 rel-L2; the last band's rows element by element) against the oracle's mse_loss + gdl_loss in fp64, with
    unequal upstream scalars, either or both NULL (both: all zeros), pred == gt on the first rows and two equal neighbours in the last row
    (sign(0) = 0); the scratch is exactly planes * ceil(H / 16) * 3 floats between NaN guards"""
    C.run_mse_gdl(be, geom, variant)


def test_mse_gdl_rejects(be):
    C.run_mse_gdl_rejects(be)


# ------------------------------------------------------------------------------------------------ 2. vptr_nce_fwd / vptr_nce_bwd
@pytest.mark.parametrize("frames,L,C_,tau", C.nce_cases(), ids=[_id(c) for c in C.nce_cases()])
def test_nce(be, frames, L, C_, tau):
    """loss (2e-6), the scratch's inv / S / rlse / clse sections (2e-6 rel-L2) and dg, dp (1e-5; the last 64-row block of every frame on its
    own) against F.normalize + the oracle's bipatch_nce in fp64; gout = 1.3 and NULL; one all-zero token in g and one in p"""
    C.run_nce(be, frames, L, C_, tau)


def test_nce_c6_forward_only(be):
    C.run_nce_c6(be)


def test_nce_bwd_rejects(be):
    C.run_nce_bwd_rejects(be)


# ------------------------------------------------------------------------------------------------ 3. vptr_sumsq / vptr_sumsq_ws
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("n", C.SUMSQ_SIZES)
def test_sumsq(be, n, aligned):
    """*sumsq_dev = its seeded start value + sum(g^2) at 1e-6 of an fp64 sum: the accumulate contract FlatAdamW.step relies on by zeroing first;
    the largest n runs the 4-deep unrolled loop, a full and a partial single-float4 trip and the scalar tail, the view one float in the
    scalar branch.  The kernel ends in one fp32 atomic per workgroup; at the large n the 256 roundings onto a total of 1.6e7 (ulp 1) are a
    random walk of about 4 ulp = 2.5e-7 whose realisation depends on the arrival order (profiles/step_tail_margins.md, section 3)"""
    C.run_sumsq(be, n, aligned)


@pytest.mark.parametrize("nws", C.SUMSQ_WS)
def test_sumsq_ws(be, nws):
    """the fixed-order variant at the large n into a NaN workspace that must come back finite everywhere: 1e-6 of an fp64 sum with 1 (a
    thread adds 41 000 squares), 1024 and 65 536 partials, *sumsq_dev overwritten, two calls bit-identical"""
    C.run_sumsq_ws(be, nws)


def test_sumsq_rejects(be):
    C.run_sumsq_rejects(be)


# ------------------------------------------------------------------------------------------------------------------ 4. vptr_adamw
@pytest.mark.parametrize("case", sorted(C.ADAMW_LAUNCH))
def test_adamw_launch_classes(be, case):
    """p, m and v separately against fp64 after one call from a supplied state: the second grid-stride trip with a scalar tail (compared on its
    own as well), p / g / m / v in turn one float past a 16-byte boundary (the all-scalar path), n = 1, 3, 4, 1027"""
    C.run_adamw_launch(be, case)


def test_adamw_float4_and_scalar_paths_agree_bit_for_bit(be):
    """the same 4 195 507 values through the float4 loop and, with p one float in, through the scalar loop: torch.equal, as the comment in
    adamw_kernel promises (every sum of the update is an explicit fmaf, so the compiler has no choice of what to fuse in either loop)"""
    C.run_adamw_paths_equal(be)


@pytest.mark.parametrize("wd", C.ADAMW_WD)
@pytest.mark.parametrize("case", sorted(C.ADAMW_CLIP))
def test_adamw_clip(be, case, wd):
    """sumsq_dev NULL, the clip active (norm 10 x max_norm) and inactive, grad_scale 0.25 with both (inactive only because the scale applies
    before the comparison), weight decay 0 and 0.01; the reference is pinned to clip_grad_norm_ + torch.optim.AdamW in tests/test_cpu.py"""
    C.run_adamw_clip(be, case, wd)


def test_adamw_zero_gradient(be):
    C.run_adamw_zero_grad(be)


@pytest.mark.parametrize("betas", C.ADAMW_BETAS, ids=_id)
@pytest.mark.parametrize("k", C.ADAMW_STEPS)
def test_adamw_update_precision(be, k, betas):
    """p0 = 0, so the stored p is the update itself: update, m and v at five times the distance an fp32 evaluation with cancellation-free bias
    corrections keeps to fp64 (about 1e-7, so bars of 3e-7 ... 7e-7); the distance to fp64 with the double hyper-parameters is printed.  A
    bias correction computed as 1 - powf(b, step) misses these bars at steps 2, 3 and 5 of betas (0.9, 0.999): the subtraction cancels"""
    C.run_adamw_precision(be, k, betas)


# --------------------------------------------------------------------------------- 5. vptr_dropout / vptr_droppath_scales bit for bit
@pytest.mark.parametrize("n", C.DROP_SIZES)
def test_dropout_matches_the_integer_emulation(be, n):
    """torch.equal with helpers.drop_scale_emu for p = 0.1, 0.5, 0.999 x seeds that differ in the low word, the high word and both x sites 0, 1
    and 2^32 - 1: a hash that ignored a seed word or the site, or dropped index bits, fails here"""
    C.run_dropout(be, n)


@pytest.mark.parametrize("maxcount", C.DROPPATH_COUNTS)
def test_droppath_scales_match_the_integer_emulation(be, maxcount):
    C.run_droppath(be, maxcount)
