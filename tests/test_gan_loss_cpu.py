"""CPU side of the fused adversarial losses: the ABI table of include/vptr_hip_gan.h, the host-side rejects of its two entry points, the
inputs' planted values, the fp64 reference builder against the reference's own GANLoss, the `gan_loss=` argument of the trainers, and
every case of tests/gan_loss_cases.py against the fp32 CPU emulation of the entry points -- inside every bar -- and against eight named
mutations of it, each of which must fail the cases listed for it."""
import ctypes
import importlib
import inspect
import os
import re
import sys

import pytest
import torch

import gan_loss_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vptr_gan_loss_fwd", "vptr_gan_loss_bwd"}


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_gan_signatures_match_header_and_library():
    from vptr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vptr_hip_gan.h")).read()
    assert '#include "vptr_hip.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(decls) == set(_lib.GAN_SIGNATURES) == NAMES
    P, I, F, L = _lib.c_void_p, _lib.c_int, _lib.c_float, _lib.c_int64
    kind = {"float": F, "long": L, "int": I}
    for name, args in decls.items():
        kinds = [P if ("*" in a or "vptr_stream_t" in a) else kind[a.split()[0]] for a in args.split(",")]
        assert kinds == _lib.GAN_SIGNATURES[name], name                                   # the stream included
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == _lib.GAN_SIGNATURES[name] and fn.restype is _lib.c_int
    assert ctypes.sizeof(ctypes.c_long) == 8                                               # the header's `long` is what c_int64 passes
    assert "ceil(na / 2048) + ceil(nb / 2048) floats" in text and G.CHUNK == 2048          # the scratch size the cases allocate
    from vptr_amd.build import SOURCES
    assert "gan_loss.hip" in SOURCES
    from vptr_amd import ops
    assert ops.GAN_MODES == G.MODES and ops.losses.GAN_CHUNK == G.CHUNK


def test_other_tables_are_unchanged():
    from vptr_amd import _lib
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES), set(_lib.ACCUM_SIGNATURES),
              set(_lib.LOSS_SIGNATURES)]
    assert all(not NAMES & o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    assert set(_lib.LOSS_SIGNATURES) == {"vptr_recon_loss_fwd", "vptr_recon_loss_bwd"}


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    base = dict(xa=a, na=16, stride_a=1, a_is_real=0, xb=a, nb=16, stride_b=2, b_is_real=1, mode=0, real_label=1.0, fake_label=0.0, coef=0.5,
                scratch=a, out3=a, dxa=a, dxb=a, g_a=a, g_b=a, g_total=a)
    for which, order, extra in (("fwd", G.FWD_ARGS, G.REJECTS_FWD), ("bwd", G.BWD_ARGS, G.REJECTS_BWD)):
        for change in G.REJECTS + extra:
            vals = dict(base, **change)
            assert getattr(L, "vptr_gan_loss_" + which)(*(vals[k] for k in order), None) != 0, (which, change)
            assert L.vptr_last_error().decode().startswith("gan_loss_" + which), L.vptr_last_error()
    assert all(x == 0.0 for x in buf)


# ---- the inputs and the reference ---------------------------------------------------------------------------------------------------
def test_cases_reach_their_hazards():
    sizes = {n for g in G.GEOMS.values() for n in g[:2] if n is not None}
    assert {1, 3, G.CHUNK - 1, G.CHUNK, G.CHUNK + 1, 2880, 70001} <= sizes
    assert 70001 > 16 * 20 * 14 * 14                                                       # above KTH128's logits
    assert any(g[1] is None for g in G.GEOMS.values()) and any(g[1] not in (None, g[0]) for g in G.GEOMS.values())
    assert any(g[2] == 4 for g in G.GEOMS.values()) and any(g[3] == 4 for g in G.GEOMS.values())
    assert {(g[4], g[5]) for g in G.GEOMS.values() if g[1] is not None} >= {(0, 1), (1, 0), (1, 1)}
    assert {s[0] for s in G.SETTINGS.values()} == {0.5, 3.0, 20.0}
    assert {s[1] for s in G.SETTINGS.values()} == {(1.0, 0.0), (0.9, 0.1)} and {s[2] for s in G.SETTINGS.values()} == {0.005, 1.0}
    assert len(G.UPSTREAM) == 5 and all(set(u) <= {None, 1.0, 1.3} for u in G.UPSTREAM.values())
    x = G.logits(2880, 9100, 3.0)
    assert x.dtype == torch.float32 and x[:8].tolist() == G.PLANTED and bool(torch.signbit(x[1]))
    assert G.logits(1, 9100, 3.0).tolist() == [-104.0] and G.logits(3, 9100, 3.0).tolist() == [-90.0, 104.0, -104.0]
    # what the planted values do to the naive forms in fp32
    big = torch.tensor([104.0, 90.0])
    assert bool(torch.isinf(torch.log(1.0 + torch.exp(big))).all()) and bool(torch.isnan(torch.exp(big) / (1.0 + torch.exp(big))).all())
    buf = G.strided(x, 4, "cpu")
    assert buf.numel() == 4 * 2880 and torch.equal(buf[::4], x) and bool(torch.isnan(buf.view(-1, 4)[:, 1:]).all())
    assert G.scratch_floats(2047, 2049) == 3 and G.scratch_floats(2048, None) == 1 and G.scratch_floats(70001, 2880) == 37


@pytest.fixture(scope="module")
def ref_criterion():
    from oracle.ref_import import REFERENCE_ROOT, import_reference
    if not os.path.isdir(REFERENCE_ROOT):
        pytest.skip("the reference checkout is not present")
    before = set(sys.modules)
    import_reference()
    saved = list(sys.path)
    sys.path.insert(0, REFERENCE_ROOT)
    try:
        crit = importlib.import_module("model.criterion")
    finally:
        sys.path[:] = saved
    assert crit.__file__.startswith(REFERENCE_ROOT)
    yield crit
    for k in set(sys.modules) - before:
        if k.split(".")[0] in ("utils", "model"):
            del sys.modules[k]


@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_reference_builder_is_the_reference(ref_criterion, mode):
    """the fp64 builder with this project's GANLoss against the same builder with the reference's own class"""
    for geom in ("n3", "n2047_2049", "n2880_2160_s4_1"):
        for setting in G.SETTINGS:
            _, _, _, _, ar, br = G.GEOMS[geom]
            _, labels, coef = G.SETTINGS[setting]
            xa, xb = G.inputs(geom, setting)
            ours = G.criterion_eval(mode, xa, ar, xb, br, labels, coef, G.UPSTREAM["all"])
            theirs = G.criterion_eval(mode, xa, ar, xb, br, labels, coef, G.UPSTREAM["all"], crit=ref_criterion)
            for a, b in zip(ours["out"], theirs["out"]):
                assert abs(a - b) <= 1e-14 * abs(b), (mode, geom, setting)
            for k in ("dxa", "dxb"):
                if theirs[k] is not None:
                    assert float((ours[k] - theirs[k]).abs().max()) <= 1e-14 * float(theirs[k].abs().max()), (mode, geom, setting, k)


# ---- the trainers' argument ---------------------------------------------------------------------------------------------------------
def test_trainers_take_gan_loss_and_the_ops_exist():
    from vptr_amd import ops, train
    for cls in (train.NARTrainer, train.FARTrainer, train.AETrainer):
        assert inspect.signature(cls.__init__).parameters["gan_loss"].default == "torch", cls
    par = inspect.signature(ops.gan_loss).parameters
    assert list(par) == ["logits", "target_is_real", "mode", "real_label", "fake_label"]
    assert (par["mode"].default, par["real_label"].default, par["fake_label"].default) == ("vanilla", 1.0, 0.0)
    par = inspect.signature(ops.gan_loss_pair).parameters
    assert list(par) == ["fake_logits", "real_logits", "coef", "mode", "real_label", "fake_label"]
    x = torch.zeros(4)
    with pytest.raises(RuntimeError):
        ops.gan_loss(x, True)                                   # CPU tensors are refused, as everywhere
    with pytest.raises(RuntimeError):
        ops.gan_loss_pair(x, x, 0.5)


def test_gan_loss_argument_errors():
    """an unknown setting, and a mode the kernels do not have, raise before anything is built on a device"""
    from vptr_amd.train import _GanMixin
    m = _GanMixin()
    assert m.gan_fused is False
    for bad in ("hip", "", None, True):
        with pytest.raises(ValueError, match="gan_loss"):
            m._init_gan_loss(bad, "vanilla")
    with pytest.raises(ValueError, match="gan_mode"):
        m._init_gan_loss("fused", "hinge")
    for mode in G.MODES:
        m._init_gan_loss("fused", mode)
        assert m.gan_fused and m.gan_mode == mode and m.gan_loss == "fused"
    m._init_gan_loss("torch", "vanilla")
    assert not m.gan_fused
    from vptr_amd import ops
    with pytest.raises(ValueError):
        ops.losses._gan_cfg("gan_loss", "hinge", 1.0, 0.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.losses._gan_cfg("gan_loss", "vanilla", bad, 0.0)
        with pytest.raises(ValueError):
            ops.losses._gan_cfg("gan_loss_pair", "vanilla", 1.0, 0.0, bad)


def test_element_stride_of_views():
    from vptr_amd.ops.losses import _elem_stride
    y = torch.zeros(6, 4)
    assert _elem_stride(y) == 1 and _elem_stride(y[:, :1]) == 4 and _elem_stride(y[:, :1].reshape(2, 1, 3, 1)) == 4
    assert _elem_stride(y[:, :2]) is None and _elem_stride(y.t()) is None and _elem_stride(y[::2, 0]) == 8
    assert _elem_stride(torch.zeros(())) == 1 and _elem_stride(torch.zeros(1, 1)) == 1
    assert _elem_stride(torch.zeros(3).expand(2, 3)) is None and _elem_stride(torch.zeros(1).expand(3)) is None


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return G.GanEmu()


@pytest.mark.parametrize("case", G.all_cases(), ids=G.case_id)
def test_case_passes_on_the_emulation(be, case):
    G.run_case(be, *case)


def test_rejects_on_the_emulation(be):
    G.run_rejects(be)


def test_two_calls_are_bit_identical_on_the_emulation(be):
    G.run_twice_identical(be, "vanilla", "n70001", "s3_soft")


def test_mutation_lists_name_real_cases():
    known = set(G.all_cases())
    assert len(G.MUTATIONS) == 8
    for name, cases in G.MUTATIONS.items():
        assert cases and set(cases) <= known and len(set(cases)) == len(cases), name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(G.MUTATIONS) for c in G.MUTATIONS[m]],
                         ids=lambda x: x if isinstance(x, str) else G.case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        G.run_case(G.GanEmu(mutation), *case)
