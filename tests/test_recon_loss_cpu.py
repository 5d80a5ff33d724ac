"""CPU side of the reconstruction losses with temporal weights, L1 and a GDL exponent: the ABI table of include/vptr_hip_loss.h, the
host-side rejects of its two entry points, the inputs' tie properties, the fp64 reference builder against the reference's own criterion
classes, `ReconLoss` and its `from_criteria`, and every case of tests/recon_loss_cases.py against the fp32 CPU emulation of the entry
points -- and against seven named mutations of it, each of which must fail the cases listed for it."""
import ctypes
import importlib
import inspect
import os
import re
import sys

import pytest
import torch

import recon_loss_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vptr_recon_loss_fwd", "vptr_recon_loss_bwd"}


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_loss_signatures_match_header_and_library():
    from vptr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vptr_hip_loss.h")).read()
    assert '#include "vptr_hip.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(decls) == set(_lib.LOSS_SIGNATURES) == NAMES
    P, I, F = _lib.c_void_p, _lib.c_int, _lib.c_float
    for name, args in decls.items():
        kinds = [P if ("*" in a or "vptr_stream_t" in a) else (F if a.split()[0] == "float" else I) for a in args.split(",")]
        assert kinds == _lib.LOSS_SIGNATURES[name], name                                  # the stream included
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == _lib.LOSS_SIGNATURES[name] and fn.restype is _lib.c_int
    assert "planes * ceil(H / 16) * 4 floats" in text                                      # the scratch size the cases allocate
    from vptr_amd.build import SOURCES
    assert "recon_loss.hip" in SOURCES and "losses.hip" in SOURCES


def test_other_tables_are_unchanged():
    from vptr_amd import _lib
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES), set(_lib.ACCUM_SIGNATURES)]
    assert all(not NAMES & o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    assert set(_lib.EXT_SIGNATURES) == {"vptr_meters_add"}
    assert set(_lib.OPTIM_SIGNATURES) == {"vptr_optim_prepare", "vptr_adamw_ctl"}
    assert set(_lib.CONVFFN_SIGNATURES) == {"vptr_norm_act_bwd_sums", "vptr_dwconv3x3_norm_bwd"}
    assert set(_lib.ACCUM_SIGNATURES) == {"vptr_accum_begin", "vptr_optim_prepare_accum", "vptr_adamw_ctl_ema", "vptr_slab_swap"}
    assert _lib.SIGNATURES["vptr_mse_gdl_fwd"] == [_lib.c_void_p] * 5 + [_lib.c_int] * 3 + [_lib.c_void_p]
    assert _lib.SIGNATURES["vptr_mse_gdl_bwd"] == [_lib.c_void_p] * 5 + [_lib.c_int] * 3 + [_lib.c_void_p]


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    for planes, ppf, T, H, W, alpha in R.REJECTS:
        assert L.vptr_recon_loss_fwd(a, a, a, a, a, a, planes, ppf, T, H, W, alpha, None) != 0, (planes, ppf, T, H, W, alpha)
        assert L.vptr_last_error().decode().startswith("recon_loss_fwd"), L.vptr_last_error()
        assert L.vptr_recon_loss_bwd(a, a, a, a, a, a, a, a, planes, ppf, T, H, W, alpha, None) != 0, (planes, ppf, T, H, W, alpha)
        assert L.vptr_last_error().decode().startswith("recon_loss_bwd"), L.vptr_last_error()
    for i in (0, 1, 4, 5):
        args = [a] * 6
        args[i] = None
        assert L.vptr_recon_loss_fwd(*args, 4, 1, 2, 4, 4, 1.0, None) != 0, i
    for i in (0, 1, 7):
        args = [a] * 8
        args[i] = None
        assert L.vptr_recon_loss_bwd(*args, 4, 1, 2, 4, 4, 1.0, None) != 0, i
    assert all(x == 0.0 for x in buf)


# ---- the inputs and the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", sorted(R.GEOMS))
def test_inputs_have_exact_ties_and_no_sign_disagreement(geom):
    """every element takes part in every comparison: no GDL sign argument and no sign(pred - gt) differs between fp32 and fp64, and the
    exact ties the cases are about do occur"""
    gdl_bad, l1_bad, ties = R.input_tie_counts(geom)
    assert gdl_bad == 0 and l1_bad == 0 and ties > 0, (geom, gdl_bad, l1_bad, ties)
    planes, ppf, T, H, W = R.geometry(geom)
    shape = R.GEOMS[geom][0]
    assert planes % (ppf * T) == 0 and planes * H * W == torch.Size(shape).numel()
    assert ppf == (shape[2] if len(shape) == 5 else shape[2] * shape[3])
    pred, _ = R.inputs(geom)
    assert bool((pred[..., -1, 0] == pred[..., -1, 1]).all())


def test_geometries_reach_their_hazards():
    g = {k: R.geometry(k) for k in R.GEOMS}
    assert g["2x3x3x17x5"][3] % 16 == 1 and g["2x5x1x33x4"][3] % 16 == 1                   # one-row last bands
    assert g["5x4x15x5x3"][0] * 1 > 256                                                    # a second trip of the final loop
    assert g["1x2x1x16x300"][3] == 16 and g["1x2x1x16x300"][4] > 256                       # exactly one band; rows wider than the workgroup
    assert g["1x1x1x2x2"] == (1, 1, 1, 2, 2) and g["2x3x2x1x4x4"][1] == 2
    for k in R.GEOMS:                                                                      # a weight of 0 and the exponential weights
        wp, wg = R.weights(k, "both")
        T = g[k][2]
        assert wp.dtype == wg.dtype == torch.float32 and wp.numel() == wg.numel() == T and not torch.equal(wp, wg)
        if T > 1:
            assert float(wg[0]) == 0.0 and torch.equal(wp, R.exp_weights(T))


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


@pytest.mark.parametrize("geom", ["2x3x3x17x5", "1x2x1x16x300", "2x3x2x1x4x4"])
def test_reference_builder_is_the_reference(ref_criterion, geom):
    """the fp64 builder with this project's criterion classes against the same builder with the reference's own classes"""
    pred, gt = R.inputs(geom)
    T = R.geometry(geom)[2]
    assert torch.equal(ref_criterion.temporal_weight_func(T).float(), R.exp_weights(T))
    for mode in R.WEIGHTS:
        for alpha in R.ALPHAS:
            wp, wg = R.weights(geom, mode)
            ours = R.criteria_eval(pred, gt, wp, wg, alpha, R.UPSTREAM["all"], torch.float64)
            theirs = R.criteria_eval(pred, gt, wp, wg, alpha, R.UPSTREAM["all"], torch.float64, crit=ref_criterion)
            for k in ("mse", "l1", "gdl"):
                assert abs(ours[k] - theirs[k]) <= 1e-14 * abs(theirs[k]), (geom, mode, alpha, k)
            assert float((ours["dpred"] - theirs["dpred"]).abs().max()) <= 1e-14 * float(theirs["dpred"].abs().max()), (geom, mode, alpha)


# ---- ReconLoss ------------------------------------------------------------------------------------------------------------------------
def test_recon_loss_configuration():
    from vptr_amd.model.criterion import GDL, L1Loss, MSELoss, temporal_weight_func
    from vptr_amd.train import ReconLoss
    d = ReconLoss()
    assert (d.point, d.gdl_alpha, d.temporal_weight, d.gdl_temporal_weight, d.has_weights) == ("mse", 1.0, None, None, False)
    e = ReconLoss("l1", 2, "exp")
    assert e.temporal_weight == "exp" and e.gdl_temporal_weight == "exp" and e.has_weights
    assert torch.equal(ReconLoss.resolve("exp", 7), temporal_weight_func(7).float())
    assert ReconLoss.resolve(None, 7) is None
    assert ReconLoss("mse", 1.0, [1.0, 2.0], None).gdl_temporal_weight is None
    w = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    r = ReconLoss("mse+l1", 1.5, w, [3.0, 2.0, 1.0])
    assert r.temporal_weight.dtype == torch.float32 and torch.equal(r.temporal_weight, w.float()) and r.gdl_temporal_weight.tolist() == [3.0, 2.0, 1.0]
    for bad in (dict(point="huber"), dict(gdl_alpha=0.5), dict(gdl_alpha=float("nan")), dict(gdl_alpha=float("inf")), dict(gdl_alpha="2"),
                dict(gdl_alpha=True), dict(temporal_weight="linear"), dict(temporal_weight=torch.ones(2, 2)), dict(temporal_weight=[1.0, float("nan")]),
                dict(gdl_temporal_weight=[])):
        with pytest.raises(ValueError):
            ReconLoss(**bad)
    with pytest.raises(ValueError):
        ReconLoss.resolve(w, 4)                                 # a wrong length
    with pytest.raises(ValueError):
        ReconLoss.resolve("exp", 1)
    a, b, c = torch.tensor(2.0), torch.tensor(3.0), None
    assert ReconLoss("mse").total(a, b) is a and ReconLoss("l1").total(a, b) is b and float(ReconLoss("mse+l1").total(a, b)) == 5.0 and c is None

    # from_criteria
    tw = temporal_weight_func(5)
    f = ReconLoss.from_criteria(MSELoss(temporal_weight=tw), GDL(alpha=2, temporal_weight=tw * 2))
    assert (f.point, f.gdl_alpha) == ("mse", 2.0) and torch.equal(f.temporal_weight, tw.float()) and torch.equal(f.gdl_temporal_weight, (tw * 2).float())
    f = ReconLoss.from_criteria(L1Loss(), GDL())
    assert (f.point, f.gdl_alpha, f.has_weights) == ("l1", 1.0, False)
    f = ReconLoss.from_criteria((MSELoss(temporal_weight=tw), L1Loss(temporal_weight=tw.clone())))
    assert (f.point, f.gdl_alpha) == ("mse+l1", 1.0) and f.gdl_temporal_weight is None
    for bad in (lambda: ReconLoss.from_criteria(MSELoss(norm_dim=2), GDL()), lambda: ReconLoss.from_criteria(L1Loss(norm_dim=1)),
                lambda: ReconLoss.from_criteria(GDL()), lambda: ReconLoss.from_criteria(MSELoss(), MSELoss()),
                lambda: ReconLoss.from_criteria((MSELoss(), MSELoss())), lambda: ReconLoss.from_criteria((MSELoss(temporal_weight=tw), L1Loss())),
                lambda: ReconLoss.from_criteria(MSELoss(), GDL(alpha=0.5))):
        with pytest.raises(ValueError):
            bad()


def test_trainers_take_recon_and_the_op_exists():
    from vptr_amd import ops, train
    for cls in (train.NARTrainer, train.FARTrainer, train.AETrainer):
        assert inspect.signature(cls.__init__).parameters["recon"].default is None, cls
        assert callable(getattr(cls, "set_temporal_weight"))
    par = inspect.signature(ops.recon_losses).parameters
    assert list(par) == ["pred", "gt", "w_point", "w_gdl", "gdl_alpha", "time_dim"]
    assert (par["w_point"].default, par["w_gdl"].default, par["gdl_alpha"].default, par["time_dim"].default) == (None, None, 1.0, 1)
    assert list(inspect.signature(ops.mse_gdl).parameters) == ["pred", "gt"]


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return R.ReconEmu()


@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_case_passes_on_the_emulation(be, case):
    R.run_case(be, *case)


def test_rejects_on_the_emulation(be):
    R.run_rejects(be)


def test_mutation_lists_name_real_cases():
    known = set(R.all_cases())
    assert len(R.MUTATIONS) == 7
    for name, cases in R.MUTATIONS.items():
        assert cases and set(cases) <= known, name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(R.MUTATIONS) for c in R.MUTATIONS[m]],
                         ids=lambda x: x if isinstance(x, str) else R.case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        R.run_case(R.ReconEmu(mutation), *case)
