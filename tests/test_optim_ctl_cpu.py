"""CPU side of the device-resident optimizer controls: `LRSchedule` against torch's schedulers, its argument validation, the ABI table of
include/vptr_hip_optim.h, the host-side rejects of the two entry points, and every case of tests/optim_ctl_cases.py against the fp32 CPU
emulation of the entry points -- and against four named mutations of it, each of which must fail the cases listed for it (a case that a
wrong kernel could pass shows here, without a GPU)."""
import ctypes
import math
import os
import re

import pytest
import torch

import optim_ctl_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- LRSchedule ---------------------------------------------------------------------------------------------------------------------
def test_cosine_factor_matches_cosine_annealing_closed_form():
    """W = 0: base * factor(k) is CosineAnnealingLR's closed form eta_min + (base - eta_min) (1 + cos(pi k / T_max)) / 2 with eta_min = r * base"""
    from vptr_amd.optim import LRSchedule
    base, T, r = 3e-4, 25, 0.125                      # r is exact in fp32
    s = LRSchedule("cosine", warmup_steps=0, total_steps=T, min_ratio=r)
    p = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=base)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T, eta_min=r * base)
    for k in range(T + 1):
        closed = r * base + (base - r * base) * (1.0 + math.cos(math.pi * k / T)) / 2.0
        assert abs(base * s.factor(k) - closed) <= 1e-15 * base, k
        assert abs(opt.param_groups[0]["lr"] - closed) <= 1e-12 * base, k        # torch's recursive form drifts by a few fp64 ulp
        opt.step()
        sch.step()
    assert s.factor(T + 7) == r


@pytest.mark.parametrize("kind", C.KINDS)
def test_factor_is_what_lambda_lr_applies(kind):
    """LambdaLR(opt, schedule.factor) on fp64 parameters: the rate of the update after k applied updates is base * factor(k)"""
    from vptr_amd.optim import LRSchedule
    s = LRSchedule(kind, warmup_steps=3, total_steps=12, min_ratio=0.25)
    p = torch.nn.Parameter(torch.ones(4, dtype=torch.float64))
    opt = torch.optim.SGD([p], lr=0.5)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, s.factor)
    x = 1.0
    for k in range(16):
        assert opt.param_groups[0]["lr"] == 0.5 * s.factor(k)
        p.grad = torch.ones_like(p)
        opt.step()
        sch.step()
        x -= 0.5 * s.factor(k)
    assert abs(float(p[0]) - x) < 1e-12
    assert [s.factor(k) for k in range(3)] == [1 / 3, 2 / 3, 1.0] and s.factor(3) == 1.0
    assert s.factor(12) == (1.0 if kind == "constant" else 0.25) and s.factor(400) == s.factor(12)
    if kind == "linear":
        assert abs(s.factor(3 + 3) - (1.0 - 0.75 * 3 / 9)) < 1e-15


def test_schedule_validation():
    from vptr_amd.optim import LRSchedule
    for bad in (dict(kind="exp"), dict(kind="cosine"), dict(kind="linear", total_steps=None), dict(warmup_steps=-1), dict(warmup_steps=1.5),
                dict(warmup_steps=True), dict(kind="linear", warmup_steps=5, total_steps=4), dict(kind="cosine", total_steps=1 << 24),
                dict(min_ratio=-0.1), dict(min_ratio=1.5), dict(min_ratio=float("nan")), dict(min_ratio="x"), dict(total_steps=-3)):
        with pytest.raises(ValueError):
            LRSchedule(**bad)
    s = LRSchedule("cosine", 2, 9, 0.1)
    for k in (-1, 1.0, True):
        with pytest.raises(ValueError):
            s.factor(k)
    assert s.min_ratio == float(torch.tensor(0.1, dtype=torch.float32))       # held as the fp32 word the device reads
    assert LRSchedule.from_dict(s.to_dict()) == s and LRSchedule().factor(10 ** 6) == 1.0
    assert LRSchedule("constant", warmup_steps=4).total_steps == 4


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_optim_signatures_match_header_and_library():
    from vptr_amd import _lib, optim
    text = open(os.path.join(ROOT, "include", "vptr_hip_optim.h")).read()
    assert '#include "vptr_hip.h"' in text
    declared = set(re.findall(r"\b(vptr_\w+)\s*\(", text))
    assert declared == set(_lib.OPTIM_SIGNATURES) == {"vptr_optim_prepare", "vptr_adamw_ctl"}
    assert not set(_lib.OPTIM_SIGNATURES) & set(_lib.EXPORTS) and not set(_lib.OPTIM_SIGNATURES) & set(_lib.EXT_SIGNATURES)
    for name, argt in _lib.OPTIM_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == argt and fn.restype is _lib.c_int
    assert _lib.lib.vptr_abi_version() == 10
    from vptr_amd.build import SOURCES
    assert "optim.hip" in SOURCES
    # the record layout: header, host layer and the cases agree
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_OPT_(\w+) (\d+)", text)}
    assert {k: defs["H_" + k] for k in C.H} == C.H and {k: defs["S_" + k] for k in C.S} == C.S
    assert defs["H_WORDS"] == defs["S_WORDS"] == optim.WORDS == C.WORDS == 16
    for k, i in C.H.items():
        assert getattr(optim, "H_" + k) == i
    for k, i in C.S.items():
        assert getattr(optim, "S_" + k) == i


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device"""
    from vptr_amd import _lib
    buf = (ctypes.c_float * 96)()
    base = (ctypes.addressof(buf) + 63) & ~63
    hyper, state, step, sumsq, slab = base, base + 64, base + 128, base + 132, base + 192
    prep = _lib.lib.vptr_optim_prepare
    for args in ((None, state, step, sumsq), (hyper, None, step, sumsq), (hyper, state, None, sumsq), (hyper, state, step, None),
                 (hyper + 4, state, step, sumsq), (hyper, state + 32, step, sumsq)):
        assert prep(*args, None) != 0, args
        assert _lib.lib.vptr_last_error().decode().startswith("optim_prepare")
    ctl = _lib.lib.vptr_adamw_ctl
    for args in ((None, slab, slab, slab, 4, state), (slab, None, slab, slab, 4, state), (slab, slab, None, slab, 4, state), (slab, slab, slab, None, 4, state),
                 (slab, slab, slab, slab, 4, None), (slab, slab, slab, slab, 0, state), (slab, slab, slab, slab, -5, state), (slab, slab, slab, slab, 4, state + 16)):
        assert ctl(*args, None) != 0, args
        assert _lib.lib.vptr_last_error().decode().startswith("adamw_ctl")
    assert all(x == 0.0 for x in buf)


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return C.OptimEmu()


def _all_cases():
    out = [("run_prepare_schedule", (k,)) for k in C.KINDS] + [("run_prepare_schedule_edges", (e,)) for e in sorted(C.SCHED_EDGES)]
    out += [("run_prepare_scalars", (k, b)) for k in C.ADAMW_STEPS for b in C.ADAMW_BETAS]
    out += [("run_prepare_clip", (c,)) for c in sorted(C.CLIP)]
    out += [("run_prepare_nonfinite", (w, s)) for w in sorted(C.NONFINITE) for s in (0, 1)] + [("run_prepare_sequence", ())]
    out += [("run_ctl_same_bits_launch", (c,)) for c in sorted(C.CTL_LAUNCH)]
    out += [("run_ctl_same_bits_clip", (c, wd)) for c in sorted(C.CTL_CLIP) for wd in C.CTL_WD]
    out += [("run_ctl_same_bits_stage1", ()), ("run_ctl_cosine_same_bits", ()), ("run_ctl_trajectory", ())] + [("run_ctl_skip", (c,)) for c in sorted(C.CTL_SKIP_N)] + [("run_rejects", ())]
    return out


def _case_id(c):
    return c[0][4:] + "".join("-%s" % (("%g_%g" % a) if isinstance(a, tuple) else a) for a in c[1])


@pytest.mark.parametrize("case", _all_cases(), ids=_case_id)
def test_case_passes_on_the_emulation(be, case):
    getattr(C, case[0])(be, *case[1])


def test_mutation_lists_name_real_cases():
    known = set(_all_cases())
    assert len(C.MUTATIONS) >= 4
    for name, cases in C.MUTATIONS.items():
        assert cases and set(cases) <= known, name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(C.MUTATIONS) for c in C.MUTATIONS[m]], ids=lambda x: x if isinstance(x, str) else _case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        getattr(C, case[0])(C.OptimEmu(mutation), *case[1])
