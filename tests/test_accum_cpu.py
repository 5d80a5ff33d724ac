"""CPU side of gradient accumulation and EMA weights in the device-resident optimizer controls: the ABI table of
include/vptr_hip_accum.h, the host-side rejects of its four entry points, the host rules of `optim.OptimControls` that need no device, and
every case of tests/accum_cases.py against the fp32 CPU emulation of the entry points -- and against eight named mutations of it, each of
which must fail the cases listed for it."""
import ctypes
import inspect
import os
import re

import pytest

import accum_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vptr_accum_begin", "vptr_optim_prepare_accum", "vptr_adamw_ctl_ema", "vptr_slab_swap"}


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_accum_signatures_match_header_and_library():
    from vptr_amd import _lib, optim
    text = open(os.path.join(ROOT, "include", "vptr_hip_accum.h")).read()
    assert '#include "vptr_hip_optim.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(re.findall(r"\b(vptr_\w+)\s*\(", text)) == set(decls) == set(_lib.ACCUM_SIGNATURES) == NAMES
    for name, args in decls.items():
        assert len(args.split(",")) == len(_lib.ACCUM_SIGNATURES[name]), name             # the stream included
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == _lib.ACCUM_SIGNATURES[name] and fn.restype is _lib.c_int
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES)]
    assert all(not NAMES & o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    assert set(_lib.OPTIM_SIGNATURES) == {"vptr_optim_prepare", "vptr_adamw_ctl"}
    from vptr_amd.build import SOURCES
    assert "optim.hip" in SOURCES
    # the record layout: header, host layer and the cases agree
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_ACC_(\w+) (\d+)", text)}
    assert {k: defs["W_" + k] for k in A.W} == A.W and defs["W_WORDS"] == optim.WORDS == A.WORDS == 16 and defs["SKIP_HOLD"] == optim.SKIP_HOLD == 2
    for k, i in A.W.items():
        assert getattr(optim, "W_" + k) == i
    assert all(i < 8 for k, i in A.W.items() if k in ("ACCUM_STEPS", "EMA_DECAY", "EMA_WARMUP")) and all(i >= 8 for k, i in A.W.items() if k not in ("ACCUM_STEPS", "EMA_DECAY", "EMA_WARMUP"))


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 160)()
    base = (ctypes.addressof(buf) + 63) & ~63
    hyper, state, window, step, sumsq, slab, slab2 = base, base + 64, base + 128, base + 192, base + 196, base + 256, base + 384

    def bad(fn, prefix, *args):
        assert fn(*args, None) != 0, (prefix, args)
        assert L.vptr_last_error().decode().startswith(prefix), L.vptr_last_error()

    for args in ((None, 4, window), (slab, 4, None), (slab, 0, window), (slab, -7, window), (slab, 4, window + 4), (slab, 4, window + 32)):
        bad(L.vptr_accum_begin, "accum_begin", *args)
    good = (hyper, state, window, step, sumsq)
    for i in range(5):
        bad(L.vptr_optim_prepare_accum, "optim_prepare_accum", *[None if j == i else a for j, a in enumerate(good)])
    for i in range(3):
        bad(L.vptr_optim_prepare_accum, "optim_prepare_accum", *[a + 16 if j == i else a for j, a in enumerate(good)])
    good = (slab, slab, slab, slab, slab2, 4, state, window)
    for i in (0, 1, 2, 3, 4, 6, 7):
        bad(L.vptr_adamw_ctl_ema, "adamw_ctl_ema", *[None if j == i else a for j, a in enumerate(good)])
    for n in (0, -5):
        bad(L.vptr_adamw_ctl_ema, "adamw_ctl_ema", *(good[:5] + (n,) + good[6:]))
    for i in (6, 7):
        bad(L.vptr_adamw_ctl_ema, "adamw_ctl_ema", *[a + 4 if j == i else a for j, a in enumerate(good)])
    for args in ((None, slab2, 4), (slab, None, 4), (slab, slab2, 0), (slab, slab2, -1), (slab, slab, 4), (slab, slab + 12, 4), (slab + 4, slab, 4), (slab, slab2, 40)):
        bad(L.vptr_slab_swap, "slab_swap", *args)
    assert all(x == 0.0 for x in buf)


# ---- host rules that need no device -----------------------------------------------------------------------------------------------------
class _Word:
    def fill_(self, value):
        pass


class _FakeRecord:
    """stands in for the device record: the host layer only ever slices one word and fills it"""

    def __getitem__(self, idx):
        return _Word()

    def data_ptr(self):
        return 0

    def numel(self):
        return 16


def _host_controls(k=2):
    from vptr_amd import optim
    c = optim.OptimControls.__new__(optim.OptimControls)
    c.window, c.micro_host = _FakeRecord(), 0
    c._wput = optim.Record(c.window).put
    c.accum_steps, c.ema_decay, c.ema_warmup = 1, None, True
    c.set_accum_steps(k)
    return c


def test_window_value_validation():
    c = _host_controls()
    for bad in (0, -1, 1 << 24, 2.0, True, "3", None):
        with pytest.raises(ValueError):
            c.set_accum_steps(bad)
    c.set_accum_steps((1 << 24) - 1)
    assert c.accum_steps == (1 << 24) - 1
    for bad in (1.0, -0.1, float("nan"), float("inf"), "0.9", True, 1.0 - 1e-9):        # the last one rounds to 1 in fp32
        with pytest.raises(ValueError):
            c.set_ema_decay(bad)
    for bad in (1, 0, "yes"):
        with pytest.raises(ValueError):
            c.set_ema_decay(0.9, bad)
    c.set_ema_decay(0.9, False)
    assert c.ema_decay == A.f32(0.9) and c.ema_warmup is False
    c.set_ema_decay(0.0)
    assert c.ema_decay == 0.0 and c.ema_warmup is False


def test_set_accum_steps_raises_inside_a_window():
    c = _host_controls(3)
    assert not c.closes_next()
    assert c.advance_mirror() is False and c.micro_host == 1
    with pytest.raises(RuntimeError, match="inside a window"):
        c.set_accum_steps(2)
    assert c.accum_steps == 3
    c.reset_window()
    c.set_accum_steps(2)
    assert [c.advance_mirror() for _ in range(5)] == [False, True, False, True, False] and c.closes_next()
    c2 = _host_controls(1)
    assert c2.closes_next() and [c2.advance_mirror() for _ in range(3)] == [True] * 3 and c2.micro_host == 0


def test_controls_without_a_window_refuse_the_window_calls():
    from vptr_amd import optim
    c = optim.OptimControls.__new__(optim.OptimControls)
    assert c.window is None
    for call in (lambda: c.set_accum_steps(2), lambda: c.set_ema_decay(0.9), c.reset_window, lambda: c.wword(8)):
        with pytest.raises(RuntimeError, match="accumulation window"):
            call()


def test_public_arguments_and_state_dict_keys():
    """the arguments exist with defaults that switch nothing on.  The state_dict keys need an optimizer on a device: they are asserted
    on a real dict in tests/test_18_accum_ema_gpu.py::test_state_dict_round_trip"""
    from vptr_amd import train
    for cls in (train.FlatAdamW, train.NARTrainer, train.FARTrainer):
        par = inspect.signature(cls.__init__).parameters
        assert par["accum_steps"].default is None and par["ema_decay"].default is None and par["ema_warmup"].default is True, cls


def test_repeated_destinations_split_only_on_an_accumulating_slab(monkeypatch):
    """ops.wgrad._split_repeats: nothing changes unless the deterministic mode is on AND a destination lies in a slab marked as
    accumulating; then the later records of a destination come out as rounds of their own, in recording order"""
    from vptr_amd.ops import wgrad
    items = [("a", 1000), ("b", 2000), ("c", 1000), ("d", 5000), ("e", 1000), ("f", 5000)]
    key = lambda it: (it[1],)
    monkeypatch.setattr(wgrad.config, "deterministic", True)
    monkeypatch.setattr(wgrad, "_accumulating_ranges", lambda: [])
    assert wgrad._split_repeats(items, key) == ([], items)
    monkeypatch.setattr(wgrad, "_accumulating_ranges", lambda: [(900, 2100)])
    later, first = wgrad._split_repeats(items, key)
    assert later == [[("c", 1000)], [("e", 1000)]] and first == [("a", 1000), ("b", 2000), ("d", 5000), ("f", 5000)]
    monkeypatch.setattr(wgrad.config, "deterministic", False)
    assert wgrad._split_repeats(items, key) == ([], items)


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return A.AccumEmu()


@pytest.mark.parametrize("case", A.all_cases(), ids=A.case_id)
def test_case_passes_on_the_emulation(be, case):
    getattr(A, case[0])(be, *case[1])


def test_mutation_lists_name_real_cases():
    known = set(A.all_cases())
    assert len(A.MUTATIONS) == 8
    for name, cases in A.MUTATIONS.items():
        assert cases and set(cases) <= known, name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(A.MUTATIONS) for c in A.MUTATIONS[m]], ids=lambda x: x if isinstance(x, str) else A.case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        getattr(A, case[0])(A.AccumEmu(mutation), *case[1])
