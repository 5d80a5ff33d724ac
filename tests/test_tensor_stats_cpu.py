"""CPU side of the per-tensor statistics (include/vptr_hip_diag.h, vptr_amd/diagnostics.py): the ABI table, the host-side rejects of the
entry point, the properties of the plan, every case of tests/tensor_stats_cases.py against the CPU emulation of the call -- and against nine
named mutations of it, each of which must fail the cases listed for it --, the fp64 builder of the cases pinned to torch's own norms per
parameter of a small nn.Module, and every ValueError of the host layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tensor_stats_cases as T
from vptr_amd import diagnostics as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_diag_signatures_match_header_and_library():
    from vptr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vptr_hip_diag.h")).read()
    assert '#include "vptr_hip_optim.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(decls) == set(_lib.DIAG_SIGNATURES) == {"vptr_tensor_stats"}
    args = [a.strip() for a in decls["vptr_tensor_stats"].split(",")]
    sig = _lib.DIAG_SIGNATURES["vptr_tensor_stats"]
    assert len(args) == len(sig) == 15                                                   # the stream included
    for a, t in zip(args, sig):
        want = _lib.P if ("*" in a or "vptr_stream_t" in a) else (_lib.L if a.startswith("int64_t") else _lib.I)
        assert t is want, (a, t)
    fn = _lib.lib.vptr_tensor_stats
    assert fn.argtypes == sig and fn.restype is _lib.c_int
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES), set(_lib.ACCUM_SIGNATURES),
              set(_lib.LOSS_SIGNATURES), set(_lib.GAN_SIGNATURES), set(_lib.GROUP_SIGNATURES), set(_lib.DATA_SIGNATURES)]
    assert all("vptr_tensor_stats" not in o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    from vptr_amd.build import FLAGS, SOURCES
    assert "tensor_stats.hip" in SOURCES
    assert not any("fast-math" in f or "unsafe-math" in f or "correctly-rounded" in f for f in FLAGS)   # what the DIR_RMS bar rests on
    # the constants: header, host layer and cases agree
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_TS_(\w+) (\d+)", text)}
    assert defs["CHUNK"] == D.CHUNK == 4096 and defs["MAX_TENSORS"] == D.MAX_TENSORS == 65535
    assert defs["ROW_WORDS"] == D.ROW_WORDS == len(D.COLUMNS) == 8 and defs["CTL_WORDS"] == D.CTL_WORDS == 16
    assert [defs["R_" + c.upper()] for c in D.COLUMNS] == list(range(8))
    assert (defs["C_EVERY"], defs["C_ON_SKIP"], defs["C_PHASE"], defs["C_COMPUTED"], defs["C_AGE"]) == (D.C_EVERY, D.C_ON_SKIP, D.C_PHASE, D.C_COMPUTED, D.C_AGE)
    assert defs["AGE_MAX"] == D.AGE_MAX == 1 << 24 and defs["PART_BYTES"] == D.PART_BYTES == 40
    optim_h = open(os.path.join(ROOT, "include", "vptr_hip_optim.h")).read()
    words = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_OPT_S_(\w+) (\d+)", optim_h)}
    assert (words["SKIP_NOW"], words["INV_SQRT_BC2"], words["EPS"]) == (T.S_SKIP_NOW, T.S_INV_SQRT_BC2, T.S_EPS)


def test_entry_point_rejects_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 1024)()
    base = (ctypes.addressof(buf) + 63) & ~63
    slab, seg, items, scale, state, ctl, table, ws = base + 1024, base + 64, base + 128, base + 192, base + 256, base + 320, base + 384, base + 512
    good = [slab, slab, slab, slab, seg, items, 2, scale, state, ctl, table, ws, 80, 0]

    def bad(**kw):
        names = ["p", "g", "m", "v", "seg_off", "item_first", "S", "scale", "state", "ctl", "table", "ws", "ws_bytes", "grid_cap"]
        args = [kw.get(n, a) for n, a in zip(names, good)]
        assert L.vptr_tensor_stats(*args, None) != 0, kw
        assert L.vptr_last_error().decode().startswith("tensor_stats"), L.vptr_last_error()

    for name in ("p", "g", "seg_off", "item_first", "ctl", "table", "ws"):
        bad(**{name: None})
    for S in (0, -1, 65536):
        bad(S=S, ws_bytes=1 << 30)
    bad(ctl=ctl + 4)
    bad(ctl=ctl + 32)
    bad(table=table + 16)
    bad(ws=ws + 4)
    bad(ws_bytes=79)
    bad(ws_bytes=0)
    bad(ws_bytes=-40)
    for absent in (("m",), ("v",), ("state",), ("m", "v"), ("m", "state"), ("v", "state")):
        bad(**{n: None for n in absent})
    bad(state=state + 16)
    bad(grid_cap=-1)
    assert all(x == 0.0 for x in buf)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", sorted(T.GEOS))
def test_plan_covers_every_element_once_and_never_straddles(geo):
    sizes = T.GEOS[geo][0]
    seg_off, item_first = D.plan(sizes)
    so = seg_off.tolist()
    assert so[0] == 0 and [b - a for a, b in zip(so, so[1:])] == list(sizes)
    items = D.items_of(seg_off, item_first)
    assert len(items) == int(item_first[-1]) == sum(-(-n // D.CHUNK) for n in sizes)
    seen = np.zeros(so[-1], dtype=np.int64)
    for k, (i, a, b) in enumerate(items):
        assert so[i] <= a < b <= so[i + 1] and 1 <= b - a <= D.CHUNK, "item %d straddles a tensor or is empty" % k
        assert (a - so[i]) % D.CHUNK == 0 and int(item_first[i]) <= k < int(item_first[i + 1])
        seen[a:b] += 1
    assert bool((seen == 1).all())
    for i in range(len(sizes)):      # only a tensor's last chunk is short
        own = [(a, b) for j, a, b in items if j == i]
        assert all(b - a == D.CHUNK for a, b in own[:-1])


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return T.TsEmu()


@pytest.mark.parametrize("case", T.all_cases(), ids=T.case_id)
def test_case_passes_on_the_emulation(be, case):
    getattr(T, case[0])(be, *case[1])


def test_mutation_lists_name_real_cases():
    known = set(T.all_cases())
    assert len(T.MUTATIONS) == 9
    for name, cases in T.MUTATIONS.items():
        assert cases and set(cases) <= known, name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(T.MUTATIONS) for c in T.MUTATIONS[m]], ids=lambda x: x if isinstance(x, str) else T.case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        getattr(T, case[0])(T.TsEmu(mutation), *case[1])


def test_bars_are_the_derived_ones():
    assert T.NORM_RTOL == 2.0 ** -23 and 4 * 2.0 ** -24 + 2.0 ** -27 < T.DIR_RTOL <= 2.0 ** -22 + 2.0 ** -26 and T.DIR_ATOL == 2.0 ** -149


# ---- the fp64 builder is torch ----------------------------------------------------------------------------------------------------------
def test_fp64_builder_is_torch_per_parameter():
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(7, 13), torch.nn.LayerNorm(13), torch.nn.Conv2d(13, 5, 3), torch.nn.Linear(5, 1, bias=False)).double()
    params = list(net.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 0.3
    m = [torch.randn_like(p) * 0.1 for p in params]
    v = [torch.rand_like(p) * 0.01 for p in params]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    ref = T.ref_table(flat(params), flat([p.grad for p in params]), flat(m), flat(v), [p.numel() for p in params], 0.25, T.ISB, T.EPS, True)

    def close(a, b):
        return abs(a - b) <= 1e-12 * abs(b)
    for i, p in enumerate(params):
        assert close(float(ref[i, D.GRAD_NORM]), 0.25 * float(p.grad.norm())) and close(float(ref[i, D.WEIGHT_NORM]), float(p.detach().norm()))
        assert close(float(ref[i, D.GRAD_MAXABS]), 0.25 * float(p.grad.abs().max())) and close(float(ref[i, D.WEIGHT_MAXABS]), float(p.detach().abs().max()))
        d = m[i] / (v[i].sqrt() * T.ISB + T.EPS)
        assert close(float(ref[i, D.DIR_RMS]), float(d.pow(2).mean().sqrt())) and float(ref[i, D.NUMEL]) == p.numel()
    S = len(params)
    assert close(float(ref[S, D.GRAD_NORM]), 0.25 * float(torch.nn.utils.clip_grad_norm_(params, 1e30)))
    assert close(float(ref[S, D.WEIGHT_NORM]), float(flat(params).norm())) and float(ref[S, D.NUMEL]) == sum(p.numel() for p in params)
    assert float(ref[:, D.GRAD_NONFINITE:D.WEIGHT_NONFINITE + 1].abs().sum()) == 0.0


# ---- the host layer's ValueErrors ---------------------------------------------------------------------------------------------------------
def test_configuration_value_errors():
    for every in (0, -1, 1 << 24, 1.0, 2.5, True, None, "3"):
        with pytest.raises(ValueError, match="every"):
            D.TensorStats(every=every)
    assert D.TensorStats(every=(1 << 24) - 1).every == (1 << 24) - 1 and D.TensorStats(every=np.int64(3)).every == 3
    for flag in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="moments"):
            D.TensorStats(moments=flag)
    with pytest.raises(ValueError, match="on_skip"):
        D.TensorStats(on_skip=1)
    with pytest.raises(ValueError, match="on_skip=True needs moments=True"):
        D.TensorStats(moments=False, on_skip=True)
    c = D.TensorStats(moments=False)
    assert (c.every, c.moments, c.on_skip) == (1, False, False) and D.TensorStats().on_skip is True


def test_plan_and_name_value_errors():
    with pytest.raises(ValueError, match="0 tensors"):
        D.plan([])
    with pytest.raises(ValueError, match="65536 tensors"):
        D.plan([1] * 65536)
    assert len(D.plan([1] * 65535)[0]) == 65536
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="whole number >= 1"):
            D.plan([4, bad, 4])
    seg_off, item_first = D.plan([5, 4097])
    assert seg_off.tolist() == [0, 5, 4102] and item_first.tolist() == [0, 1, 3]
    for so, it in (([1, 5, 4102], [0, 1, 3]), ([0, 5, 5], [0, 1, 1]), ([0, 5, 4102], [0, 1, 2]), ([0, 5, 4102], [1, 2, 4])):
        with pytest.raises(ValueError):
            D.validate_plan(torch.tensor(so, dtype=torch.int64), torch.tensor(it, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        D.validate_plan(seg_off.int(), item_first)
    with pytest.raises(ValueError, match="2 names for 3"):
        D.check_names(["a", "b"], 3)
    with pytest.raises(ValueError, match="'a' appears twice"):
        D.check_names(["a", "b", "a"], 3)
    with pytest.raises(ValueError, match="strings"):
        D.check_names(["a", 1, "b"], 3)
    assert D.check_names(None, 2) == ["param_0", "param_1"]
    with pytest.raises(ValueError, match="no column"):
        D.column("grad")
    with pytest.raises(ValueError, match="column"):
        D.column(8)
    assert D.column("dir_rms") == D.DIR_RMS == 4 and D.column(7) == 7
