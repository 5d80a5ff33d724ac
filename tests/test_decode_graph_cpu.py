"""The device-held decoding position without a GPU: the header against the binding table, an fp32 CPU emulation of the three entry
points run through the direct-call checks of tests/test_12b_decode_graph_gpu.py (and caught by them under named mutations), and the
host-side rules of `FARCache(device_pos=True)`, `far_rollout(graph=)` and `CachedDecoder` that need no device."""
import inspect
import os
import re

import pytest
import torch

import decode_graph_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ 1. header and bindings
def test_header_matches_binding_table():
    from vptr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vptr_hip_decode.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(vptr_\w+)\s*\(([^)]*)\)\s*;", body)}
    assert set(decls) == set(_lib.DECODE_SIGNATURES) == {"vptr_decode_begin", "vptr_tattn_step_pos", "vptr_decode_advance"}
    for name, args in decls.items():
        want = []
        for a in (x.strip() for x in args.split(",")):
            want.append(_lib.P if ("*" in a or a.startswith("vptr_stream_t")) else _lib.I)
            assert "*" in a or a.startswith("vptr_stream_t") or a.startswith("int "), a
        assert _lib.DECODE_SIGNATURES[name] == want, name
        assert args.split(",")[-1].strip() == "vptr_stream_t stream"
    for word, val in (("WORDS", D.WORDS), ("POS", D.POS), ("TCAP", D.TCAP), ("OVERFLOW", D.OVERFLOW), ("STEPS", D.STEPS), ("MAXT", D.MAXT)):
        assert int(re.search(r"#define\s+VPTR_DECODE_%s\s+(\d+)" % word, hdr).group(1)) == val
    assert D.WORDS * 4 == 64


def test_existing_abi_is_untouched():
    from vptr_amd import _lib
    assert len(_lib.EXPORTS) == 77 and not set(_lib.DECODE_SIGNATURES) & set(_lib.EXPORTS)
    assert _lib.SIGNATURES["vptr_tattn_step"] == [_lib.P] * 4 + [_lib.I] * 6 + [_lib.P]
    assert _lib.lib.vptr_abi_version() == 10
    import vptr_amd.ops as ops
    assert (ops.DECODE_WORDS, ops.DECODE_POS, ops.DECODE_TCAP, ops.DECODE_OVERFLOW, ops.DECODE_STEPS, ops.DECODE_MAXT) == \
        (D.WORDS, D.POS, D.TCAP, D.OVERFLOW, D.STEPS, D.MAXT)


# ------------------------------------------------------------------------------------------------------ 2. the emulation
def _runners(mut=None):
    def step(q, kn, vn, kc, vc, o, rec, rows, Tcap, C, nh, p16):
        D.emu_step_pos(q, kn, vn, kc, vc, o, rec, nh, mut)

    def begin(rec, tpos, cur, Tmax, C):
        D.emu_begin(rec, tpos, cur, mut)

    def advance(rec):
        D.emu_advance(rec, mut)
    return step, begin, advance


def _all_failures(mut=None):
    step, begin, advance = _runners(mut)
    bad = []
    for case in D.STEP_CASES:
        bad += ["%s: %s" % (case, b) for b in D.check_step_case(step, case)]
    bad += D.check_full_case(step, 17, 5, 48, 4)
    for C in (15, 528):
        bad += D.check_begin(begin, C, 6)
    bad += D.check_advance(advance, 5)
    return bad


def test_emulation_passes_the_direct_call_checks():
    assert _all_failures() == []


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_checks_catch_mutation(mut):
    bad = _all_failures(mut)
    assert bad, "the direct-call checks do not notice the mutation %r" % mut


def test_full_cache_and_advance_count_overflow():
    step, _, advance = _runners()
    rec = D.record(5, 5)
    advance(rec)
    assert rec.tolist()[:4] == [5, 5, 1, 0]


# ------------------------------------------------------------------------------------------------------ 3. host rules
def test_keyword_defaults_are_off():
    from vptr_amd.inference import far_rollout
    from vptr_amd.model.vidhrformer import FARCache
    from vptr_amd.train import FARTrainer
    import vptr_amd.ops as ops
    assert inspect.signature(far_rollout).parameters["graph"].default is False
    assert inspect.signature(FARTrainer.predict).parameters["graph"].default is False
    assert inspect.signature(FARCache.__init__).parameters["device_pos"].default is False
    sig = inspect.signature(ops.proj_temporal_attention_step).parameters
    assert sig["pos"].default is None and sig["staging"].default is None


def test_graph_without_kv_cache_is_a_value_error():
    from vptr_amd.inference import far_rollout
    with pytest.raises(ValueError):
        far_rollout(None, None, None, torch.zeros(1, 2, 1, 8, 8), 3, kv_cache=False, graph=True)


def test_host_mirror_and_capacity_on_cpu_tensors():
    """the record, the mirror and the capacity rule of FARCache(device_pos=True); fill_ on a CPU tensor stands in for the fill kernel"""
    from vptr_amd.model.vidhrformer import FARCache
    c = FARCache(2, 6, 1, 2, 2, 16, "cpu", device_pos=True)
    assert c.pos.dtype == torch.int32 and c.pos.numel() == D.WORDS and c.pos.tolist()[:4] == [0, 6, 0, 0]
    assert c.tpos_cur.shape == (16,) and [tuple(s.shape) for s in c.staging] == [(4, 16), (4, 16)]
    c.len = 3
    c.put_pos(3)
    assert c.counters() == {"pos": 3, "tcap": 6, "overflow": 0, "steps": 0}
    c.check()
    c.pos[D.OVERFLOW] = 1
    with pytest.raises(RuntimeError):
        c.check()
    c.reset()
    assert c.len == 0 and c.pos[D.POS] == 0
    plain = FARCache(2, 6, 1, 2, 2, 16, "cpu")
    assert plain.pos is None and plain.staging is None
    plain.check()
    with pytest.raises(ValueError):
        FARCache(1, D.MAXT + 1, 1, 2, 2, 16, "cpu", device_pos=True)


class _Stub(torch.nn.Module):
    pass


def test_cached_decoder_rejects_before_touching_a_device():
    from vptr_amd.inference import CachedDecoder
    e, d, t = _Stub().eval(), _Stub().eval(), _Stub().eval()
    with pytest.raises(ValueError):
        CachedDecoder(e, d, t, 2, "NAR")
    with pytest.raises(ValueError):
        CachedDecoder(e, d, _Stub().train(), 2, "RIL")
    with pytest.raises(ValueError):
        CachedDecoder(_Stub().train(), d, t, 2, "RIP")
    with pytest.raises(ValueError):
        CachedDecoder(e, d, t, 0, "RIL")
