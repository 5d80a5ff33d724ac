"""Host-side checks of the conv-FFN backward entry points of include/vptr_hip_convffn.h: the ABI table against the header and the library, and
the argument checks of the two calls, which run before any launch and can therefore be exercised without a device (the pointers are never
dereferenced on the host)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_convffn_signatures_match_header_and_library():
    from vptr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vptr_hip_convffn.h")).read()
    assert '#include "vptr_hip.h"' in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vptr_\w+)\s*\(", code))
    assert declared == set(_lib.CONVFFN_SIGNATURES) == {"vptr_norm_act_bwd_sums", "vptr_dwconv3x3_norm_bwd"}
    others = set(_lib.EXPORTS) | set(_lib.EXT_SIGNATURES) | set(_lib.OPTIM_SIGNATURES)
    assert not declared & others
    for name, argt in _lib.CONVFFN_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == argt and fn.restype is _lib.c_int
        decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(argt), name           # one ctypes entry per declared parameter
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10


P = ctypes.c_void_p(1 << 20)          # a 16-byte aligned non-null address (never dereferenced: every call below is rejected first)
ODD = ctypes.c_void_p((1 << 20) + 4)


def _fused(lib, frames=4, H=8, W=8, F=64, p=0.0, seed=None, dy=P, ah=P, fpg=0):
    return lib.vptr_dwconv3x3_norm_bwd(dy, P, P, P, P, P, P, 1, p, seed, 0, ah, P, P, P, P, frames, H, W, F, fpg, None)


@pytest.mark.parametrize("kw,word", [(dict(W=5), "W even"), (dict(F=48), "F %"), (dict(H=16, W=8), "64 pixels"), (dict(W=2, H=8, F=64), "(W/2)*(F/4)"),
                                     (dict(p=0.1), "seed_dev"), (dict(p=1.0, seed=P), "p < 1"), (dict(dy=ODD), "aligned"), (dict(ah=ODD), "aligned"),
                                     (dict(frames=0), "bad arguments"), (dict(fpg=-1), "bad arguments"), (dict(frames=65536, fpg=1), "65535")])
def test_dwconv3x3_norm_bwd_rejects_on_the_host(kw, word):
    from vptr_amd import _lib
    assert _lib.lib.vptr_get_deterministic() == 0
    assert _fused(_lib.lib, **kw) < 0
    msg = _lib.lib.vptr_last_error().decode()
    assert "dwconv3x3_norm_bwd" in msg and word in msg, msg


def test_dwconv3x3_norm_bwd_refuses_the_deterministic_mode():
    from vptr_amd import _lib
    lib = _lib.lib
    prev = lib.vptr_get_deterministic()
    lib.vptr_set_deterministic(1)
    try:
        assert _fused(lib) < 0
        assert "deterministic" in lib.vptr_last_error().decode()
    finally:
        lib.vptr_set_deterministic(prev)


def test_norm_act_bwd_sums_rejects_on_the_host():
    from vptr_amd import _lib
    lib = _lib.lib

    def call(rows=128, F=32, HW=16, p=0.0, seed=None, dw=P, db=P, part=None, dy=P):
        return lib.vptr_norm_act_bwd_sums(dy, P, P, P, P, P, dw, db, P, rows, F, HW, 1, p, seed, 0, part, None)
    for kw, word in ((dict(rows=130), "multiple of HW"), (dict(F=30), "multiple of 4"), (dict(dw=None), "bad arguments"), (dict(p=0.1), "seed_dev"),
                     (dict(dy=ODD), "aligned"), (dict(part=P), "no deferred variant")):      # 8 frames < 64: no partial rows
        assert call(**kw) < 0, kw
        assert word in lib.vptr_last_error().decode(), (kw, lib.vptr_last_error().decode())
    assert lib.vptr_norm_act_bwd_partials(128, 32, 16, 0) == 0


def test_bwd_predicate_follows_the_kernel_geometry():
    import vptr_amd.ops as ops
    ok = ops.norm_dwconv_bwd_ok
    assert ok(64, 2112, 8, 8) and ok(16, 128, 4, 4) and ok(32, 64, 4, 8)
    assert not ok(256, 2112, 16, 16)      # more than 64 pixels
    assert not ok(64, 48, 8, 8)           # F % 64
    assert not ok(20, 64, 4, 5)           # odd W
    assert not ok(64, 64, 8, 4)           # H * W != HW
    prev = ops.config.fused_convffn_bwd
    try:
        ops.config.fused_convffn_bwd = False
        assert not ok(64, 2112, 8, 8)
    finally:
        ops.config.fused_convffn_bwd = prev
