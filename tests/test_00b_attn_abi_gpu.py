"""The attention cores through the C ABI against plain torch fp64: vptr_winattn_fwd / _bwd / _bwd_ws, vptr_tattn_fwd / _bwd and vptr_tsattn_fwd /
_bwd called directly (vptr_amd._lib) with the options the trained model runs them with -- P16 outputs, dropout on the probabilities,
dq_scale = head_dim^-0.5 -- in every kernel family (attn16.hip second and first generation, attn_mfma.hip plain and tile-sharing, the 16-token
and the generic fp32 vector kernels of attn.hip), every head-dim instantiation class and every launch class (workgroups that loop over several
problems, windows / pixels per workgroup, slot tails).

The cases, the guarded output buffers, the references and the bars live in tests/attn_abi_cases.py, which tests/test_cpu.py also runs against a
CPU emulation of the calls; this file supplies the backend that hands the pointers to the library.  Bars: forward 5e-5, dq / dk / dv / dbias 1e-4
(fp32 and decoded P16, the project's own), decoded P16 vs the fp32 output of the same call 1e-5 (the format's bound is 2^-17 per element).
Each id names the class its case targets."""
import pytest
import torch

import attn_abi_cases as A
from helpers import ATTN_MODES, TS_GEOMS, attn_geom_route, attn_kernel_mode

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: tensors become raw device pointers, the current stream is appended"""

    def __init__(self, dev):
        import vptr_amd.ops as ops
        from vptr_amd import _lib
        self.dev, self.ops, self.lib = dev, ops, _lib

    def call(self, name, *args):
        L = self.lib
        if name == "winattn_bwd_workspace":
            return L.lib.vptr_winattn_bwd_workspace(*args)
        for a in args:
            assert a is None or not isinstance(a, torch.Tensor) or (a.is_cuda and a.is_contiguous())
        raw = [L.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
        L.check(getattr(L.lib, "vptr_" + name)(*raw, L.stream()), "vptr_" + name)

    def seed(self, value):
        self.ops.manual_seed(self.dev, value)
        self.ops.new_seed_scope(self.dev)
        return self.ops.seed_tensor(self.dev).clone()

    def dropout_mask(self, n, p, seed, site):
        L = self.lib
        ones, md = torch.ones(n, device=self.dev), torch.empty(n, device=self.dev)
        L.check(L.lib.vptr_dropout(L.ptr(ones), L.ptr(md), n, p, L.ptr(seed), site, L.stream()), "vptr_dropout")
        return md


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.fixture
def attn_mode(request):
    """every case names its kernel family (helpers.attn_kernel_mode) as its `mode` parameter"""
    with attn_kernel_mode(request.getfixturevalue("mode")) as mode:
        yield mode


def _ids(rows):
    return ["-".join(str(x) for x in r) for r in rows]


# mode is the innermost loop: the cases that share a (cached) reference run back to back
HEAD_CASES = [(hc, g, m) for hc in A.HEAD_CLASSES for g in A.GEOMS for m in A.head_modes(hc, ATTN_MODES)]
DROP_CASES = [(hc, g, m) for hc in A.DROP_HEADS for g in A.DROP_GEOMS for m in ATTN_MODES]
LAUNCH = [(name, "nh%d_C%d" % hc, m) for name, (_, hcs, modes) in A.LAUNCH_CASES.items() for hc in hcs for m in (modes or ATTN_MODES)]


@pytest.mark.parametrize("hc,geom,mode", HEAD_CASES, ids=_ids(HEAD_CASES))
def test_head_class(be, attn_mode, hc, geom, mode):
    """every head-dim instantiation class x geometry x kernel family: fp32 and (C % 16 == 0) P16 outputs vs fp64, dq_scale = hd^-0.5"""
    nh, C = A.HEAD_CLASSES[hc]
    A.run_parity(be, A.GEOMS[geom], nh, C)


@pytest.mark.parametrize("hc,geom,mode", DROP_CASES, ids=_ids(DROP_CASES))
def test_dropout_on_probabilities(be, attn_mode, hc, geom, mode):
    """dropout 0.1 (site 7) on the probabilities with P16 outputs vs the fp64 reference under the regenerated mask"""
    nh, C = A.HEAD_CLASSES[hc]
    A.run_dropout(be, A.GEOMS[geom], nh, C)


@pytest.mark.parametrize("name,hc,mode", LAUNCH, ids=_ids(LAUNCH))
def test_launch_class(be, attn_mode, name, hc, mode):
    """launch classes the small cases do not reach: workgroups looping over several problems with the next one's loads in flight (1547 windows /
    1551 pixels exceed every attn16 grid), wpb 2 / 4 / 8 with a tail, 4 pixels per wave (T = 10 and its limit T = 11 at hd 66, T = 16 beyond it),
    attn_mfma slots with nprob % slots != 0 (nh = 3)"""
    geom = A.LAUNCH_CASES[name][0]
    nh, C = (int(x[2:] if x.startswith("nh") else x[1:]) for x in hc.split("_"))
    A.run_parity(be, geom, nh, C)


@pytest.mark.parametrize("geom,mode", [(g, m) for g in A.TABLE_GEOMS for m in ATTN_MODES])
def test_table_gradient_is_accumulated(be, attn_mode, geom, mode):
    """dbias_table starts from seeded non-zero values (result - start == reference at 1e-4); dbias_table == NULL with a bias table"""
    A.run_table_contract(be, A.TABLE_GEOMS[geom], 2, 48)


@pytest.mark.parametrize("nh,C", [(2, 48), (8, 192)])
def test_table_gradient_workspace(be, nh, C):
    """vptr_winattn_bwd_ws at 1547 windows (the full grid of the second-generation backward) with the full workspace (twice: bit-identical table
    gradient, as the header promises), a workspace one float too small (atomic fallback) and NULL"""
    with attn_kernel_mode("default"):
        A.run_workspace_contract(be, A.LAUNCH_CASES["win4_1547win_loop_wpb8_tail"][0], nh, C)


@pytest.mark.parametrize("geom,nh,C", [("win4_B3_8x8_bias", 2, 48), ("t5x5_causal", 8, 528)])
def test_unaligned_tensors_take_first_generation(be, geom, nh, C):
    """default routing, fp32 outputs, every tensor 8 bytes past a 16-byte boundary: the second-generation attn16 kernels need 16-byte aligned
    rows, so the call falls back to the first generation, forward and backward (vptr_attn_route says so), and meets the same bars"""
    with attn_kernel_mode("default"):
        for backward in (0, 1):
            assert attn_geom_route(A.GEOMS[geom], nh, C, backward, aligned16=0)[0] == "a16_gen1"
            assert attn_geom_route(A.GEOMS[geom], nh, C, backward, aligned16=1)[0] == "a16_gen2"
        A.run_unaligned(be, A.GEOMS[geom], nh, C)


@pytest.mark.parametrize("N,Tq,Tk,H,W,ws,C,nh", [TS_GEOMS[0], TS_GEOMS[1], TS_GEOMS[5]])
def test_tslma_p16(be, N, Tq, Tk, H, W, ws, C, nh):
    """vptr_tsattn_fwd / _bwd with fp32 and P16 outputs on guarded buffers, same bars"""
    A.run_tslma(be, N, Tq, Tk, H, W, ws, C, nh)


def test_argument_guards(be):
    """p16 with C % 16 != 0 (each entry point), causal with Tq != Tk, ws * ws > 64, dropout without a seed: RuntimeError before any launch"""
    def raises(fn):
        with pytest.raises(RuntimeError):
            fn()
    A.run_guards(be, raises)
    torch.cuda.synchronize()
