"""The nt P16 GEMM against fp64 through the C ABI, per element and per launch class: vptr_gemm with a_mode = VPTR_A_P16 / b_mode = VPTR_B_P16 in
all ten vptr_gemm_p16_kernel<EPI, NST> instantiations and the three epilogue functions EPI 0 chooses between at run time (twelve classes,
helpers.gemm_p16_class), at the smallest geometries at which each path can still go wrong (K = 16, fewer K-steps than the prefetch depth, a tail
step in every K segment, row and column overhangs, N % 16 != 0, the serial epilogue, atomics, batch members, batch_accum, the strided form,
frame_stats, act_grad_src, P16 outputs), every operand encoded on the CPU, every pitch wider than its row, every buffer between canaries.

The cases, the guarded buffers, the references and the bars live in tests/gemm_p16_cases.py, which tests/test_cpu.py also runs against a CPU
emulation of the call and against mutations of that emulation; this file supplies the backend that fills a GemmDesc and calls vptr_gemm.  The
NST = 2 geometries grow with the device's compute units (more tiles than compute units); their fp64 references are taken with torch fp64 on
the device, all others on the CPU."""
import ctypes

import pytest
import torch

import gemm_p16_cases as C

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: the descriptor's tensors become raw device pointers, the return code comes back"""
    dry = False

    def __init__(self, dev):
        from vptr_amd import _lib
        self.dev, self.lib = dev, _lib
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def gemm(self, d):
        L = self.lib
        desc = L.GemmDesc()
        for name, ctype in L.GemmDesc._fields_:
            v = d.get(name)
            if v is None:
                continue
            if isinstance(v, torch.Tensor):
                assert v.is_cuda
                v = v.data_ptr()
            setattr(desc, name, v)
        return L.lib.vptr_gemm(ctypes.byref(desc), L.stream())

    def last_error(self):
        return self.lib.lib.vptr_last_error().decode()

    def mm64(self, a, b):
        dev = self.dev if a.shape[0] > 2048 else "cpu"
        a, b = a.to(dev).double(), b.to(dev).double()
        return (a @ b.t()).cpu(), (a.abs() @ b.abs().t()).cpu()

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a P16 GEMM call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


def test_every_launch_class_is_run_by_two_cases(be):
    """the twelve classes (EPI 1 .. 4 x NST 2 / 4, EPI 0 x batched-4 / rows-halves-2 / serial-2 / serial-4) on THIS device's compute units"""
    census = C.class_census(be.cus)
    assert sorted(census) == sorted(C.CLASSES) and len(census) == 12
    thin = {k: v for k, v in census.items() if len(v) < 2}
    assert not thin, thin


@pytest.mark.parametrize("cid", C.CASES)
def test_gemm_p16(be, cid):
    """every element of D (and Dpre) within its derived bar of the fp64 reference, every row and column below 3e-5 rel-L2, the dropout pattern
    exactly the emulated one, frame_stats against fp64 of the returned D, canaries and inputs bit for bit, no NaN / Inf; the case asserts the
    launch class it reaches on this device (gemm_p16_cases.build)"""
    C.run_case(be, cid)


@pytest.mark.parametrize("k", C.REJECTS)
def test_gemm_p16_rejects(be, k):
    """one descriptor per VPTR_CHECK of vptr_gemm_p16_launch: negative return code, a message, nothing written; host-side, nothing is launched"""
    C.run_reject(be, k)
