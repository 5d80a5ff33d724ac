"""The fp32-staged MFMA GEMM against fp64 through the C ABI, per element and per launch class: vptr_gemm with a_mode 0 / 1 / 2 and b_mode 0 / 1
(csrc/gemm.hip) in both main loops (the pipelined vptr_gemm_kernel_p and, from 384 workgroups on, the single-image vptr_gemm_kernel), the four
epilogue functions they choose between, NFN 4 / 8 / 11, every operand stager at both precisions, the implicit-GEMM convolution with its paddings
and its transposed and sub-pixel forms, split-K and atomics, K segments, batch members and a_rowsum -- at the smallest geometries that reach each
path, every pitch wider than its row, every buffer between canaries.

The cases, references, bars and the CPU emulation live in tests/gemm_f32_cases.py (tests/test_cpu.py runs them against the emulation and its
mutations); this file supplies the backend that fills a GemmDesc and calls vptr_gemm.  fp64 products of more than 2048 rows are taken with torch
fp64 on the device, all others on the CPU."""
import ctypes

import pytest
import torch

import gemm_f32_cases as C

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: the descriptor's tensors become raw device pointers, the return code comes back"""
    dry = False

    def __init__(self, dev):
        from vptr_amd import _lib
        self.dev, self.lib = dev, _lib

    def gemm(self, d):
        L = self.lib
        if d is None:
            return L.lib.vptr_gemm(None, L.stream())
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
        return (a.to(dev).double() @ b.to(dev).double().t()).cpu()

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after an fp32-staged GEMM call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


def test_census_of_launch_classes():
    """all ten (loop, epilogue, NFN) combinations by two cases or more and with the full epilogue option set, the five operand-mode pairs, both
    B stagers at each NFN and every stager at precision 1, in both loops (no device property enters the class)"""
    census = C.class_census()
    assert not C.census_gaps(census), C.census_gaps(census)
    assert sum(len(v) for v in census.values()) == len(C.CASES)


@pytest.mark.parametrize("name", C.CASES)
def test_gemm_f32(be, name):
    """every element of D (and Dpre, a_rowsum) within its derived bar of the fp64 reference, every row and column below TOL3 / TOL1 of the raw
    fp64 product, the dropout pattern exactly the emulated one with +0 for dropped elements, canaries and inputs bit for bit, no NaN / Inf; the
    case asserts the launch class and the grid it reaches (gemm_f32_cases.build)"""
    C.run_case(be, name)


@pytest.mark.parametrize("k", C.REJECTS)
def test_gemm_f32_rejects(be, k):
    """the null descriptor and one descriptor per VPTR_CHECK of vptr_gemm that fp32-staged operands reach: negative return code, a message,
    nothing written; host-side"""
    C.run_reject(be, k)
