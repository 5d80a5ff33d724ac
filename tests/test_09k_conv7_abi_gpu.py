"""The 7x7 end convolutions of the auto-encoder (csrc/conv7.hip) through the C ABI, per element and per launch class: vptr_conv7_in_fwd (with
the folded BatchNorm + ReLU and raw) on its three kernels -- the single-channel one, the row-chunk one for 2 - 4 image channels past its first
64-column chunk and above 64 KB of LDS, the first-generation one --, vptr_conv7_in_fwd_planes, vptr_conv7_in_bwd_weight around its 2048-pixel
chunk in both determinism modes, vptr_conv7_out_fwd with out_act 0 / 1 / 2 on both kernels, vptr_conv7_out_bwd_data on the W = 64 kernel up to
its LDS limit and on the first-generation one with Cin 32 / 64 / 128, vptr_conv7_out_bwd_weight with 4 and 16 frames per workgroup, and
vptr_conv7_out_bwd_weight_ws with 3 - 33 partials, sizes that are no multiple of 8, a tile above 64 KB, db = NULL, its three fallbacks and
both determinism modes; every refused argument; ops.conv7_out forward + backward at two sizes whose weight gradient only the workspace kernel
can form.

The cases, the guarded buffers, the fp64 references and the bars live in tests/conv7_cases.py, which tests/test_cpu.py also runs against a CPU
emulation of the calls and against named mutations of it; this file supplies the backend that hands the pointers to the library.  Bars
(DESIGN.md section 3): every element within a worst-case fp32 chain of the operation on absolute values, every channel / weight row within
2e-5 (values) or 5e-5 (gradients) rel-L2, bit equality for everything a call must not touch and for repeated calls where the header promises
it.  The worst figure of every class is in profiles/conv7_margins.md."""
import pytest
import torch

import conv7_cases as C

pytestmark = pytest.mark.gpu


class LibBackend:
    """the library itself: tensors become raw device pointers, the current stream is appended, the return code comes back"""

    def __init__(self, dev):
        from vptr_amd import _lib
        self.dev, self.lib = dev, _lib

    def call(self, name, *args):
        L = self.lib
        for a in args:
            assert not isinstance(a, torch.Tensor) or (a.is_cuda and a.is_contiguous())
        raw = [L.ptr(a) if (a is None or isinstance(a, torch.Tensor)) else a for a in args]
        return getattr(L.lib, "vptr_" + name)(*raw, L.stream())

    def workspace_floats(self, B, Cimg):
        return self.lib.lib.vptr_conv7_out_bwd_weight_workspace(B, Cimg)

    def set_deterministic(self, on):
        self.lib.lib.vptr_set_deterministic(int(on))

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a conv7 call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


def _id(g):
    return "x".join(str(v) for v in g)


# --------------------------------------------------------------------------------------------------------------------- conv7_in
@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "raw"])
@pytest.mark.parametrize("geom", list(C.IN_FWD), ids=_id)
def test_conv7_in_fwd(be, geom, with_scale):
    C.run_in_fwd(be, geom, with_scale)


def test_conv7_in_fwd_rejects(be):
    C.run_in_fwd_rejects(be)


@pytest.mark.parametrize("geom", list(C.IN_PLANES), ids=_id)
def test_conv7_in_fwd_planes(be, geom):
    C.run_in_planes(be, geom)


def test_conv7_in_fwd_planes_rejects(be):
    C.run_in_planes_rejects(be)


@pytest.mark.parametrize("case", C.in_dw_cases(), ids=_id)
def test_conv7_in_bwd_weight(be, case):
    C.run_in_dw(be, *case)


def test_conv7_in_bwd_weight_rejects(be):
    C.run_in_dw_rejects(be)


# -------------------------------------------------------------------------------------------------------------------- conv7_out
@pytest.mark.parametrize("geom", list(C.OUT_FWD), ids=_id)
def test_conv7_out_fwd(be, geom):
    """out_act 0, 1, 2; the activations' own error, measured against fp64 tanh / sigmoid of the out_act = 0 output, stays within the recorded
    conv7_cases.ACT_ERR"""
    C.run_out_fwd(be, geom)


def test_conv7_out_fwd_rejects(be):
    C.run_out_fwd_rejects(be)


@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("geom", list(C.OUT_DX), ids=_id)
def test_conv7_out_bwd_data(be, geom, act):
    C.run_out_dx(be, geom, act)


def test_conv7_out_bwd_data_rejects(be):
    C.run_out_dx_rejects(be)


@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("geom", list(C.OUT_DW), ids=_id)
def test_conv7_out_bwd_weight(be, geom, act):
    C.run_out_dw(be, geom, act)


def test_conv7_out_bwd_weight_rejects(be):
    C.run_out_dw_rejects(be)


@pytest.mark.parametrize("det", [0, 1], ids=["atomic", "det"])
@pytest.mark.parametrize("geom", list(C.OUT_WS), ids=_id)
def test_conv7_out_bwd_weight_ws(be, geom, det):
    """sigmoid in the default mode, tanh in the deterministic one"""
    C.run_out_ws(be, geom, C.TANH if det else C.SIGMOID, det)


def test_conv7_out_bwd_weight_ws_without_db(be):
    C.run_out_ws(be, (2, 3, 9, 11), C.NONE, 0, with_db=False)


@pytest.mark.parametrize("name", list(C.OUT_WS_FALLBACKS))
def test_conv7_out_bwd_weight_ws_fallbacks(be, name):
    C.run_out_ws_fallback(be, name)


def test_conv7_out_bwd_weight_ws_rejects(be):
    C.run_out_ws_rejects(be)


# ------------------------------------------------------------------------------------------------------------------ through ops
@pytest.mark.parametrize("geom", [(2, 3, 9, 11), (1, 1, 8, 128)], ids=_id)
def test_conv7_out_through_ops(dev, geom):
    """ops.conv7_out forward + backward against fp64 autograd of tanh(conv2d(pad(x, reflect)) + b): 9 x 11 has no plain weight-gradient kernel
    (H % 8), so dw and db come from the workspace kernel alone"""
    import vptr_amd.ops as ops
    B, Cimg, H, W = geom
    x, w, b = C.rn((B * H * W, 64), 15000 + H), C.rn((Cimg, 64, 7, 7), 15001 + H, 0.02), C.rn((Cimg,), 15002 + H, 0.3)
    go = C.rn((B, Cimg, H, W), 15003 + H)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    y_ref = torch.tanh(C.conv_ref(C.nchw(xr.view(B, H, W, 64)), wr) + br.view(1, Cimg, 1, 1))
    y_ref.backward(go.double())
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = ops.conv7_out(xd, wd, bd, B, H, W, C.TANH)
    y.backward(go.to(dev))
    torch.cuda.synchronize()
    assert C.slice_rel(y.cpu(), y_ref.detach(), (1,)) < C.TOLV
    assert C.slice_rel(xd.grad.cpu(), xr.grad, (1,)) < C.TOLG
    assert C.slice_rel(wd.grad.cpu(), wr.grad, (0, 2)) < C.TOLG
    assert C.slice_rel(bd.grad.cpu(), br.grad, ()) < C.TOLG
