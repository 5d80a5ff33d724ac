"""vptr_recon_loss_fwd / vptr_recon_loss_bwd (include/vptr_hip_loss.h, csrc/recon_loss.hip) through the C ABI against the criterion
classes in fp64: six geometries x weights none / point / GDL / both x alpha 1, 2, 1.5, 3 x upstream scalars present, each NULL in turn
and all NULL; bit identity with vptr_mse_gdl_fwd / _bwd at the default settings; every documented reject; one graph capture replayed
twice with the weight buffer rewritten in between; `ops.recon_losses` forward + backward against fp64 autograd.

The cases, the guarded buffers, the references and the bars live in tests/recon_loss_cases.py, which tests/test_recon_loss_cpu.py also
runs against a CPU emulation of the calls and its mutations; this file supplies the backend that hands the pointers to the library.
Measured distances: profiles/recon_loss.md."""
import pytest
import torch

import recon_loss_cases as R

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

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:          # a faulted device fails every later call as well: end the run instead of launching more
            pytest.exit("GPU error after a recon-loss call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_recon_loss(be, case):
    """mse, l1, gdl and dpred against MSELoss / L1Loss / GDL on .double() inputs; alpha 1 and 2 at 1e-6 / 2e-6 rel-L2, alpha 1.5 and 3 at
    five times the distance of an fp32 torch evaluation to fp64 (floored at those bars); all upstream scalars NULL: dpred == 0"""
    R.run_case(be, *case)


@pytest.mark.parametrize("geom", R.GEOMS_5D)
def test_default_settings_are_bit_identical_to_mse_gdl(be, geom):
    """w_point = w_gdl = NULL, alpha 1, g_l1 NULL: mse and gdl bit for bit with vptr_mse_gdl_fwd, dpred torch.equal with vptr_mse_gdl_bwd"""
    R.run_bit_identity(be, geom)


def test_rejects(be):
    R.run_rejects(be)


def test_capture_replays_read_the_rewritten_weights(be, dev):
    """forward + backward captured once; two replays with the weight vector rewritten in place between them, each bit-identical to an
    eager call with the values the buffer held; the graph holds kernel nodes only"""
    from vptr_amd.train import graph_node_census
    geom, alpha = "2x3x3x17x5", 1.5
    planes, ppf, T, H, W = R.geometry(geom)
    pred, gt = (t.to(dev).reshape(-1) for t in R.inputs(geom))
    w1, w2 = R.weights(geom, "both")
    wp, wg = w1.to(dev), w2.to(dev)
    gs = [R.scalar(u, dev) for u in R.UPSTREAM["all"]]
    scratch = torch.empty(R.scratch_floats(planes, H), device=dev)

    def launch(out3, dpred):
        assert be.call("recon_loss_fwd", pred, gt, wp, wg, scratch, out3, planes, ppf, T, H, W, alpha) == 0
        assert be.call("recon_loss_bwd", pred, gt, wp, wg, *gs, dpred, planes, ppf, T, H, W, alpha) == 0

    def eager():
        out3, dpred = torch.full((3,), float("nan"), device=dev), torch.full((planes * H * W,), float("nan"), device=dev)
        launch(out3, dpred)
        be.sync()
        return out3.cpu(), dpred.cpu()

    s_out3, s_dpred = torch.empty(3, device=dev), torch.empty(planes * H * W, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(s_out3, s_dpred)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        launch(s_out3, s_dpred)
    nodes = graph_node_census(g)
    assert nodes == {"kernel": 3}, nodes
    g.instantiate()
    seen = []
    for new_p, new_g in ((w1, w2), (w2.flip(0) + 0.25, w1 * 0.5)):
        wp.copy_(new_p.to(dev))
        wg.copy_(new_g.to(dev))
        s_out3.fill_(float("nan"))
        s_dpred.fill_(float("nan"))
        g.replay()
        be.sync()
        got = (s_out3.cpu().clone(), s_dpred.cpu().clone())
        want = eager()
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
        seen.append(got)
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])      # the new weights were read


def _op_reference(pred, gt, wp, wg, alpha, coef, time_dim=1):
    return R.criteria_eval(pred, gt, wp, wg, alpha, coef, torch.float64)


@pytest.mark.parametrize("geom", ["2x3x3x17x5", "2x3x2x1x4x4"])
def test_ops_recon_losses_against_fp64_autograd(dev, geom):
    from vptr_amd import ops
    pred, gt = R.inputs(geom)
    wp, wg = R.weights(geom, "both")
    coef = R.UPSTREAM["all"]
    ref = _op_reference(pred, gt, wp, wg, 2.0, coef)
    p = pred.to(dev).requires_grad_(True)
    mse, l1, gdl = ops.recon_losses(p, gt.to(dev), wp.to(dev), wg.to(dev), gdl_alpha=2.0)
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in (mse, l1, gdl))
    for k, t in (("mse", mse), ("l1", l1), ("gdl", gdl)):
        v = R.record("op %s %s" % (geom, k), abs(float(t.detach()) - ref[k]) / abs(ref[k]), R.TOL_VALUE)
        assert v < R.TOL_VALUE, (geom, k, v)
    (coef[0] * mse + coef[1] * l1 + coef[2] * gdl).backward()
    v = R.record("op %s dpred" % geom, R.rel(p.grad, ref["dpred"]), R.TOL_GRAD)
    assert v < R.TOL_GRAD, (geom, v)
    # a term nobody differentiates reaches the kernel as NULL: the gradient of l1 alone
    ref1 = _op_reference(pred, gt, wp, wg, 2.0, (None, 1.0, None))
    p2 = pred.to(dev).requires_grad_(True)
    ops.recon_losses(p2, gt.to(dev), wp.to(dev), wg.to(dev), gdl_alpha=2.0)[1].backward()
    assert R.rel(p2.grad, ref1["dpred"]) < R.TOL_GRAD
    # the defaults are ops.mse_gdl bit for bit
    p3, p4 = pred.to(dev).requires_grad_(True), pred.to(dev).requires_grad_(True)
    m3, _, g3 = ops.recon_losses(p3, gt.to(dev))
    m4, g4 = ops.mse_gdl(p4, gt.to(dev))
    (g3 + m3).backward()
    (g4 + m4).backward()
    assert R.same_bits(m3, m4) and R.same_bits(g3, g4) and torch.equal(p3.grad, p4.grad)


def test_ops_recon_losses_rejects(dev):
    from vptr_amd import ops
    pred, gt = (t.to(dev) for t in R.inputs("2x3x3x17x5"))
    T = pred.shape[1]
    good = torch.ones(T, device=dev)
    for bad in (torch.ones(T + 1, device=dev), torch.ones(T), torch.ones(T, device=dev, dtype=torch.float64), torch.ones(1, T, device=dev), [1.0] * T):
        with pytest.raises(ValueError):
            ops.recon_losses(pred, gt, w_point=bad)
        with pytest.raises(ValueError):
            ops.recon_losses(pred, gt, w_point=good, w_gdl=bad)
    for alpha in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.recon_losses(pred, gt, gdl_alpha=alpha)
    with pytest.raises(RuntimeError):
        ops.recon_losses(pred, gt[:1])
    with pytest.raises(RuntimeError):
        ops.recon_losses(pred[0], gt[0])                          # 4-D: no time axis to index
    with pytest.raises(RuntimeError):
        ops.recon_losses(pred.cpu(), gt.cpu())
    p = pred.clone().requires_grad_(True)
    t = gt.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no gradient path"):
        ops.recon_losses(p, t)[0].backward()
