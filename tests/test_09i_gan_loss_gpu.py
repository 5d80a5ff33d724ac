"""vptr_gan_loss_fwd / vptr_gan_loss_bwd (include/vptr_hip_gan.h, csrc/gan_loss.hip) through the C ABI against `GANLoss` in fp64: three
modes x nine geometries (n = 1, 3, one below / at / above the workgroup's chunk, 2880, 70 001; na != nb; xb NULL; stride 4 with NaN in
the gaps) x four settings (logit scales 0.5, 3, 20 around the planted values 0, -0, +-30, +-90, +-104; labels (1, 0) and (0.9, 0.1); coef
0.005 and 1) x five combinations of the upstream scalars, dxa or dxb NULL; every documented reject; two calls bit for bit; one graph
capture replayed with the logits rewritten in between; `ops.gan_loss` / `ops.gan_loss_pair` forward + backward against fp64 autograd.

The cases, the guarded buffers, the references and the bars live in tests/gan_loss_cases.py, which tests/test_gan_loss_cpu.py also runs
against a CPU emulation of the calls and its mutations; this file supplies the backend that hands the pointers to the library.
Measured distances: profiles/gan_loss.md."""
import pytest
import torch

import gan_loss_cases as G

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
            pytest.exit("GPU error after a gan-loss call: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def be(dev):
    return LibBackend(dev)


@pytest.mark.parametrize("case", G.all_cases(), ids=G.case_id)
def test_gan_loss(be, case):
    """out3 and both gradients against GANLoss on .double() inputs inside the derived bars of gan_loss_cases; all upstream scalars NULL:
    dx == 0; a gradient that is not wanted leaves the other one bit for bit"""
    G.run_case(be, *case)


def test_rejects(be):
    G.run_rejects(be)


@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_two_calls_are_bit_identical(be, mode):
    G.run_twice_identical(be, mode, "n70001", "s3_soft")


def test_capture_replays_read_the_rewritten_logits(be, dev):
    """forward + backward captured once; two replays with the logits rewritten in place between them, each bit-identical to an eager
    call on the values the buffers held; the graph holds three kernel nodes and nothing else"""
    from vptr_amd.train import graph_node_census
    geom, setting, mode = "n2880_2160_s4_1", "s3_soft", "vanilla"
    na, nb, sa, sb, ar, br = G.GEOMS[geom]
    _, (rl, fl), coef = G.SETTINGS[setting]
    xa, xb = G.inputs(geom, setting)
    da, db = G.strided(xa, sa, dev), G.strided(xb, sb, dev)
    gs = [G.scalar(u, dev) for u in G.UPSTREAM["all"]]
    scratch = torch.empty(G.scratch_floats(na, nb), device=dev)

    def launch(out3, dxa, dxb):
        assert be.call("gan_loss_fwd", da, na, sa, ar, db, nb, sb, br, G.MODES[mode], rl, fl, coef, scratch, out3) == 0
        assert be.call("gan_loss_bwd", da, na, sa, ar, dxa, db, nb, sb, br, dxb, G.MODES[mode], rl, fl, coef, *gs) == 0

    def fresh():
        return [torch.full((n,), G.NAN, device=dev) for n in (3, na, nb)]

    def eager():
        outs = fresh()
        launch(*outs)
        be.sync()
        return [o.cpu() for o in outs]

    static = [torch.empty(n, device=dev) for n in (3, na, nb)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(*static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        launch(*static)
    nodes = graph_node_census(g)
    assert set(nodes) <= {"kernel", "memcpy", "empty"} and nodes == {"kernel": 3}, nodes
    g.instantiate()
    seen = []
    for shift in (0.0, 0.75):
        da[::sa] = (xa + shift).to(dev)
        db[::sb] = (xb * (1.0 + shift)).to(dev)
        for s in static:
            s.fill_(G.NAN)
        g.replay()
        be.sync()
        got = [s.cpu().clone() for s in static]
        want = eager()
        assert all(G.same_bits(a, b) for a, b in zip(got, want))
        assert all(bool(torch.isfinite(a).all()) for a in got)
        seen.append(got)
    assert all(not torch.equal(a, b) for a, b in zip(*seen))                                # the new logits were read


def _check_op(tag, got, grads, ref, mode, xs, ts, coef, ups):
    bounds = [G.value_bound(mode, x, t) for x, t in zip(xs, ts)]
    bounds = bounds + [0.0] * (2 - len(bounds))
    bounds.append(abs(G.f32(coef)) * (bounds[0] + bounds[1]))
    for i, v in enumerate(got):
        d = G.record("op %s out[%d]" % (tag, i), abs(float(v.detach()) - ref["out"][i]), bounds[i])
        assert d <= bounds[i], (tag, i, float(v.detach()), ref["out"][i])
    for name, d, x, t, g in zip(("dxa", "dxb"), grads, xs, ts, ups[:2]):
        g_eff = (0.0 if g is None else G.f32(g)) + G.f32(coef) * (0.0 if ups[2] is None else G.f32(ups[2]))
        units = float(((d.detach().cpu().double().reshape(-1) - ref[name]).abs() / G.grad_bound(mode, x, t, g_eff)).max()) * G.GRAD_UNITS
        G.record("op %s %s" % (tag, name), units, G.GRAD_UNITS)
        assert units <= G.GRAD_UNITS, (tag, name, units)


@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_ops_against_fp64_autograd(dev, mode):
    """`ops.gan_loss_pair` on a contiguous tensor beside a channel slice y[:, :1] read in place (the other channels hold NaN), and
    `ops.gan_loss` on a view without a uniform stride (made contiguous), against GANLoss in fp64"""
    from vptr_amd import ops
    setting = "s3_soft"
    _, labels, _ = G.SETTINGS[setting]
    rl, fl = (G.f32(v) for v in labels)
    coef, ups = 0.005, G.UPSTREAM["all"]
    xa, xb = G.logits(2160, 9100, 3.0), G.logits(2880, 9200, 3.0)
    fake = xa.view(15, 1, 12, 12).to(dev).requires_grad_(True)
    buf = torch.full((2880, 4), G.NAN, device=dev)
    buf[:, 0] = xb.to(dev)
    buf.requires_grad_(True)
    real = buf[:, :1]
    l_fake, l_real, total = ops.gan_loss_pair(fake, real, coef, mode=mode, real_label=labels[0], fake_label=labels[1])
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in (l_fake, l_real, total))
    (ups[0] * l_fake + ups[1] * l_real + ups[2] * total).backward()
    ref = G.criterion_eval(mode, xa, False, xb, True, labels, coef, ups)
    assert fake.grad.shape == fake.shape and bool(torch.isnan(buf.grad[:, 1:]).logical_not().all())
    _check_op("pair " + mode, (l_fake, l_real, total), (fake.grad, buf.grad[:, 0]), ref, mode, (xa, xb), (fl, rl), coef, ups)
    assert float(buf.grad[:, 1:].abs().max()) == 0.0                                        # the gap channels get no gradient
    # the total alone, as the discriminator update differentiates it: g_a = g_b = NULL
    f2 = xa.to(dev).requires_grad_(True)
    r2 = xb.to(dev).requires_grad_(True)
    ops.gan_loss_pair(f2, r2, coef, mode=mode, real_label=labels[0], fake_label=labels[1])[2].backward()
    ref2 = G.criterion_eval(mode, xa, False, xb, True, labels, coef, (None, None, 1.0))
    _check_op("pair-total " + mode, (), (f2.grad, r2.grad), ref2, mode, (xa, xb), (fl, rl), coef, (None, None, 1.0))
    # one tensor; a transposed view has no uniform stride
    base = G.logits(2880, 9300, 3.0)
    y = base.view(40, 72).to(dev).requires_grad_(True)
    loss = ops.gan_loss(y.t(), True, mode=mode, real_label=labels[0], fake_label=labels[1])
    (1.3 * loss).backward()
    xt = base.view(40, 72).t().reshape(-1)
    ref3 = G.criterion_eval(mode, xt, True, None, False, labels, 1.0, (1.3, None, None))
    _check_op("single " + mode, (loss,), (y.grad.t(),), ref3, mode, (xt,), (rl,), 1.0, (1.3, None, None))
    # the trainers' default labels: GANLoss(mode, 1.0, 0.0)
    ref4 = G.criterion_eval(mode, xa, False, None, False, (1.0, 0.0), 1.0, (None, None, None))
    v = ops.gan_loss(xa.to(dev), False, mode=mode)
    assert abs(float(v) - ref4["out"][0]) <= G.value_bound(mode, xa, 0.0)


def test_ops_refuse(dev):
    from vptr_amd import ops
    x = torch.zeros(8, device=dev)
    with pytest.raises(RuntimeError):
        ops.gan_loss(x.cpu(), True)
    with pytest.raises(RuntimeError):
        ops.gan_loss_pair(x, x.cpu(), 0.5)
    with pytest.raises(RuntimeError):
        ops.gan_loss(x.double(), True)
    with pytest.raises(RuntimeError):
        ops.gan_loss(x[:0], True)
    with pytest.raises(ValueError):
        ops.gan_loss(x, True, mode="hinge")
    with pytest.raises(ValueError):
        ops.gan_loss_pair(x, x, float("nan"))
    with pytest.raises(ValueError):
        ops.gan_loss(x, True, real_label=float("inf"))
