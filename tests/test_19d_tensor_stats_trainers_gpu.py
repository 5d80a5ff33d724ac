"""Per-tensor statistics on the trainers (`tensor_stats=` of NARTrainer / FARTrainer / FlatAdamW, `opt.tensor_stats`), on the tiny fixtures
of tests/validation_cases.py in deterministic mode, set up as tests/test_19c_param_groups_trainers_gpu.py does:

  * after a step every row against torch on `p.grad`, `p` and the optimizer's moments BY NAME inside the bars of tests/tensor_stats_cases.py
    (channel-last stored parameters included), and row S against the step's own "grad_norm" at the 1e-6 sum-of-squares bar of
    tests/test_09d_step_tail_gpu.py;
  * the trajectory is bit-identical to a twin with a constant schedule and no statistics;
  * capture: the node census is the controlled trainer's plus two kernel nodes, no memset node; `set_every` between replays takes effect;
  * a FlatAdamW with skip_nonfinite and a NaN in one parameter's gradient: skipped, parameters bit for bit, `culprits()` names it;
  * a view through `DeviceLossMeters`; `accum_steps=2, every=2` samples the closes only; `report()`; AETrainer and misuse raise."""
import numpy as np
import pytest
import torch

import tensor_stats_cases as T
import validation_cases as V
from vptr_amd import diagnostics as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import vptr_amd.model as pkg
    return pkg


@pytest.fixture(autouse=True)
def _deterministic(dev):
    from vptr_amd import ops
    ops.unregister_flat_slabs()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)
    ops.unregister_flat_slabs()


def _trainer(pkg, kind, dev, **ctl):
    from vptr_amd import ops
    from vptr_amd.train import FARTrainer, NARTrainer
    c = V.case(kind)
    enc, dec, Tm, _ = V.modules(pkg, c)
    ops.manual_seed(dev, 77)
    if kind == "nar":
        tr = NARTrainer(enc.to(dev), dec.to(dev), Tm.to(dev), batch_size=c["meta"]["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **ctl)
    else:
        tr = FARTrainer(enc.to(dev), dec.to(dev), Tm.to(dev), lr=1e-4, max_grad_norm=1.0, **ctl)
    return tr, c


def _batch(c, s, dev):
    past, fut = V.batch(c, s)
    return past.to(dev), fut.to(dev)


def _slabs(tr):
    o = tr.opt
    return [t.clone() for t in (o.flat, o.m, o.v, o.step_dev)]


def _named_reference(tr, scale=1.0):
    """the fp64 table from the parameters as torch sees them, in `named_parameters()` order: (names, [S + 1, 8])"""
    from vptr_amd.optim import S_EPS, S_INV_SQRT_BC2
    opt = tr.opt
    named = [(n, p) for n, p in tr.T.named_parameters() if p.requires_grad]
    assert [id(p) for _, p in named] == [id(p) for p in opt.params]
    flat = lambda ts: torch.cat([t.detach().cpu().reshape(-1) for t in ts])
    state = opt.ctl.state.cpu()
    ref = T.ref_table(flat([p for _, p in named]), flat([p.grad for _, p in named]), flat([opt._logical(opt.m, i) for i in range(len(named))]),
                      flat([opt._logical(opt.v, i) for i in range(len(named))]), [p.numel() for _, p in named], scale,
                      float(state[S_INV_SQRT_BC2]), float(state[S_EPS]), True)
    return [n for n, _ in named], ref


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_rows_against_torch_by_name(pkg, dev, kind):
    tr, c = _trainer(pkg, kind, dev, tensor_stats=D.TensorStats())
    ts = tr.opt.tensor_stats
    assert tr.opt.ctl is not None and ts.S == len(tr.opt.params) and tuple(ts.table.shape) == (ts.S + 1, 8)
    assert any(cl is not None for _, _, cl in tr.opt._layout), "the fixture has no channel-last stored parameter"
    for s in range(2):
        out = tr.step(*_batch(c, s, dev))
    names, ref = _named_reference(tr)
    assert names == ts.names and float(ts.computed()) == 1.0 and float(ts.age()) == 0.0
    worst = T.check_table(ts.table, ref, True, kind)
    print("%s: %d tensors, worst norm %.3f, worst dir_rms %.3f of their bars" % (kind, ts.S, worst["norm"], worst["dir"]))
    for n, p in tr.T.named_parameters():        # and once more through the public view, by name
        assert abs(float(ts.view(n, "weight_norm")) - float(p.detach().double().norm())) <= T.NORM_RTOL * float(p.detach().double().norm()), n
        assert float(ts.view(n, "grad_maxabs")) == float(p.grad.abs().max()), n
    a, b = float(ts.view("<all>", "grad_norm")) ** 2, float(out["grad_norm"]) ** 2
    print("%s: row S grad_norm^2 against the step's own: %.3e relative" % (kind, abs(a - b) / a))
    assert abs(a - b) <= 1e-6 * a
    rep = ts.report(top=5)
    assert len(rep) == 5 and all(rep[i]["grad_norm"] >= rep[i + 1]["grad_norm"] for i in range(4)) and set(D.COLUMNS) <= set(rep[0])
    i = ts.row(rep[0]["name"])
    lr = float(tr.opt.lr_now())
    want = lr * float(ts.table[i, D.DIR_RMS]) * ts.sizes[i] ** 0.5 / float(ts.table[i, D.WEIGHT_NORM])
    assert rep[0]["update_ratio"] == pytest.approx(want, rel=1e-12) and 0.0 < want < 1.0
    assert ts.culprits() == []
    assert not any("tensor" in str(k) or "stats" in str(k) for k in tr.opt.state_dict()["param_groups"][0])


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_trajectory_is_bit_identical_to_a_twin_without_statistics(pkg, dev, kind):
    from vptr_amd.optim import LRSchedule
    runs = []
    for ctl in (dict(schedule=LRSchedule()), dict(tensor_stats=D.TensorStats(every=2))):
        tr, c = _trainer(pkg, kind, dev, **ctl)
        outs = [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(3)]
        runs.append((outs, _slabs(tr), tr.opt.tensor_stats))
        del tr
    (oa, sa, ta), (ob, sb, tb) = runs
    assert ta is None and tb is not None
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(x, y), "slab %d differs in %d elements" % (i, int((x != y).sum()))
    assert oa == ob, (oa, ob)
    assert (float(tb.ctl[D.C_PHASE]), float(tb.computed()), float(tb.age())) == (1.0, 0.0, 1.0)      # three calls at every = 2


def test_capture_census_and_set_every_between_replays(pkg, dev):
    from vptr_amd import ops
    from vptr_amd.optim import LRSchedule
    tw, c = _trainer(pkg, "far", dev, schedule=LRSchedule())
    past, fut = _batch(c, 0, dev)
    tw.capture(past, fut, warmup=1)
    controlled = dict(tw.graph_nodes)
    del tw
    ops.unregister_flat_slabs()
    tr, c = _trainer(pkg, "far", dev, tensor_stats=D.TensorStats(every=3))
    tr.capture(past, fut, warmup=1)
    census = dict(tr.graph_nodes)
    print("census: controlled %r, with statistics %r" % (controlled, census))
    assert census == dict(controlled, kernel=controlled["kernel"] + 2) and "memset" not in census
    ts = tr.opt.tensor_stats
    ts.set_every(1)
    tr.step(past, fut)
    assert float(ts.computed()) == 1.0 and float(ts.ctl[D.C_PHASE]) == 0.0
    first = ts.table.clone()
    T.check_table(first, _named_reference(tr)[1], True, "replay at every = 1")
    ts.set_every(2)
    tr.step(past, fut)
    assert (float(ts.computed()), float(ts.age())) == (0.0, 1.0) and torch.equal(ts.table, first), "a replay that is not due wrote the table"
    tr.step(past, fut)
    assert (float(ts.computed()), float(ts.age())) == (1.0, 0.0) and not torch.equal(ts.table, first)
    T.check_table(ts.table, _named_reference(tr)[1], True, "replay at every = 2")


def test_skipped_step_names_the_culprit(dev):
    from vptr_amd.train import FlatAdamW
    shapes = {"0.weight": (33, 9), "0.bias": (33,), "1.weight": (33,), "2.weight": (130, 33), "2.bias": (130,)}
    gen = torch.Generator(dev).manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(*sh, device=dev, generator=gen)) for sh in shapes.values()]
    names = list(shapes)
    opt = FlatAdamW(params, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, tensor_stats=D.TensorStats(every=1000), names=names)
    ts = opt.tensor_stats
    by_name = dict(zip(names, params))

    def backward():
        opt.grad.copy_(torch.randn(opt.grad.numel(), device=dev, generator=gen) * 0.1)
    backward()
    opt.step()
    assert float(opt.skipped()) == 0.0 and float(ts.computed()) == 0.0 and ts.culprits() == []        # every = 1000: not sampled
    backward()
    victim = "2.bias"
    by_name[victim].grad[7] = float("nan")
    before = [t.clone() for t in (opt.flat, opt.m, opt.v, opt.step_dev)]
    opt.step()
    assert float(opt.skipped()) == 1.0 and float(ts.computed()) == 1.0, "on_skip did not sample the skipped step"
    for x, y in zip(before, (opt.flat, opt.m, opt.v, opt.step_dev)):
        assert torch.equal(x, y), "a skipped step wrote"
    assert ts.culprits() == [victim]
    assert float(ts.view(victim, "grad_nonfinite")) == 1.0 and float(ts.view("<all>", "grad_nonfinite")) == 1.0
    assert all(float(ts.view(n, "grad_nonfinite")) == 0.0 and np.isfinite(float(ts.view(n, "grad_norm"))) for n in names if n != victim)
    rep = ts.report(top=1)
    assert rep[0]["name"] == victim and rep[0]["grad_norm"] != rep[0]["grad_norm"]                 # NaN sorts first
    backward()
    opt.step()
    assert float(opt.skipped()) == 1.0 and float(ts.computed()) == 0.0 and float(ts.age()) == 1.0
    ts.set_on_skip(False)
    backward()
    by_name["0.weight"].grad[0, 0] = float("inf")
    opt.step()
    assert float(opt.skipped()) == 2.0 and float(ts.computed()) == 0.0 and ts.culprits() == [victim]   # the table still holds the last sample
    opt.close()


def test_view_through_device_loss_meters_and_accumulation(pkg, dev):
    from vptr_amd.meters import DeviceLossMeters
    tr, c = _trainer(pkg, "far", dev, accum_steps=2, tensor_stats=D.TensorStats(every=2))
    ts = tr.opt.tensor_stats
    name = ts.names[0]
    meters = DeviceLossMeters(["gn0", "gn_all"], dev)
    seen = []
    for s in range(4):
        out = tr.step(*_batch(c, s, dev))
        seen.append((float(out["applied"]), float(ts.computed())))
        if s % 2 == 1:
            # a close: the slab holds the window's sum and the record's scale its 1 / accum_steps
            T.check_table(ts.table, _named_reference(tr, 0.5)[1], True, "close %d" % s)
            meters.update({"gn0": ts.view(name, "grad_norm"), "gn_all": ts.view(-1)})
            last = (float(ts.view(name)), float(ts.view(-1)))
    assert seen == [(0.0, 0.0), (1.0, 1.0), (0.0, 0.0), (1.0, 1.0)], seen
    res = meters.compute()
    assert res["gn0"]["count"] == 2 and res["gn0"]["last"] == last[0] and res["gn_all"]["last"] == last[1] and res["gn_all"]["nonfinite"] == 0


def test_limits_and_the_untouched_default(pkg, dev):
    from vptr_amd import ops
    from vptr_amd.train import AETrainer, FlatAdamW
    c = V.case("ae")
    enc, dec, _, disc = V.modules(pkg, c)
    with pytest.raises(ValueError, match="stage-1"):
        AETrainer(enc.to(dev), dec.to(dev), disc.to(dev), lam_gan=c["lam_gan"], tensor_stats=D.TensorStats())
    params = [torch.nn.Parameter(torch.ones(3, 4, device=dev)), torch.nn.Parameter(torch.zeros(3, device=dev))]
    for kw, match in ((dict(tensor_stats=True), "TensorStats"), (dict(tensor_stats=D.TensorStats(), names=["w"]), "1 names for 2"),
                      (dict(tensor_stats=D.TensorStats(), names=["w", "w"]), "twice"), (dict(names=["w", "b"]), "belongs to tensor_stats")):
        with pytest.raises(ValueError, match=match):
            FlatAdamW(params, **kw)
        assert params[0].grad is None, "a refused construction rebound the parameters"
    opt = FlatAdamW(params, tensor_stats=D.TensorStats(moments=False))
    ts = opt.tensor_stats
    assert ts.names == ["param_0", "param_1"] and ts.on_skip is False
    for call, match in ((lambda: ts.set_every(0), "every"), (lambda: ts.set_on_skip(True), "moments"), (lambda: ts.view("nope"), "no tensor named"),
                        (lambda: ts.view(0, "nope"), "no column"), (lambda: ts.view(9), "row"), (lambda: ts.report(sort="nope"), "no column")):
        with pytest.raises(ValueError, match=match):
            call()
    opt.grad.fill_(2.0)
    opt.step()
    assert float(ts.view(1, "grad_norm")) == pytest.approx(2.0 * 3 ** 0.5, rel=1e-6) and float(ts.view(1, "dir_rms")) == 0.0
    assert ts.report()[0]["update_ratio"] is None
    opt.close()
    ops.unregister_flat_slabs()
    tr, c = _trainer(pkg, "far", dev)
    assert tr.opt.ctl is None and tr.opt.tensor_stats is None
