"""Device-resident optimizer controls on the trainers (`schedule=`, `skip_nonfinite=` of NARTrainer / FARTrainer / AETrainer), on the tiny
fixtures of tests/validation_cases.py:

  * a constant `LRSchedule` leaves three steps torch.equal to an uncontrolled twin (deterministic mode, set up as tests/test_11 does);
  * a cosine schedule: the returned rate equals the host mirror within one fp32 ulp, and the parameters match a twin stepped eagerly with
    `opt.lr` set by hand before each step, at `verify_graph`'s `param_rtol`;
  * `capture()` with a schedule: `verify_graph` passes, the rate follows the schedule per replay, `set_lr` between replays changes the next
    update -- and WITHOUT controls the same assignment after `capture()` changes nothing (today's behaviour, the gap the controls close);
  * a batch with an Inf pixel: with `skip_nonfinite=True` slab, moments and step stay bit for bit, the step is counted, the meters show the
    non-finite term, the next good step succeeds; with `skip_nonfinite=False` the slab turns non-finite;
  * `state_dict` -> a fresh trainer -> the same next step; the dict still loads into torch.optim.AdamW, and an uncontrolled dict loads into
    a controlled optimizer."""
import math

import numpy as np
import pytest
import torch

import validation_cases as V

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
PARAM_RTOL = 3e-4          # NARTrainer.verify_graph's param_rtol
KINDS = ("nar", "far", "nar_gan", "ae")


def f32(x):
    return float(np.float32(x))


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
    """the trainer of validation_cases.trainer with the controls' arguments; the dropout seed is reset, so two trainers built by this see
    the same masks step for step"""
    from vptr_amd import ops
    from vptr_amd.train import AETrainer, FARTrainer, NARTrainer
    c = V.case(kind)
    enc, dec, T, disc = V.modules(pkg, c)
    meta = c["meta"]
    d = disc.to(dev) if disc is not None else None
    ops.manual_seed(dev, 77)
    if kind == "ae":
        tr = AETrainer(enc.to(dev), dec.to(dev), d, lr=2e-4, lam_gan=c["lam_gan"], **ctl)
    elif kind.startswith("nar"):
        tr = NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=meta["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, disc=d, lam_gan=c["lam_gan"], **ctl)
    else:
        tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, disc=d, lam_gan=c["lam_gan"], **ctl)
    return tr, c


def _opts(tr):
    """the trainer's optimizers, the generator's first"""
    if hasattr(tr, "opt_G"):
        return [tr.opt_G, tr.opt_D]
    return [tr.opt] + ([tr.opt_D] if tr.disc is not None else [])


def _batch(c, s, dev):
    past, fut = V.batch(c, s)
    return past.to(dev), fut.to(dev)


def _slabs(tr):
    return [t.clone() for o in _opts(tr) for t in (o.flat, o.m, o.v, o.step_dev)]


def _lr_keys(kind):
    return ("lr_G", "lr_D") if kind == "ae" else ("lr",)


@pytest.mark.parametrize("kind", KINDS)
def test_constant_schedule_equals_the_uncontrolled_trainer(pkg, dev, kind):
    """Three steps of a trainer with a constant schedule against an uncontrolled twin, torch.equal on parameters, moments and step count.
    `nar_gan` and `ae` need the deterministic mode to cover the discriminator and the stage-1 step (convolution weight gradients without
    K-splits, single-adder 7x7 weight / bias gradients: ops.set_deterministic); without that two UNCONTROLLED trainers differ run to run."""
    from vptr_amd.optim import LRSchedule
    runs = []
    for ctl in ({}, dict(schedule=LRSchedule())):
        tr, c = _trainer(pkg, kind, dev, **ctl)
        outs = [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(3)]
        runs.append((outs, _slabs(tr)))
        assert all((o.ctl is not None) == bool(ctl) for o in _opts(tr))
        del tr
    (oa, sa), (ob, sb) = runs
    for s in range(3):
        print("%s step %d terms that differ (uncontrolled, constant schedule): %r" % (kind, s, {k: (oa[s][k], ob[s][k]) for k in oa[s] if oa[s][k] != ob[s][k]}))
    print("%s slabs equal: %r" % (kind, [torch.equal(a, b) for a, b in zip(sa, sb)]))
    for s in range(3):
        assert all(oa[s][k] == ob[s][k] for k in oa[s]), (s, {k: (oa[s][k], ob[s][k]) for k in oa[s] if oa[s][k] != ob[s][k]})
        assert set(ob[s]) - set(oa[s]) <= {"lr", "skipped", "skipped_D", "lr_G", "lr_D", "skipped_G"} and set(_lr_keys(kind)) <= set(ob[s])
    for a, b in zip(sa, sb):
        assert torch.equal(a, b), "a constant schedule changed the trajectory"
    assert float(sa[3]) == 3.0


@pytest.mark.parametrize("kind", ["nar_gan", "ae"])
def test_constant_schedule_update_equals_uncontrolled_on_the_same_gradients(pkg, dev, kind):
    """independent of the reproducibility of forward / backward: every optimizer step of a controlled trainer is repeated by an
    uncontrolled FlatAdamW from the same pre-step slabs and the same gradient slab; parameters, moments and step count must agree bit for bit"""
    from vptr_amd.optim import LRSchedule
    from vptr_amd.train import FlatAdamW
    tr, c = _trainer(pkg, kind, dev, schedule=LRSchedule())
    checked = []

    def shadowed(o):
        shadow = FlatAdamW([torch.nn.Parameter(torch.zeros(o.flat.numel(), device=dev))], lr=o.lr, betas=o.betas, eps=o.eps, weight_decay=o.weight_decay,
                           max_grad_norm=o.max_grad_norm)
        assert shadow.ctl is None and shadow.flat.numel() == o.flat.numel()
        real = o.step

        def step(grad_scale=1.0):
            with torch.no_grad():
                for dst, src in ((shadow.flat, o.flat), (shadow.m, o.m), (shadow.v, o.v), (shadow.step_dev, o.step_dev), (shadow.grad, o.grad)):
                    dst.copy_(src)
            real(grad_scale)
            shadow.step(grad_scale)
            checked.append(all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                               for a, b in ((shadow.flat, o.flat), (shadow.m, o.m), (shadow.v, o.v), (shadow.step_dev, o.step_dev))))
        o.step = step

    for o in _opts(tr):
        shadowed(o)
    for s in range(3):
        tr.step(*_batch(c, s, dev))
    assert len(checked) == 6 and all(checked), checked


@pytest.mark.parametrize("kind", KINDS)
def test_cosine_schedule_equals_lr_set_by_hand(pkg, dev, kind):
    from vptr_amd.optim import LRSchedule
    # four steps: factors 1 (warm-up), 1 (t = 0), 0.7 (t = 1 / 3), 0.325 (t = 2 / 3)
    sched = LRSchedule("cosine", warmup_steps=1, total_steps=4, min_ratio=0.1)
    tr, c = _trainer(pkg, kind, dev, schedule=sched)
    base = f32(_opts(tr)[0].lr)
    for s in range(4):
        out = tr.step(*_batch(c, s, dev))
        want = base * sched.factor(s)
        for k in _lr_keys(kind):
            assert abs(float(out[k]) - want) <= want * ULP, (s, k, float(out[k]), want)
    got = _slabs(tr)
    del tr
    twin, c = _trainer(pkg, kind, dev)
    for s in range(4):
        for o in _opts(twin):
            o.lr = base * sched.factor(s)
        twin.step(*_batch(c, s, dev))
    want = _slabs(twin)
    for i in range(0, len(got), 4):
        d = float((got[i].double() - want[i].double()).norm() / want[i].double().norm())
        print("cosine %s slab %d: rel-L2 to the hand-set twin %.3e (bar %.1e)" % (kind, i // 4, d, PARAM_RTOL))
        assert d <= PARAM_RTOL, (kind, i, d)
    assert abs(sched.factor(3) - 0.325) < 1e-7          # the schedule did something inside the compared steps


def test_capture_with_a_schedule(pkg, dev):
    from vptr_amd.optim import LRSchedule
    sched = LRSchedule("linear", warmup_steps=2, total_steps=40, min_ratio=0.1)
    tr, c = _trainer(pkg, "nar", dev, schedule=sched)
    past, fut = _batch(c, 0, dev)
    tr.capture(past, fut, warmup=1)
    assert set(tr.graph_nodes) <= {"kernel", "memcpy", "empty"}
    ok, rep = tr.verify_graph(past, fut, steps=2)
    assert ok, rep
    base, k0 = f32(tr.opt.lr), int(float(tr.opt.step_dev))
    for i in range(3):
        out = tr.step(past, fut)
        want = base * sched.factor(k0 + i)
        assert abs(float(out["lr"]) - want) <= want * ULP, (i, float(out["lr"]), want)
        assert float(tr.opt.step_dev) == k0 + i + 1
    # set_lr between replays: a rate of 0 (and the decay 1 - 0 * wd = 1) leaves the parameters where they are, the moments still move
    before = tr.opt.flat.clone()
    tr.opt.set_lr(0.0)
    out = tr.step(past, fut)
    assert float(out["lr"]) == 0.0 and torch.equal(tr.opt.flat, before)
    tr.opt.lr = 1e-4                                                    # the attribute routes to set_lr
    out = tr.step(past, fut)
    want = f32(1e-4) * sched.factor(k0 + 4)
    assert abs(float(out["lr"]) - want) <= want * ULP and not torch.equal(tr.opt.flat, before)


def test_without_controls_a_captured_step_ignores_lr(pkg, dev):
    """today's behaviour, pinned: after capture() the rate is frozen into the kernel node; assigning `opt.lr` changes an attribute only"""
    tr, c = _trainer(pkg, "nar", dev)
    past, fut = _batch(c, 0, dev)
    tr.capture(past, fut, warmup=1)
    snap = tr._snapshot()
    tr.step(past, fut)
    moved = tr.opt.flat.clone()
    tr._restore(snap)
    tr.opt.lr = 0.0
    tr.step(past, fut)
    assert torch.equal(tr.opt.flat, moved) and not torch.equal(moved, snap["flat"])
    with pytest.raises(RuntimeError):
        tr.opt.set_lr(0.0)


@pytest.mark.parametrize("kind", ["nar", "ae"])
def test_nonfinite_batch_is_skipped(pkg, dev, kind):
    from vptr_amd.meters import DeviceLossMeters
    tr, c = _trainer(pkg, kind, dev, skip_nonfinite=True)
    names = ["AE_total", "AEgan", "AE_MSE", "AE_GDL", "Dtotal", "Dfake", "Dreal"] if kind == "ae" else ["T_total", "T_MSE", "T_GDL", "T_bpc"]
    meters = DeviceLossMeters(names, dev)          # the controls' keys ("lr", "skipped", ...) are ignored by default, like grad_norm
    tr.step(*_batch(c, 0, dev), meters=meters)
    before = _slabs(tr)
    past, fut = _batch(c, 1, dev)
    fut[0, 0, 0, 0, 0] = float("inf")
    out = tr.step(past, fut, meters=meters)
    for k in ("skipped_G", "skipped_D") if kind == "ae" else ("skipped",):
        assert float(out[k]) == 1.0, (k, float(out[k]))
    for a, b in zip(before, _slabs(tr)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a skipped step changed parameters, moments or the step count"
    assert all(float(o.skipped_in_a_row()) == 1.0 for o in _opts(tr))
    res = meters.compute()
    assert res[names[0]]["nonfinite"] == 1 and res[names[0]]["count"] == 2
    out = tr.step(*_batch(c, 2, dev), meters=meters)
    after = _slabs(tr)
    assert all(bool(torch.isfinite(t).all()) for t in after) and not torch.equal(after[0], before[0])
    assert float(after[3]) == 2.0 and all(float(o.skipped()) == 1.0 and float(o.skipped_in_a_row()) == 0.0 for o in _opts(tr))
    assert math.isfinite(float(out["grad_norm"] if kind != "ae" else out["AE_total"]))


def test_nonfinite_batch_without_the_skip_poisons_the_slab(pkg, dev):
    from vptr_amd.optim import LRSchedule
    tr, c = _trainer(pkg, "nar", dev, schedule=LRSchedule())
    past, fut = _batch(c, 1, dev)
    fut[0, 0, 0, 0, 0] = float("inf")
    out = tr.step(past, fut)
    assert float(out["skipped"]) == 0.0 and float(tr.opt.step_dev) == 1.0
    assert not bool(torch.isfinite(tr.opt.flat).all())


def test_state_dict_round_trips(pkg, dev):
    from vptr_amd import ops
    from vptr_amd.optim import STATE_KEY, LRSchedule
    sched = LRSchedule("cosine", warmup_steps=1, total_steps=6, min_ratio=0.1)
    tr, c = _trainer(pkg, "nar", dev, schedule=sched, skip_nonfinite=True)
    past, fut = _batch(c, 1, dev)
    tr.step(*_batch(c, 0, dev))
    bad = fut.clone()
    bad[0, 0, 0, 0, 0] = float("inf")
    tr.step(past, bad)                                                  # one skipped step: the counters have something to carry
    sd = tr.opt.state_dict()
    saved = sd["param_groups"][0][STATE_KEY]
    assert saved == {"schedule": sched.to_dict(), "skip_nonfinite": True, "skipped_total": 1.0, "skipped_in_a_row": 1.0}
    weights = {k: v.clone() for k, v in tr.T.state_dict().items()}
    ops.manual_seed(dev, 5)
    out_a = {k: float(v) for k, v in tr.step(past, fut).items()}
    flat_a = tr.opt.flat.clone()
    # a fresh trainer built with ANOTHER schedule and no skip: the checkpoint brings its own
    tr2, _ = _trainer(pkg, "nar", dev, schedule=LRSchedule("linear", 0, 3, 0.5))
    tr2.T.load_state_dict(weights)
    tr2.opt.load_state_dict(sd)
    assert tr2.opt.schedule == sched and tr2.opt.ctl.skip_nonfinite and float(tr2.opt.skipped()) == 1.0 and float(tr2.opt.step_dev) == 1.0
    ops.manual_seed(dev, 5)
    out_b = {k: float(v) for k, v in tr2.step(past, fut).items()}
    assert out_a == out_b and torch.equal(flat_a, tr2.opt.flat)
    assert float(tr2.opt.skipped_in_a_row()) == 0.0
    # the controlled dict still loads into torch.optim.AdamW (an unknown group key is carried along) ...
    plain = [torch.nn.Parameter(p.detach().clone()) for p in tr.T.parameters() if p.requires_grad]
    topt = torch.optim.AdamW(plain, lr=1e-4)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == 1e-4 and float(topt.state[plain[0]]["step"]) == 1.0
    # ... and an uncontrolled dict loads into a controlled optimizer, whose own controls stay
    tr3, _ = _trainer(pkg, "nar", dev)
    tr3.step(*_batch(c, 0, dev))
    sd3 = tr3.opt.state_dict()
    assert STATE_KEY not in sd3["param_groups"][0] and set(sd3["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach",
                                                                                      "capturable", "differentiable", "fused", "params"}
    tr2.opt.load_state_dict(sd3)
    assert tr2.opt.schedule == sched and float(tr2.opt.step_dev) == 1.0 and float(tr2.opt.skipped()) == 1.0
