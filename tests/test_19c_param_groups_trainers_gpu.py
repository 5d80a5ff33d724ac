"""Parameter groups on the trainers (`param_groups=` of NARTrainer / FARTrainer, `FlatAdamW.set_group` / `group_lr`), on the tiny fixtures
of tests/validation_cases.py in deterministic mode, set up as tests/test_17_optim_ctl_gpu.py does:

  * groups that all carry the defaults: three steps torch.equal to a twin with a constant schedule;
  * `no_decay_groups` plus a group at lr_scale 0.1 and one at lr_scale 0: after one step from a recorded state every parameter tensor
    against the fp64 AdamW update of the trainer's own gradient slab with its group's rate and decay; the lr_scale 0 group bit for bit;
  * capture: the node census is the controlled trainer's plus one kernel node; `set_group` between replays reaches the next replay;
  * with `accum_steps=2` and `ema_decay`: a hold writes nothing, default groups match the ungrouped trainer bit for bit;
  * `state_dict` into a torch.optim.AdamW built with the same grouping, one step on each side, at the bar of tests/test_10_resume_gpu.py;
  * AETrainer raises; without `param_groups` the optimizer has neither controls nor groups.

The per-tensor bar of the fp64 comparison.  p_new = fmaf(p, decay, -upd) rounds once: half an ulp of p_new.  upd = step_size * m / denom
carries the rounding of its own chain (a handful of ulp of upd) and the fp32 sum of squares behind the clip coefficient, whose two-pass
sum over 10^5 .. 10^6 elements stays within 2^-20 relative, so 2^-21 in the coefficient.  Per element:
|p_new - ref| <= 2^-23 |ref| + 2^-18 |upd|.  A wrong group shows: the decay alone moves p by lr * wd * |p| = 10^-6 |p| = 8 ulp."""
import numpy as np
import pytest
import torch

import validation_cases as V
from helpers import adamw_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
UPDATE_RTOL = 2e-3         # tests/test_10_resume_gpu.py: the two implementations' updates, relative to the size of the update


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
    from vptr_amd import ops
    from vptr_amd.train import FARTrainer, NARTrainer
    c = V.case(kind)
    enc, dec, T, _ = V.modules(pkg, c)
    ops.manual_seed(dev, 77)
    if kind == "nar":
        tr = NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=c["meta"]["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **ctl)
    else:
        tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, **ctl)
    return tr, c


def _batch(c, s, dev):
    past, fut = V.batch(c, s)
    return past.to(dev), fut.to(dev)


def _slabs(tr):
    o = tr.opt
    return [t.clone() for t in (o.flat, o.m, o.v, o.step_dev)] + ([o.ema.clone()] if o.ema is not None else [])


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: slab %d differs in %d elements" % (what, i, int((x != y).sum()))


def _default_groups(T):
    """three groups, all with the defaults: every third parameter listed in one entry, every third in another, the rest unlisted"""
    ps = [p for p in T.parameters() if p.requires_grad]
    return [{"params": ps[0::3]}, {"params": ps[1::3], "lr_scale": 1.0, "weight_decay": None}]


SLOW, STILL = "linear1.weight", "linear2.weight"


def _mixed_groups(T):
    """no_decay_groups' split, the first feed-forward matrices at a tenth of the rate, the second ones held still"""
    from vptr_amd.optim import no_decay_groups
    named = [(n, p) for n, p in T.named_parameters() if p.requires_grad]
    slow, still = [p for n, p in named if n.endswith(SLOW)], [p for n, p in named if n.endswith(STILL)]
    assert slow and still
    return no_decay_groups(T) + [{"params": slow, "lr_scale": 0.1}, {"params": still, "lr_scale": 0.0}]


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_default_groups_equal_the_controlled_trainer(pkg, dev, kind):
    from vptr_amd.optim import LRSchedule
    runs = []
    for ctl in (dict(schedule=LRSchedule()), dict(param_groups=_default_groups)):
        tr, c = _trainer(pkg, kind, dev, **ctl)
        outs = [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(3)]
        runs.append((outs, _slabs(tr), tr.opt.groups))
        del tr
    (oa, sa, ga), (ob, sb, gb) = runs
    assert ga is None and gb is not None and gb.ngroups == 3 and len(set(gb.gid.unique().tolist())) == 3
    _same(sa, sb, "groups with the defaults")
    assert float(sb[3]) == 3.0 and all(oa[s] == ob[s] for s in range(3)), (oa, ob)


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_mixed_groups_against_the_fp64_update_of_the_trainers_own_gradients(pkg, dev, kind):
    tr, c = _trainer(pkg, kind, dev, param_groups=_mixed_groups)
    opt = tr.opt
    assert opt.groups.ngroups == 4 and opt.groups.lr_scale == [1.0, 1.0, 0.1, 0.0] and [opt.groups.decay_of(g) for g in range(4)] == [0.01, 0.0, 0.01, 0.01]
    assert sorted(i for g in range(4) for i in opt.group_params(g)) == list(range(len(opt.params)))           # every parameter in exactly one group
    for s in range(2):
        tr.step(*_batch(c, s, dev))
    before = [[opt._logical(slab, i).detach().cpu().clone() for i in range(len(opt.params))] for slab in (opt.flat, opt.m, opt.v)]
    out = tr.step(*_batch(c, 2, dev))
    k = float(opt.step_dev)
    assert k == 3.0
    grads = [opt._logical(opt.grad, i).detach().cpu().clone() for i in range(len(opt.params))]
    sumsq = float(sum((g.double() ** 2).sum() for g in grads))
    assert abs(float(out["grad_norm"]) - sumsq ** 0.5) <= 4 * ULP * sumsq ** 0.5          # (the tiny fixtures' norm stays below the clip at 1.0)
    lr_now = f32(1e-4)
    assert float(out["lr"]) == lr_now
    names = {id(p): n for n, p in tr.T.named_parameters()}
    worst, moved = [], []
    for g in range(4):
        scale, wd = opt.groups.lr_scale[g], opt.groups.decay_of(g)
        assert float(opt.group_lr(g)) == f32(np.float32(lr_now) * np.float32(scale)), g
        for i in opt.group_params(g):
            p0, m0, v0 = (before[j][i] for j in range(3))
            ref = adamw_ref(p0, grads[i], m0, v0, k, lr_now * f32(scale), f32(opt.betas[0]), f32(opt.betas[1]), f32(opt.eps), f32(wd), sumsq=sumsq, max_norm=1.0,
                            abi_hyper=False)
            got = [opt._logical(slab, i).detach().cpu() for slab in (opt.flat, opt.m, opt.v)]
            name = names[id(opt.params[i])]
            if scale == 0.0:
                assert name.endswith(STILL) and torch.equal(got[0], p0), "%s (lr_scale 0) changed" % name
                assert not torch.equal(got[1], m0) and not torch.equal(got[2], v0), "%s: the moments of a group at lr_scale 0 stood still" % name
                continue
            upd = (ref[0] - p0.double() * (1.0 - lr_now * f32(scale) * f32(wd))).abs()
            err, bar = (got[0].double() - ref[0]).abs(), ULP * ref[0].abs() + 2.0 ** -18 * upd
            worst.append((float((err / bar.clamp_min(1e-300)).max()), name, g))
            assert bool((err <= bar).all()), "%s (group %d): %d of %d elements outside the bar, worst %.2f of it" % (name, g, int((err > bar).sum()), err.numel(), worst[-1][0])
            moved.append(not torch.equal(got[0], p0))       # (a tensor whose gradient vanishes analytically, in a group without decay, may stand still)
            for j, what in ((1, "m"), (2, "v")):
                assert float((got[j].double() - ref[j]).norm()) <= 4 * ULP * float(ref[j].norm()), (name, what)
    assert sum(moved) >= 0.8 * len(moved), (sum(moved), len(moved))
    worst.sort(reverse=True)
    print("%s mixed groups, worst tensors (error / bar, name, group): %r" % (kind, worst[:4]))
    exempt = [names[id(opt.params[i])] for i in opt.group_params(1)]
    assert any(n.endswith("bias") for n in exempt) and any("norm" in n and n.endswith("weight") for n in exempt)
    assert all(names[id(opt.params[i])].endswith(SLOW) for i in opt.group_params(2))


def test_capture_census_and_set_group_between_replays(pkg, dev):
    from vptr_amd.optim import LRSchedule
    tw, c = _trainer(pkg, "far", dev, schedule=LRSchedule())
    past, fut = _batch(c, 0, dev)
    tw.capture(past, fut, warmup=1)
    controlled = dict(tw.graph_nodes)
    del tw
    from vptr_amd import ops
    ops.unregister_flat_slabs()
    tr, c = _trainer(pkg, "far", dev, param_groups=_mixed_groups)
    tr.capture(past, fut, warmup=1)
    grouped = dict(tr.graph_nodes)
    print("census: controlled %r, grouped %r" % (controlled, grouped))
    assert grouped == dict(controlled, kernel=controlled["kernel"] + 1) and "memset" not in grouped
    ok, rep = tr.verify_graph(past, fut, steps=2)
    assert ok, rep
    opt = tr.opt
    slow, still, rest = (torch.from_numpy(np.isin(opt.groups.gid.cpu().numpy(), g)).to(dev) for g in ([2], [3], [0, 1]))
    p0 = opt.flat.clone()
    tr.step(past, fut)
    p1 = opt.flat.clone()
    assert torch.equal(p1[still], p0[still]) and not bool((p1[slow] == p0[slow]).all()) and not bool((p1[rest] == p0[rest]).all())
    lr_now = float(opt.lr_now())
    assert float(opt.group_lr(2)) == f32(np.float32(lr_now) * np.float32(0.1)) and float(opt.group_lr(3)) == 0.0
    opt.set_group(3, lr_scale=1.0)              # the held group moves from the next replay on, the slow one is held instead
    opt.set_group(2, lr_scale=0.0, weight_decay=0.5)
    tr.step(past, fut)
    p2 = opt.flat.clone()
    assert torch.equal(p2[slow], p1[slow]) and not bool((p2[still] == p1[still]).all()) and not bool((p2[rest] == p1[rest]).all())
    assert float(opt.group_lr(3)) == lr_now and float(opt.group_lr(2)) == 0.0
    opt.set_weight_decay(0.02)                  # group 0 inherits, group 1 (no decay) and group 2 (explicit) do not
    assert [opt.groups.decay_of(g) for g in range(4)] == [0.02, 0.0, 0.5, 0.02]
    tr.step(past, fut)
    assert torch.equal(opt.flat[slow], p1[slow]) and bool(torch.isfinite(opt.flat).all())


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_groups_with_accumulation_and_ema(pkg, dev, kind):
    runs = []
    for ctl in ({}, dict(param_groups=_default_groups), dict(param_groups=_mixed_groups)):
        tr, c = _trainer(pkg, kind, dev, accum_steps=2, ema_decay=0.9, **ctl)
        snaps, applied = [_slabs(tr)], []
        for s in range(4):
            applied.append(float(tr.step(*_batch(c, s, dev))["applied"]))
            snaps.append(_slabs(tr))
        assert applied == [0.0, 1.0, 0.0, 1.0]
        _same(snaps[1], snaps[0], "the first hold")
        _same(snaps[3], snaps[2], "the second hold")
        assert not torch.equal(snaps[2][0], snaps[1][0]) and not torch.equal(snaps[4][4], snaps[2][4]) and float(snaps[4][3]) == 2.0
        runs.append(snaps[4])
        if "param_groups" in ctl:
            assert float(tr.opt.group_lr(0)) == f32(1e-4)
        del tr
    _same(runs[1], runs[0], "default groups under accumulation and EMA")
    assert not torch.equal(runs[2][0], runs[0][0]) and not torch.equal(runs[2][4], runs[0][4])


def test_checkpoint_into_a_grouped_torch_adamw(pkg, dev):
    from vptr_amd.optim import SCALE_KEY
    tr, c = _trainer(pkg, "nar", dev, param_groups=_mixed_groups)
    opt = tr.opt
    for s in range(2):
        tr.step(*_batch(c, s, dev))
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 4 and [g[SCALE_KEY] for g in sd["param_groups"]] == [1.0, 1.0, 0.1, 0.0]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.01, 0.0, 0.01, 0.01] and [g["lr"] for g in sd["param_groups"]] == [1e-4, 1e-4, 1e-4 * 0.1, 0.0]
    assert [i for g in sd["param_groups"] for i in g["params"]] == list(range(len(opt.params)))
    # torch.optim.AdamW over plain clones, built with the same grouping
    clones = [torch.nn.Parameter(p.detach().clone().contiguous()) for p in opt.params]
    stock = torch.optim.AdamW([{"params": [clones[i] for i in opt.group_params(g)], "lr": 1e-4 * opt.groups.lr_scale[g], "weight_decay": opt.groups.decay_of(g)}
                               for g in range(4)], lr=1e-4)
    stock.load_state_dict(sd)
    before = [p.detach().clone() for p in clones]
    tr.step(*_batch(c, 2, dev))
    for q, p in zip(clones, opt.params):
        q.grad = p.grad.detach().clone().contiguous()
    torch.nn.utils.clip_grad_norm_(clones, 1.0)
    stock.step()

    def update_err(ours):
        num = sum(float((a.detach().double() - b.detach().double()).pow(2).sum()) for a, b in zip(ours, clones))
        den = sum(float((b.detach().double() - b0.double()).pow(2).sum()) for b, b0 in zip(clones, before))
        return (num / den) ** 0.5

    e = update_err(opt.params)
    print("third step after exporting the grouped state to torch.optim.AdamW: update differs by %.3e" % e)
    assert e < UPDATE_RTOL
    still = opt.group_params(3)
    assert all(torch.equal(clones[i], before[i]) and torch.equal(opt.params[i], before[i]) for i in still)
    # and back: the torch dict into a fresh grouped trainer, a fourth step on each side
    from vptr_amd import ops
    model = {k: v.detach().clone() for k, v in tr.T.state_dict().items()}
    ops.unregister_flat_slabs()
    tr2, _ = _trainer(pkg, "nar", dev, param_groups=_mixed_groups)
    tr2.T.load_state_dict(model)
    with torch.no_grad():
        for p, q in zip(tr2.opt.params, clones):
            p.copy_(q)
    back = stock.state_dict()
    for g in back["param_groups"]:
        g.pop(SCALE_KEY)
    tr2.opt.load_state_dict(back)
    assert float(tr2.opt.step_dev) == 3.0 and tr2.opt.groups.lr_scale[:2] == [1.0, 1.0] and tr2.opt.groups.lr_scale[3] == 0.0
    assert abs(tr2.opt.groups.lr_scale[2] - 0.1) <= 1e-15 and [tr2.opt.groups.decay_of(g) for g in range(4)] == [0.01, 0.0, 0.01, 0.01]
    before = [p.detach().clone() for p in clones]
    tr2.step(*_batch(c, 3, dev))
    for q, p in zip(clones, tr2.opt.params):
        q.grad = p.grad.detach().clone().contiguous()
    torch.nn.utils.clip_grad_norm_(clones, 1.0)
    stock.step()
    e = update_err(tr2.opt.params)
    print("fourth step after importing the grouped torch.optim.AdamW state: update differs by %.3e" % e)
    assert e < UPDATE_RTOL


def test_limits_and_the_untouched_default(pkg, dev):
    from vptr_amd.train import AETrainer
    c = V.case("ae")
    enc, dec, _, disc = V.modules(pkg, c)
    with pytest.raises(ValueError, match="stage-1"):
        AETrainer(enc.to(dev), dec.to(dev), disc.to(dev), lam_gan=c["lam_gan"], param_groups=[])
    with pytest.raises(ValueError, match="two|param_groups"):
        _trainer(pkg, "far", dev, param_groups=lambda T: [{"params": list(T.parameters())[:2]}, {"params": list(T.parameters())[1:3]}])
    from vptr_amd import ops
    ops.unregister_flat_slabs()
    tr, c = _trainer(pkg, "far", dev)
    assert tr.opt.ctl is None and tr.opt.groups is None
    out = tr.step(*_batch(c, 0, dev))
    assert "lr" not in out and "applied" not in out
    for call in (lambda: tr.opt.set_group(0, lr_scale=1.0), lambda: tr.opt.group_lr(0)):
        with pytest.raises(RuntimeError, match="param_groups"):
            call()
