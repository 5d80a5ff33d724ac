"""Gradient accumulation and EMA weights on the trainers (`accum_steps=`, `ema_decay=`, `ema_warmup=` of NARTrainer / FARTrainer), on the
tiny fixtures of tests/validation_cases.py in deterministic mode, set up as tests/test_17_optim_ctl_gpu.py does:

  * `accum_steps=1`: three steps torch.equal to a twin with a constant schedule;
  * `accum_steps=2`: four micro-steps against a twin driven by hand (zero-fill at window starts only, backward every call,
    `opt.step(grad_scale=0.5)` at closes only), `applied` = 0, 1, 0, 1;
  * capture with `accum_steps=2`: `verify_graph(steps=4)`, replays against eager micro-steps of a twin, `applied` per replay, no memset node;
  * an Inf pixel in the first micro-batch of a window with the skip on: slabs, step and EMA bit for bit, the next window applies; without
    the skip the slab turns non-finite;
  * `eval_step` between the micro-steps of a window changes nothing;
  * the EMA slab against the fp64 recursion over the recorded parameter slabs; `ema_weights()`, `eval_step(weights="ema")` against the
    oracle on `ema_state_dict()`, `predict(weights="ema")`, `step()` inside the context;
  * `state_dict` at a window boundary -> a fresh trainer -> the same next window, EMA included; torch.optim.AdamW loads the dict; a dict
    of an uncontrolled optimizer loads; a dict saved inside a window loads with the window dropped and one warning;
  * `disc=` / AETrainer with the new arguments raise; without them `opt.ctl is None`, `step` returns today's keys and the captured
    graph's node census is what it was;
  * the oracle's NARStep / FARStep driven by the test's own accumulation loop: accumulated gradient per parameter tensor, grad_norm, the
    loss terms of every micro-step, the parameters after two windows;
  * one child process on a one-rank RCCL group with the forced exchange: no all-reduce on holds, the usual ones on closes."""
import warnings

import pytest
import torch

import validation_cases as V
from test_02_model_gpu import TOL

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
PARAM_RTOL = 3e-4          # NARTrainer.verify_graph's param_rtol


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
    enc, dec, T, disc = V.modules(pkg, c)
    d = disc.to(dev) if disc is not None else None
    ops.manual_seed(dev, 77)
    if kind.startswith("nar"):
        tr = NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=c["meta"]["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, disc=d, lam_gan=c["lam_gan"], **ctl)
    else:
        tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, disc=d, lam_gan=c["lam_gan"], **ctl)
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


def _drive_by_hand(tw, k):
    """make a controlled twin accumulate by hand: zero-fill at window starts only, `opt.step(grad_scale=1 / k)` at closes only"""
    from vptr_amd import ops
    real_zero, real_step, pos = tw.opt.zero_grad, tw.opt.step, [0]

    def zero_grad():
        if pos[0] % k == 0:
            real_zero()
        else:
            ops.discard_wgrads()

    def step(grad_scale=1.0):
        pos[0] += 1
        if pos[0] % k == 0:
            real_step(grad_scale=grad_scale / k)

    tw.opt.zero_grad, tw.opt.step = zero_grad, step
    # what FlatAdamW does itself when it owns a window: tell ops.flush_wgrads that this slab carries partial sums from one backward pass to
    # the next, so that in deterministic mode every destination keeps one adder per launch (a twice-applied module: the NCE projector)
    tw.opt.grad._vptr_accumulates = True


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_accum_steps_1_equals_a_constant_schedule(pkg, dev, kind):
    from vptr_amd.optim import LRSchedule
    runs = []
    for ctl in (dict(schedule=LRSchedule()), dict(accum_steps=1)):
        tr, c = _trainer(pkg, kind, dev, **ctl)
        outs = [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(3)]
        runs.append((outs, _slabs(tr)))
        del tr
    (oa, sa), (ob, sb) = runs
    _same(sa, sb, "accum_steps=1")
    assert float(sb[3]) == 3.0 and all(ob[s]["applied"] == 1.0 and set(ob[s]) - set(oa[s]) == {"applied"} for s in range(3))
    assert all(oa[s][k] == ob[s][k] for s in range(3) for k in oa[s])


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_accum_steps_2_equals_a_twin_driven_by_hand(pkg, dev, kind):
    """The nar case is the one that needs ops.flush_wgrads' one-adder-per-launch rule of the deterministic mode: the NCE projector is
    applied twice per forward, and two problems of ONE grouped launch adding into a destination that already holds a partial sum
    differed run to run by one fp32 ulp in 155 .. 398 elements of its two weights (from a zero-filled slab a + b is order-independent,
    from a partial sum c the order of (c + a) + b shows)."""
    from vptr_amd.optim import LRSchedule
    tr, c = _trainer(pkg, kind, dev, accum_steps=2)
    outs = [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(4)]
    got = _slabs(tr)
    assert [o["applied"] for o in outs] == [0.0, 1.0, 0.0, 1.0] and float(tr.opt.micro()) == 0.0
    del tr
    tw, c = _trainer(pkg, kind, dev, schedule=LRSchedule())
    _drive_by_hand(tw, 2)
    ref = [{k: float(v) for k, v in tw.step(*_batch(c, s, dev)).items()} for s in range(4)]
    _same(got, _slabs(tw), "accum_steps=2")
    assert float(got[3]) == 2.0
    for s in range(4):
        for k in ("T_total", "T_MSE", "T_GDL"):
            assert outs[s][k] == ref[s][k], (s, k)
    for s in (1, 3):
        assert outs[s]["grad_norm"] == ref[s]["grad_norm"] and outs[s]["lr"] == ref[s]["lr"]


def test_capture_with_accum_steps_2(pkg, dev):
    tr, c = _trainer(pkg, "far", dev, accum_steps=2)
    past, fut = _batch(c, 0, dev)
    tr.capture(past, fut, warmup=2)
    assert "memset" not in tr.graph_nodes, tr.graph_nodes
    tr.opt.reset_window()
    ok, rep = tr.verify_graph(past, fut, steps=4)
    assert ok, rep
    assert tr.opt.ctl.micro_host == 0 and float(tr.opt.micro()) == 0.0
    step0 = float(tr.opt.step_dev)
    from vptr_amd import ops
    start = {"flat": tr.opt.flat.clone(), "m": tr.opt.m.clone(), "v": tr.opt.v.clone(), "step": tr.opt.step_dev.clone(),
             "seed": ops._master_seed(dev).clone()}
    applied, flats, lrs = [], [], []
    for s in range(4):
        if s == 2:
            tr.opt.set_lr(3e-4)                      # between the windows: the second close only
        out = tr.step(*_batch(c, s, dev))
        applied.append(float(out["applied"]))
        lrs.append(float(out["lr"]))
        flats.append(tr.opt.flat.clone())
    assert applied == [0.0, 1.0, 0.0, 1.0] and float(tr.opt.step_dev) == step0 + 2.0
    assert torch.equal(flats[0], start["flat"]) and torch.equal(flats[2], flats[1]) and not torch.equal(flats[1], flats[0])
    assert lrs[1] == lrs[2] and abs(lrs[3] - 3e-4) <= 3e-4 * ULP and abs(lrs[1] - 1e-4) <= 1e-4 * ULP
    # the same four micro-steps eagerly on a twin that starts from the state the replays started from
    tw, _ = _trainer(pkg, "far", dev, accum_steps=2)
    with torch.no_grad():
        tw.opt.flat.copy_(start["flat"]); tw.opt.m.copy_(start["m"]); tw.opt.v.copy_(start["v"]); tw.opt.step_dev.copy_(start["step"])
        ops._master_seed(dev).copy_(start["seed"])          # the dropout masks of the replays
    ops._seed_scope.pop(ops._dev_key(dev), None)
    if tw.opt.planes is not None:
        tw.opt.planes.refresh()
    for s in range(4):
        if s == 2:
            tw.opt.set_lr(3e-4)
        tw.step(*_batch(c, s, dev))
    pe, pg = tw.opt.flat.double(), flats[3].double()
    assert float((pe - pg).norm() / pe.norm()) <= PARAM_RTOL


def test_inf_pixel_first_in_its_window(pkg, dev):
    for skip in (True, False):
        tr, c = _trainer(pkg, "far", dev, accum_steps=2, ema_decay=0.9, skip_nonfinite=skip)
        for s in range(2):
            tr.step(*_batch(c, s, dev))
        before = _slabs(tr)
        past, fut = _batch(c, 2, dev)
        fut = fut.clone()
        fut[0, 0, 0, 0, 0] = float("inf")
        tr.step(past, fut)
        out = tr.step(*_batch(c, 3, dev))
        if skip:
            _same(_slabs(tr), before, "a skipped window")
            assert float(out["skipped"]) == 1.0 and float(out["applied"]) == 0.0 and float(tr.opt.micro()) == 0.0
            tr.step(*_batch(c, 4, dev))
            out = tr.step(*_batch(c, 5, dev))
            assert float(out["applied"]) == 1.0 and float(out["skipped"]) == 1.0 and float(tr.opt.step_dev) == 2.0
            assert not torch.equal(tr.opt.flat, before[0]) and bool(torch.isfinite(tr.opt.flat).all()) and bool(torch.isfinite(tr.opt.ema).all())
        else:
            assert not bool(torch.isfinite(tr.opt.flat).all())
        del tr


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_eval_step_inside_a_window_changes_nothing(pkg, dev, kind):
    runs = []
    for with_eval in (False, True):
        tr, c = _trainer(pkg, kind, dev, accum_steps=2)
        for s in range(4):
            tr.step(*_batch(c, s, dev))
            if with_eval and s % 2 == 0:
                tr.eval_step(*_batch(c, 7, dev))
        runs.append(_slabs(tr))
        del tr
    _same(runs[0], runs[1], "eval_step between micro-steps")


@pytest.mark.parametrize("warm", [False, True])
def test_ema_slab_and_ema_weights(pkg, dev, warm):
    from vptr_amd.optim import W_EMA_OMD
    tr, c = _trainer(pkg, "nar", dev, ema_decay=0.9, ema_warmup=warm)
    tw, _ = _trainer(pkg, "nar", dev, ema_decay=0.9, ema_warmup=warm)
    ema64, bound = tr.opt.flat.double().clone(), torch.zeros_like(tr.opt.flat, dtype=torch.float64)
    assert torch.equal(tr.opt.ema, tr.opt.flat)
    for s in range(3):
        tr.step(*_batch(c, s, dev))
        tw.step(*_batch(c, s, dev))
        omd, p = float(tr.opt.ctl.wword(W_EMA_OMD)), tr.opt.flat.double()
        want = 1.0 - (min(float(torch.tensor(0.9)), (1.0 + s) / (10.0 + s)) if warm else float(torch.tensor(0.9)))
        assert abs(omd - want) <= want * ULP, (s, omd, want)
        bound += ULP * (ema64.abs() + p.abs())
        ema64 = ema64 + omd * (p - ema64)
    err = (tr.opt.ema.double() - ema64).abs()
    print("EMA after 3 updates: worst error / bound %.3f" % float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), int((err > bound).sum())
    assert not torch.equal(tr.opt.ema, tr.opt.flat)
    # ema_state_dict: the transformer's keys, EMA values for parameters, buffers as they are
    esd, sd = tr.ema_state_dict(), tr.T.state_dict()
    assert list(esd) == list(sd)
    names = dict(tr.T.named_parameters())
    assert any(not torch.equal(esd[k], sd[k]) for k in names) and all(torch.equal(esd[k], sd[k]) for k in sd if k not in names)
    # inside the context the pass runs on the EMA: the oracle on ema_state_dict() at test_16's bar
    past, fut = _batch(c, 5, dev)
    raw = {k: float(v) for k, v in tr.eval_step(past, fut).items()}
    flat0, ema0 = tr.opt.flat.clone(), tr.opt.ema.clone()
    st = V.trainer_state(tr)
    st["T"] = {k: v.detach().cpu().clone() for k, v in esd.items()}
    ref = V.oracle_eval(c, st, past.cpu(), fut.cpu())
    with tr.ema_weights():
        assert torch.equal(tr.opt.flat, ema0) and torch.equal(tr.opt.ema, flat0)
        inside = {k: float(v) for k, v in tr.eval_step(past, fut).items()}
        pred_in = tr.predict(past).clone()
        with pytest.raises(RuntimeError, match="EMA"):
            tr.step(past, fut)
        with pytest.raises(RuntimeError, match="EMA"):
            tr.opt.state_dict()
    assert torch.equal(tr.opt.flat, flat0) and torch.equal(tr.opt.ema, ema0)
    for k in ref:
        assert abs(inside[k] - ref[k]) < TOL * abs(ref[k]) + 1e-6, (k, inside[k], ref[k])
    assert any(inside[k] != raw[k] for k in raw)
    assert {k: float(v) for k, v in tr.eval_step(past, fut, weights="ema").items()} == inside
    assert torch.equal(tr.predict(past, weights="ema"), pred_in) and not torch.equal(tr.predict(past), pred_in)
    with pytest.raises(RuntimeError):          # the context swaps back when its body raises
        with tr.ema_weights():
            raise RuntimeError("body")
    assert torch.equal(tr.opt.flat, flat0)
    # the next step equals a twin that never entered the context
    tr.step(*_batch(c, 3, dev))
    tw.step(*_batch(c, 3, dev))
    _same(_slabs(tr), _slabs(tw), "the step after ema_weights()")


def test_state_dict_round_trip(pkg, dev):
    from vptr_amd.optim import STATE_KEY
    tr, c = _trainer(pkg, "far", dev, accum_steps=2, ema_decay=0.9)
    for s in range(2):
        tr.step(*_batch(c, s, dev))
    sd, model = tr.opt.state_dict(), {k: v.clone() for k, v in tr.T.state_dict().items()}
    ctl = sd["param_groups"][0][STATE_KEY]
    assert {"accum_steps", "micro", "ema_decay", "ema_warmup", "ema_updates"} <= set(ctl) and ctl["micro"] == 0.0 and ctl["ema_updates"] == 1.0
    assert all("ema" in st for st in sd["state"].values())
    tr.step(*_batch(c, 2, dev))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mid = tr.opt.state_dict()
    assert mid["param_groups"][0][STATE_KEY]["micro"] == 1.0
    tr.step(*_batch(c, 3, dev))
    want = _slabs(tr)
    # the dict loads into torch.optim.AdamW
    stock = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in tr.opt.params], lr=1e-4)
    stock.load_state_dict(sd)
    assert STATE_KEY in stock.state_dict()["param_groups"][0]
    del tr
    # a fresh trainer, resumed at the window boundary: the next window is torch.equal, the EMA included.  The dropout seed is not part of
    # an optimizer's dict: the fresh trainer first takes the two steps the first run took (its slabs are then overwritten by the load)
    fresh, _ = _trainer(pkg, "far", dev, accum_steps=2, ema_decay=0.9)
    for s in range(2):
        fresh.step(*_batch(c, s, dev))
    fresh.T.load_state_dict(model)
    fresh.opt.load_state_dict(sd)
    for s in (2, 3):
        out = fresh.step(*_batch(c, s, dev))
    _same(_slabs(fresh), want, "resume at a window boundary")
    assert float(out["applied"]) == 1.0
    # a dict saved inside a window: the window is dropped, with one warning
    with pytest.warns(UserWarning, match="1 micro-batch") as rec:
        fresh.opt.load_state_dict(mid)
    assert len(rec) == 1 and float(fresh.opt.micro()) == 0.0 and fresh.opt.ctl.micro_host == 0
    # a dict of an uncontrolled optimizer loads: the EMA is seeded again from the parameters
    plain, _ = _trainer(pkg, "far", dev)
    assert plain.opt.ctl is None
    plain.step(*_batch(c, 0, dev))
    psd = plain.opt.state_dict()
    assert STATE_KEY not in psd["param_groups"][0] and "ema" not in psd["state"][0]
    fresh.opt.load_state_dict(psd)
    assert torch.equal(fresh.opt.ema, fresh.opt.flat) and float(fresh.opt.step_dev) == 1.0 and fresh.opt.accum_steps == 2


def test_limits_and_the_untouched_default(pkg, dev):
    from vptr_amd.train import AETrainer
    for ctl in (dict(accum_steps=2), dict(ema_decay=0.9)):
        with pytest.raises(ValueError, match="adversarial"):
            _trainer(pkg, "nar_gan", dev, **ctl)
        c = V.case("ae")
        enc, dec, _, disc = V.modules(pkg, c)
        with pytest.raises(ValueError, match="stage-1"):
            AETrainer(enc.to(dev), dec.to(dev), disc.to(dev), lam_gan=c["lam_gan"], **ctl)
    tr, c = _trainer(pkg, "far", dev)
    assert tr.opt.ctl is None and tr.opt.ema is None
    out = tr.step(*_batch(c, 0, dev))
    assert "applied" not in out
    with pytest.raises(RuntimeError):
        tr.opt.reset_window()
    with pytest.raises(RuntimeError):
        tr.ema_weights().__enter__()


def test_default_trainer_graph_census_is_unchanged(pkg, dev, monkeypatch):
    """Without the new arguments the captured step holds the nodes it held before: the census of a default NAR trainer (deterministic
    mode, the NCE projector applied twice) equals that of the same trainer captured with the split of repeated destinations taken out
    of ops.flush_wgrads / flush_partial_reduces, i.e. with the flush as it was.  With accum_steps=1 the split is active: the stated
    census change is extra kernel nodes (the later occurrences' launches), and still no memset node."""
    from vptr_amd.ops import wgrad

    def census(patched, **ctl):
        if patched:
            monkeypatch.setattr(wgrad, "_split_repeats", lambda items, key: ([], items))
        tr, c = _trainer(pkg, "nar", dev, **ctl)
        tr.capture(*_batch(c, 0, dev), warmup=2)
        monkeypatch.undo()
        nodes = dict(tr.graph_nodes)
        del tr
        return nodes

    plain, old = census(False), census(True)
    assert plain == old and "memset" not in plain, (plain, old)
    windowed, windowed_old = census(False, accum_steps=1), census(True, accum_steps=1)
    print("census: default %r, accum_steps=1 %r, accum_steps=1 without the split %r" % (plain, windowed, windowed_old))
    assert "memset" not in windowed and windowed["kernel"] > windowed_old["kernel"], (plain, windowed, windowed_old)


# ---- independent of the kernels' own accumulate semantics: the oracle driven by the test's own accumulation loop -------------------------
GRAD_RTOL = 2e-3     # test_02's bar on grad_norm, here per parameter tensor (rel-L2)
GRAD_FLOOR = 1e-4    # ... plus this share of the GLOBAL gradient norm: a tensor whose own norm is far below the slab's (biases in front of a
#                      normalisation: analytically zero) holds rounding noise of the large terms that cancel in it, not of its own size


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_accumulated_gradients_against_the_oracles_own_loop(pkg, dev, kind):
    """k = 2 over the distinct micro-batches V.batch(c, 0 .. 3), two windows.  The oracle's NARStep / FARStep with THIS test's loop --
    forward_losses, (loss / k).backward() per micro-batch, clip_grad_norm_, AdamW.step() -- against the trainer: the accumulated gradient
    per parameter tensor before the first close, grad_norm of both closes, the loss terms of every micro-step, the parameters after the
    two windows.  Bars of tests/test_02_model_gpu.py on its tiny 2-step records: loss terms TOL |ref| + 1e-6, grad_norm 2e-3, parameters
    helpers.post_step_params_close's (global rel-L2 1e-4, at most 2 % of the updates off by more than lr / 2); the per-tensor gradients at
    grad_norm's bar plus GRAD_FLOOR of the global norm.  A slab writer that overwrote instead of adding would lose the first micro-batch's
    half of ITS tensors' gradient: a relative error of order 1 there, whatever the other families do."""
    from oracle import vptr_oracle as O
    k, lr = 2, 1e-4
    tr, c = _trainer(pkg, kind, dev, accum_steps=k)
    st0 = V.trainer_state(tr)
    if kind == "nar":
        st = O.NARStep(st0["enc"], st0["dec"], st0["T"], c["cfg"], out_layer=c["meta"].get("out_layer", "Tanh"), lr=lr)
        names = ("T_total", "T_GDL", "T_MSE", "T_bpc")
    else:
        st = O.FARStep(st0["enc"], st0["dec"], st0["T"], c["cfg"], out_layer=c["meta"].get("out_layer", "Tanh"), lr=lr)
        names = ("T_total", "T_GDL", "T_MSE")
    params = dict(tr.T.named_parameters())
    for w in range(2):
        for p in st.params_T:
            p.grad = None
        for v in st.P_dec.values():
            if v.requires_grad:
                v.grad = None
        for j in range(k):
            s = w * k + j
            past, fut = V.batch(c, s)
            res = st.forward_losses(past, fut)
            (res[0] / k).backward()
            out = tr.step(past.to(dev), fut.to(dev))
            for name, ref in zip(names, res):
                ref = float(ref.detach())
                print("%s micro-step %d %s: %.7g (oracle %.7g)" % (kind, s, name, float(out[name]), ref))
                assert abs(float(out[name]) - ref) < TOL * abs(ref) + 1e-6, (s, name, float(out[name]), ref)
            assert float(out["applied"]) == float(j == k - 1)
        if w == 0:
            # the slab still holds the window's raw sum after the close (the update reads it, scaled by 1 / k, and leaves it)
            ref_g = {n: st.P_T[n].grad.detach().double() for n in params}
            glob = float(torch.sqrt(sum((g * g).sum() for g in ref_g.values())))
            worst = []
            for n, p in params.items():
                got = p.grad.detach().cpu().double() / k
                err, bar = float((got - ref_g[n]).norm()), GRAD_RTOL * float(ref_g[n].norm()) + GRAD_FLOOR * glob
                worst.append((err / bar, n, err, float(ref_g[n].norm())))
            worst.sort(reverse=True)
            print("%s accumulated gradient, worst tensors (error / bar, name, error, |ref|): %r; global norm %.4g" % (kind, worst[:5], glob))
            assert worst[0][0] <= 1.0, worst[:8]
        gn = float(torch.nn.utils.clip_grad_norm_(st.params_T, st.max_grad_norm))
        st.opt.step()
        print("%s window %d grad_norm %.7g (oracle %.7g)" % (kind, w, float(out["grad_norm"]), gn))
        assert abs(float(out["grad_norm"]) - gn) < 2e-3 * gn, (w, float(out["grad_norm"]), gn)
    # helpers.post_step_params_close's rule on the oracle's parameters
    num = den = 0.0
    bad = tot = 0
    for n, p in params.items():
        r = st.P_T[n].detach().double()
        d = p.detach().cpu().double() - r
        num, den = num + float((d * d).sum()), den + float((r * r).sum())
        bad, tot = bad + int((d.abs() > 0.5 * lr).sum()), tot + d.numel()
    print("%s parameters after two windows: rel-L2 %.3e, %d of %d updates off by more than lr / 2" % (kind, (num / den) ** 0.5, bad, tot))
    assert (num / den) ** 0.5 < 1e-4 and bad <= 0.02 * tot, ((num / den) ** 0.5, bad, tot)


# ---- data parallel: holds exchange nothing -----------------------------------------------------------------------------------------------
_DP_CHILD = r'''
import json, os, sys
ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], RANK="0", WORLD_SIZE="1", VPTR_FUSED_STATS="0")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch
import torch.distributed as dist
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
res = {}
try:
    import validation_cases as V
    import vptr_amd.model as pkg
    from vptr_amd import ops
    from vptr_amd.train import FARTrainer
    ops.set_deterministic(True)
    c = V.case("far")

    def run(mode):
        """mode: none (no process group), eager (forced exchange), front (capture_front, forced exchange)"""
        os.environ["VPTR_DP_FORCE_EXCHANGE"] = "0" if mode == "none" else "1"
        ops.unregister_flat_slabs()
        enc, dec, T, _ = V.modules(pkg, c)
        ops.manual_seed(dev, 77)
        tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, accum_steps=2,
                        process_group=None if mode == "none" else dist.group.WORLD)
        batches = [tuple(t.to(dev) for t in V.batch(c, s)) for s in range(4)]
        if mode == "front":
            tr.capture_front(*batches[0], warmup=2)
            tr.opt.reset_window()
        tr.comm_stats = {}
        step0 = float(tr.opt.step_dev)
        calls, nbytes, applied, scales = [], [], [], []
        for past, fut in batches:
            c0, b0 = tr.comm_stats.get("calls", 0), tr.comm_stats.get("bytes", 0)
            out = tr.step(past, fut)
            applied.append(float(out["applied"]))
            calls.append(tr.comm_stats.get("calls", 0) - c0)
            nbytes.append(tr.comm_stats.get("bytes", 0) - b0)
            scales.append(tr._grad_scale)
        slabs = [t.detach().clone() for t in (tr.opt.flat, tr.opt.m, tr.opt.v, tr.opt.step_dev)]
        return dict(calls=calls, bytes=nbytes, applied=applied, scales=scales, mirror=tr.opt.ctl.micro_host, slab_bytes=tr.opt.grad.numel() * 4,
                    updates=float(tr.opt.step_dev) - step0), slabs

    res["none"], s_none = run("none")
    res["eager"], s_eager = run("eager")
    res["eager_equal"] = [bool(torch.equal(a, b)) for a, b in zip(s_eager, s_none)]
    res["front"], s_front = run("front")
except Exception as e:
    import traceback
    res = {"error": "%s\n%s" % (e, traceback.format_exc()[-2000:])}
finally:
    dist.destroy_process_group()
print("RESULT " + json.dumps(res))
'''


def test_data_parallel_holds_exchange_nothing():
    """One child process with a one-rank RCCL group and the forced exchange (set up as tests/test_22_rccl_gpu.py does), the tiny FAR
    model with accum_steps=2, two windows, deterministic mode: zero all-reduce calls and bytes on the holds, the usual ones on the closes
    (eagerly and behind a `capture_front` graph); after the two windows the slabs equal those of the same run without a process group."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-c", _DP_CHILD, root, str(port)], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])        # before anything else runs
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][7:])
    assert "error" not in res, res["error"]
    print(res)
    assert res["none"]["calls"] == [0, 0, 0, 0] and res["none"]["applied"] == [0.0, 1.0, 0.0, 1.0]
    for mode in ("eager", "front"):
        m = res[mode]
        assert m["applied"] == [0.0, 1.0, 0.0, 1.0] and m["mirror"] == 0, (mode, m)
        assert m["calls"][0] == m["calls"][2] == 0 and m["bytes"][0] == m["bytes"][2] == 0, (mode, m)
        assert m["calls"][1] >= 1 and m["calls"][1] == m["calls"][3] and m["bytes"][1] == m["bytes"][3] == m["slab_bytes"], (mode, m)
        assert m["scales"] == [1.0] * 4                                                   # 1 / world; the 1 / k is the optimizer's
    assert all(res["eager_equal"]), res["eager_equal"]
    assert res["none"]["updates"] == res["eager"]["updates"] == res["front"]["updates"] == 2.0
