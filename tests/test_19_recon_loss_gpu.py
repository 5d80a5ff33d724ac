"""`recon=ReconLoss(...)` on the trainers, on the tiny fixtures of tests/validation_cases.py in deterministic mode:

  * `recon=ReconLoss()` (all defaults): three NAR and three FAR steps bit-identical to `recon=None` -- loss terms and every optimizer slab;
  * "l1" + alpha 2 + "exp" weights, and "mse+l1" + alpha 1.5 + distinct GDL weights, against a twin whose `_loss_terms` is overridden here
    with the torch criterion classes (NAR, FAR; AETrainer: the second setting without weights, through its `_ae_recon`): loss terms after
    one and after two steps at the loss-term bar of tests/test_16_validation_gpu.py (TOL |ref| + 1e-6), parameters after two steps at
    verify_graph's param_rtol (3e-4, the PARAM_RTOL of tests/test_18_accum_ema_gpu.py; test_16 itself compares no parameters);
  * `eval_step` returns the new key and leaves the trajectory bit-identical;
  * `capture`: the default trainer's kernel count, no memset node, `verify_graph`;
  * `set_temporal_weight` between two replays against an eager twin constructed with the new weights;
  * `DeviceLossMeters` with "T_L1" named;
  * ValueError: temporal weights on AETrainer, a wrong length at the first step, alpha < 1."""
import pytest
import torch

import validation_cases as V
from test_02_model_gpu import TOL

pytestmark = pytest.mark.gpu

PARAM_RTOL = 3e-4          # NARTrainer.verify_graph's param_rtol
GRAPH_RTOL = 2e-3          # NARTrainer.verify_graph's rtol


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


def _trainer(pkg, kind, dev, **kw):
    from vptr_amd import ops
    from vptr_amd.train import AETrainer, FARTrainer, NARTrainer
    c = V.case(kind)
    enc, dec, T, disc = V.modules(pkg, c)
    ops.manual_seed(dev, 77)
    if kind == "ae":
        tr = AETrainer(enc.to(dev), dec.to(dev), disc.to(dev), lr=2e-4, lam_gan=c["lam_gan"], **kw)
    elif kind == "nar":
        tr = NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=c["meta"]["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **kw)
    else:
        tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, **kw)
    return tr, c


def _batch(c, s, dev):
    past, fut = V.batch(c, s)
    return past.to(dev), fut.to(dev)


def _loss_T(c):
    """the number of time indices the recipe's frame loss sees"""
    cfg = c["cfg"]
    return cfg["Tf"] if c["kind"] == "nar" else cfg["Tp"] - 1 + cfg["Tf"]


def _opts(tr):
    return [o for o in (getattr(tr, "opt", None), getattr(tr, "opt_G", None), getattr(tr, "opt_D", None)) if o is not None]


def _slabs(tr):
    return [t.clone() for o in _opts(tr) for t in (o.flat, o.m, o.v, o.step_dev)]


def _floats(out):
    return {k: float(v) for k, v in out.items()}


def _settings(c):
    """id -> (ReconLoss arguments, (w_point, w_gdl) CPU vectors or None)"""
    from vptr_amd.model.criterion import temporal_weight_func
    T = _loss_T(c) if c["kind"] != "ae" else None
    if T is None:
        return {"msel1_a1.5": (dict(point="mse+l1", gdl_alpha=1.5), (None, None))}
    exp = temporal_weight_func(T).float()
    wg = torch.linspace(1.5, 0.0, T)                               # distinct GDL weights, the last frame's is 0
    return {"l1_a2_exp": (dict(point="l1", gdl_alpha=2.0, temporal_weight="exp"), (exp, exp)),
            "msel1_a1.5": (dict(point="mse+l1", gdl_alpha=1.5, temporal_weight=exp * 0.5, gdl_temporal_weight=wg), (exp * 0.5, wg))}


def _torch_twin(tw, kind, args, w):
    """override the twin's loss with the criterion classes of vptr_amd.model.criterion (ATen kernels, eager only)"""
    from vptr_amd import ops
    from vptr_amd.model.criterion import GDL, L1Loss, MSELoss
    dev = _opts(tw)[0].flat.device
    wp, wg = (None if t is None else t.to(dev) for t in w)
    alpha = args["gdl_alpha"]
    mse_c, l1_c, gdl_c = MSELoss(temporal_weight=wp), L1Loss(temporal_weight=wp), GDL(alpha=alpha, temporal_weight=wg)

    def three(pred, target):
        l_mse, l_l1, l_gdl = mse_c(target, pred), l1_c(target, pred), gdl_c(target, pred)
        point = {"mse": l_mse, "l1": l_l1, "mse+l1": l_mse + l_l1}[args["point"]]
        return l_mse, l_l1, l_gdl, point

    if kind == "nar":
        def loss_terms(pred_frames, pred_feats, past, future, future_feats):
            a = tw.T.NCE_projector(pred_feats.permute(0, 1, 3, 4, 2))
            b = tw.T.NCE_projector(future_feats.permute(0, 1, 3, 4, 2))
            N, T, h, w_, C = a.shape
            l_mse, l_l1, l_gdl, point = three(pred_frames, future)
            l_pc = ops.nce_loss(b.reshape(-1, C), a.reshape(-1, C), N * T, h * w_, tw.nce_temperature)
            return l_gdl + point + tw.lam_pc * l_pc, {"T_GDL": l_gdl, "T_MSE": l_mse, "T_bpc": l_pc, "T_L1": l_l1}
        tw._loss_terms = loss_terms
    elif kind == "far":
        def loss_terms(pred_frames, pred_feats, past, future, aux):
            real = torch.cat([past[:, 1:], future], dim=1)
            l_mse, l_l1, l_gdl, point = three(pred_frames, real)
            return l_gdl + point, {"T_GDL": l_gdl, "T_MSE": l_mse, "T_L1": l_l1}
        tw._loss_terms = loss_terms
    else:
        def ae_recon(rec, x):
            l_mse, l_l1, l_gdl, point = three(rec, x)
            return l_mse, l_gdl, point, {"AE_L1": l_l1}
        tw._ae_recon = ae_recon


# ---- the defaults change nothing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nar", "far"])
def test_default_recon_is_bit_identical_to_none(pkg, dev, kind):
    from vptr_amd.train import ReconLoss
    runs = []
    for recon in (None, ReconLoss()):
        tr, c = _trainer(pkg, kind, dev, recon=recon)
        outs = [_floats(tr.step(*_batch(c, s, dev))) for s in range(3)]
        runs.append((outs, _slabs(tr)))
        del tr
    (oa, sa), (ob, sb) = runs
    for s in range(3):
        assert set(ob[s]) - set(oa[s]) == {"T_L1"} and set(oa[s]) <= set(ob[s])
        assert all(oa[s][k] == ob[s][k] for k in oa[s]), (s, oa[s], ob[s])
        assert ob[s]["T_L1"] > 0.0
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert torch.equal(x, y), "slab %d differs in %d elements" % (i, int((x != y).sum()))


# ---- against the torch criterion classes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,setting", [("nar", "l1_a2_exp"), ("nar", "msel1_a1.5"), ("far", "l1_a2_exp"), ("far", "msel1_a1.5"), ("ae", "msel1_a1.5")])
def test_recon_steps_match_a_twin_on_the_criterion_classes(pkg, dev, kind, setting):
    from helpers import margin, rel
    from vptr_amd.train import ReconLoss
    args, w = _settings(V.case(kind))[setting]
    tr, c = _trainer(pkg, kind, dev, recon=ReconLoss(**args))
    got = [_floats(tr.step(*_batch(c, s, dev))) for s in range(2)]
    got_p = [o.flat.clone() for o in _opts(tr)]
    del tr
    tw, c = _trainer(pkg, kind, dev)
    _torch_twin(tw, kind, args, w)
    ref = [_floats(tw.step(*_batch(c, s, dev))) for s in range(2)]
    ref_p = [o.flat.clone() for o in _opts(tw)]
    new = "AE_L1" if kind == "ae" else "T_L1"
    for s in range(2):
        assert set(got[s]) == set(ref[s]) and new in got[s], (sorted(got[s]), sorted(ref[s]))
        for k in ref[s]:
            bound = TOL * abs(ref[s][k]) + 1e-6
            margin("recon_loss trainer %s %s step %d %s" % (kind, setting, s, k), abs(got[s][k] - ref[s][k]), bound)
            print("%s %s step %d %-9s got % .9e  twin % .9e  bound %.3e" % (kind, setting, s, k, got[s][k], ref[s][k], bound))
            assert abs(got[s][k] - ref[s][k]) < bound, (s, k, got[s][k], ref[s][k])
    # the setting is in force: the total holds the chosen point term(s) and the GDL
    t0 = got[0]
    pre = "AE_" if kind == "ae" else "T_"
    point = (t0[pre + "MSE"] if "mse" in args["point"] else 0.0) + (t0[pre + "L1"] if "l1" in args["point"] else 0.0)
    rest = 0.1 * t0["T_bpc"] if kind == "nar" else (c["lam_gan"] * t0["AEgan"] if kind == "ae" else 0.0)
    assert abs(t0[pre + "total"] - (t0[pre + "GDL"] + point + rest)) < 1e-5 * abs(t0[pre + "total"])
    for i, (a, b) in enumerate(zip(got_p, ref_p)):
        v = margin("recon_loss trainer %s %s params %d" % (kind, setting, i), rel(a, b), PARAM_RTOL)
        print("%s %s parameters of optimizer %d after two steps: rel-L2 %.3e (bar %.1e)" % (kind, setting, i, v, PARAM_RTOL))
        assert v < PARAM_RTOL, (i, v)


# ---- eval_step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nar", "far"])
def test_eval_step_returns_the_new_key_and_leaves_the_trajectory(pkg, dev, kind):
    from vptr_amd.train import ReconLoss
    args, _ = _settings(V.case(kind))["l1_a2_exp"]
    finals = []
    for with_eval in (True, False):
        tr, c = _trainer(pkg, kind, dev, recon=ReconLoss(**args))
        for s in range(3):
            out = tr.step(*_batch(c, s, dev))
            if with_eval and s < 2:
                a = tr.eval_step(*_batch(c, 5 + s, dev))
                assert set(a) == set(out) - {"grad_norm"} and "T_L1" in a
                assert all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in a.values())
                b = tr.eval_step(*_batch(c, 5 + s, dev))
                assert all(torch.equal(a[k], b[k]) for k in a)
        finals.append(_slabs(tr))
        del tr
    for i, (x, y) in enumerate(zip(*finals)):
        assert torch.equal(x, y), "slab %d differs" % i
    ae, c = _trainer(pkg, "ae", dev, recon=ReconLoss("mse+l1", 1.5))
    e = ae.eval_step(*_batch(c, 0, dev))
    assert "AE_L1" in e and float(e["AE_L1"]) > 0.0
    assert abs(float(e["AE_total"]) - (c["lam_gan"] * float(e["AEgan"]) + float(e["AE_MSE"]) + float(e["AE_L1"]) + float(e["AE_GDL"]))) < 1e-5 * abs(float(e["AE_total"]))


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nar", "far"])
def test_capture_keeps_the_kernel_count_and_replays_equal_eager(pkg, dev, kind):
    from vptr_amd.train import ReconLoss
    base, c = _trainer(pkg, kind, dev)
    past, fut = _batch(c, 0, dev)
    base.capture(past, fut, warmup=2)
    want = dict(base.graph_nodes)
    del base
    args, _ = _settings(c)["l1_a2_exp"]
    tr, c = _trainer(pkg, kind, dev, recon=ReconLoss(**args))
    tr.capture(past, fut, warmup=2)
    assert "memset" not in tr.graph_nodes and tr.graph_nodes["kernel"] == want["kernel"], (tr.graph_nodes, want)
    ok, rep = tr.verify_graph(past, fut, steps=3)
    assert ok, rep
    out = tr.step(past, fut)
    assert out is tr._static_out and "T_L1" in out
    tr.capture_eval(past, fut)
    assert "memset" not in tr.eval_graph_nodes and "T_L1" in tr.eval_step(past, fut)


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_set_temporal_weight_between_replays(pkg, dev, kind):
    from helpers import rel
    from vptr_amd.train import NARTrainer, ReconLoss
    c = V.case(kind)
    T = _loss_T(c)
    args, (exp, _) = _settings(c)["l1_a2_exp"]
    new_p, new_g = torch.linspace(3.0, 5.0, T), torch.linspace(0.25, 0.5, T)      # means of 4 and 0.375 against the exponential weights' ~2
    tr, c = _trainer(pkg, kind, dev, recon=ReconLoss(**args))
    past, fut = _batch(c, 0, dev)
    tr.capture(past, fut, warmup=2)
    nodes = dict(tr.graph_nodes)
    first = _floats(tr.step(past, fut))                      # a replay with the weights of the construction
    snap = tr._snapshot()
    tr.set_temporal_weight(new_p, gdl=new_g)
    assert tr.graph_nodes == nodes and tr.has_graph()
    second = _floats(tr.step(past, fut))                     # the next replay reads the new ones
    second_p = tr.opt.flat.clone()
    tr._restore(snap)
    tr.set_temporal_weight("exp")
    old = _floats(tr.step(past, fut))                        # the same replay, from the same state, with the old weights again
    del tr
    tw, c = _trainer(pkg, kind, dev, recon=ReconLoss("l1", 2.0, new_p, new_g))
    tw.step(past, fut)                                       # builds the twin's weight buffers before its state is replaced
    tw._restore(snap)
    ref = _floats(tw.step(past, fut))                        # eager
    assert set(ref) == set(second)
    for k in ref:
        d = NARTrainer._term_diff(ref[k], second[k])
        print("set_temporal_weight[%s] %-9s eager twin % .9e replay % .9e rel %.3e" % (kind, k, ref[k], second[k], d))
        assert d <= GRAPH_RTOL, (k, ref[k], second[k])
    assert rel(second_p, tw.opt.flat) < PARAM_RTOL
    for k in ("T_L1", "T_GDL"):
        assert NARTrainer._term_diff(old[k], second[k]) > 10 * GRAPH_RTOL, (k, old[k], second[k], first[k])
    assert NARTrainer._term_diff(old["T_MSE"], second["T_MSE"]) > 10 * GRAPH_RTOL


def test_set_temporal_weight_rules(pkg, dev):
    from vptr_amd.train import ReconLoss
    tr, c = _trainer(pkg, "far", dev, recon=ReconLoss("mse", 1.0))
    with pytest.raises(ValueError):
        tr.set_temporal_weight("exp")                        # constructed without weights: the launches hold NULL
    del tr
    T = _loss_T(V.case("far"))
    tr, c = _trainer(pkg, "far", dev, recon=ReconLoss("mse", 1.0, "exp", None))
    tr.step(*_batch(c, 0, dev))
    with pytest.raises(ValueError):
        tr.set_temporal_weight(torch.ones(T + 1))
    with pytest.raises(ValueError):
        tr.set_temporal_weight(torch.ones(T), gdl=torch.ones(T))       # no GDL weights to rewrite
    tr.set_temporal_weight(torch.full((T,), 2.0))
    assert torch.equal(tr._recon_w[0].cpu(), torch.full((T,), 2.0)) and tr._recon_w[1] is None


# ---- meters ------------------------------------------------------------------------------------------------------------------------------
def test_device_loss_meters_take_the_new_key(pkg, dev):
    from vptr_amd.meters import DeviceLossMeters
    from vptr_amd.train import ReconLoss
    args, _ = _settings(V.case("far"))["l1_a2_exp"]
    tr, c = _trainer(pkg, "far", dev, recon=ReconLoss(**args))
    names = ["T_total", "T_MSE", "T_GDL", "T_L1"]
    m = DeviceLossMeters(names, dev)
    outs = [_floats(tr.step(*_batch(c, s, dev), meters=m)) for s in range(3)]
    res = m.compute()
    for k in names:
        mean = sum(o[k] for o in outs) / 3
        assert res[k]["count"] == 3.0 and abs(res[k]["avg"] - mean) <= 1e-6 * abs(mean) and res[k]["last"] == outs[-1][k], (k, res[k])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_value_errors(pkg, dev):
    from vptr_amd.train import ReconLoss
    with pytest.raises(ValueError):
        _trainer(pkg, "ae", dev, recon=ReconLoss("mse", 1.0, "exp"))
    with pytest.raises(ValueError):
        _trainer(pkg, "ae", dev, recon=ReconLoss("mse", 1.0, None, [1.0, 2.0]))
    with pytest.raises(ValueError):
        ReconLoss(gdl_alpha=0.5)
    with pytest.raises(ValueError):
        _trainer(pkg, "nar", dev, recon="l1")
    for kind in ("nar", "far"):
        T = _loss_T(V.case(kind))
        tr, c = _trainer(pkg, kind, dev, recon=ReconLoss("l1", 1.0, torch.ones(T + 1)))
        with pytest.raises(ValueError):
            tr.step(*_batch(c, 0, dev))                     # a wrong length shows at the first step
        del tr
    if V.case("far")["cfg"]["Tp"] > 1:                       # the FAR loss sees Tp - 1 + Tf frames, not Tf
        tr, c = _trainer(pkg, "far", dev, recon=ReconLoss("l1", 1.0, torch.ones(V.case("far")["cfg"]["Tf"])))
        with pytest.raises(ValueError):
            tr.step(*_batch(c, 0, dev))
