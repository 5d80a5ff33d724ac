"""Validation pass and epoch loss meters on the device.

  * `vptr_meters_add` through the C ABI: guard rows and reserved slots, special values, NULL entries, 300 sequential calls against a
    Python-float loop with `==`, every reject, capture + replay.
  * `eval_step` of the three trainers against the oracle in eval mode on the same parameters and buffers, fresh and after two steps.
    Bar: the loss-term bar of tests/test_02_model_gpu.py, TOL * |ref| + 1e-6 with that file's TOL.
  * eval_step leaves a training trajectory bit-identical (deterministic mode) and writes nothing a step owns.
  * `capture_eval`: replay vs eager within verify_graph's rtol (2e-3), train and eval graphs alternating, fall-back, static inputs.
  * `run_epoch` + `DeviceLossMeters` end to end, into a checkpoint and back.
"""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import validation_cases as V
from test_02_model_gpu import TOL

pytestmark = pytest.mark.gpu

GRAPH_RTOL = 2e-3      # NARTrainer.verify_graph's rtol
SENTINEL = 0x7FF8DEADBEEF0001   # a NaN payload: any arithmetic on it, or any store over it, changes the bits


@pytest.fixture(scope="module")
def pkg():
    import vptr_amd.model as pkg
    return pkg


@pytest.fixture(autouse=True)
def _drop_slabs():
    yield
    from vptr_amd import ops
    ops.unregister_flat_slabs()


# ---- vptr_meters_add through ctypes --------------------------------------------------------------------------------------------
def _guarded_state(dev, K):
    """int64 view of (K + 2) rows of 8: the K state rows zeroed except their three reserved slots, everything else the sentinel"""
    buf = torch.full(((K + 2), 8), SENTINEL, dtype=torch.int64, device=dev)
    buf[1:K + 1, :5] = 0
    return buf


def _state_ptr(buf):
    return ctypes.c_void_p(buf.data_ptr() + 64)


def _guards_intact(buf, K):
    b = buf.cpu()
    return bool((b[0] == SENTINEL).all() and (b[K + 1] == SENTINEL).all() and (b[1:K + 1, 5:] == SENTINEL).all())


def _rows(buf, K):
    return buf[1:K + 1].view(torch.float64).cpu().tolist()


def _add(src, K, state, weight):
    from vptr_amd import _lib
    return _lib.lib.vptr_meters_add(src, K, state, weight, _lib.stream())


def _same(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


FINITE = [0.0, -0.0, 1e-45, -3e-39, 1.17549435e-38, 3.4e38, -3.4e38, 1.0, -2.5, 0.1, 16777217.0]   # zeros, denormals, extremes
NONFINITE = [float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("weight", [1.0, 16.0])
@pytest.mark.parametrize("K", [1, 5, 16])
def test_meters_add_values_nulls_and_guards(dev, K, weight):
    """phase 1: finite values only, so that every sum stays comparable with `==`; phase 2 goes on with NaN and +-Inf"""
    rng = np.random.RandomState(K)
    # NULL patterns: none, first, last, middle, first and last, all -- 6 patterns against 11 (then 3) values per row: every pairing occurs
    patterns = [set(), {0}, {K - 1}, {K // 2}, {0, K - 1}, set(range(K))]
    buf = _guarded_state(dev, K)
    recs = [V.HostRecord() for _ in range(K)]
    for pool, calls in ((FINITE, 6 * len(FINITE)), (NONFINITE, 6 * len(NONFINITE))):
        vals = np.empty((calls, K), dtype=np.float32)
        for j in range(calls):
            for k in range(K):
                vals[j, k] = pool[(j + k) % len(pool)] if (j // len(pool) + k) % 4 else np.float32(rng.randn() * 10.0 ** rng.randint(-20, 20))
        dv = torch.from_numpy(vals).to(dev)
        for j in range(calls):
            null = patterns[j % len(patterns)]
            src = (ctypes.c_void_p * K)(*[None if k in null else dv.data_ptr() + 4 * (j * K + k) for k in range(K)])
            assert _add(src, K, _state_ptr(buf), weight) == 0
            for k in range(K):
                if k not in null:
                    recs[k].add(float(vals[j, k]), weight)
        torch.cuda.synchronize()
        assert _guards_intact(buf, K)
        for k, row in enumerate(_rows(buf, K)):
            r = recs[k]
            exp = (r.sum, r.sumsq, r.count, r.nonfinite, 0.0 if r.last is None else r.last)
            assert all(_same(a, b) for a, b in zip(row[:5], exp)), (k, row[:5], exp)
        if pool is FINITE:
            assert all(r.nonfinite == 0 and math.isfinite(r.sum) and math.isfinite(r.sumsq) and r.count > 0 for r in recs)
    assert all(r.nonfinite > 0 and r.sum != r.sum for r in recs)       # as in the reference: a non-finite value poisons the average


def test_meters_add_300_sequential_calls_equal_python_loop(dev):
    K, calls = 5, 300
    rng = np.random.RandomState(2024)
    vals = (rng.randn(calls, K) * 10.0 ** rng.randint(-6, 6, size=(calls, K))).astype(np.float32)
    dv = torch.from_numpy(vals).to(dev)
    buf = _guarded_state(dev, K)
    for j in range(calls):      # no sync in between: stream order alone keeps the read-modify-write of a row race-free
        src = (ctypes.c_void_p * K)(*[dv.data_ptr() + 4 * (j * K + k) for k in range(K)])
        assert _add(src, K, _state_ptr(buf), 1.0) == 0
    torch.cuda.synchronize()
    assert _guards_intact(buf, K)
    for k, row in enumerate(_rows(buf, K)):
        r = V.HostRecord()
        for j in range(calls):
            r.add(float(vals[j, k]))
        assert row[0] == r.sum and row[1] == r.sumsq and row[2] == 300.0 and row[3] == 0.0 and row[4] == r.last, (k, row, r.__dict__)


def test_meters_add_rejects_leave_the_buffer_alone(dev):
    K = 5
    buf = _guarded_state(dev, K)
    x = torch.ones(K, dtype=torch.float32, device=dev)
    src = (ctypes.c_void_p * 16)(*([x.data_ptr() + 4 * k for k in range(K)] + [None] * 11))
    assert _add(src, K, _state_ptr(buf), 1.0) == 0
    torch.cuda.synchronize()
    before = buf.clone()
    st = _state_ptr(buf)
    bad = [(src, 0, st, 1.0), (src, -3, st, 1.0), (src, 17, st, 1.0), (src, K, None, 1.0), (src, K, ctypes.c_void_p(st.value + 4), 1.0),
           (None, K, st, 1.0), (src, K, st, 0.0), (src, K, st, -1.0), (src, K, st, float("nan")), (src, K, st, float("inf"))]
    for s, k, p, w in bad:
        assert _add(s, k, p, w) != 0, (k, w)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def test_meters_add_capture_and_replay(dev):
    from vptr_amd.train import graph_node_census
    K = 5
    buf = _guarded_state(dev, K)
    x = torch.zeros(K, dtype=torch.float32, device=dev)
    src = (ctypes.c_void_p * K)(*[None if k == 2 else x.data_ptr() + 4 * k for k in range(K)])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        assert _add(src, K, _state_ptr(buf), 1.0) == 0
    assert graph_node_census(g) == {"kernel": 1}
    g.instantiate()
    recs = [V.HostRecord() for _ in range(K)]
    for i in range(5):
        new = [_f32(0.37 * (i + 1) * (k + 1) - 1.0) for k in range(K)]
        x.copy_(torch.tensor(new, dtype=torch.float32))      # the source scalars are rewritten between replays
        g.replay()
        for k in range(K):
            if k != 2:
                recs[k].add(new[k])
    torch.cuda.synchronize()
    assert _guards_intact(buf, K)
    for k, row in enumerate(_rows(buf, K)):
        r = recs[k]
        if k == 2:
            assert row[:5] == [0.0] * 5
        else:
            assert row[2] == 5.0 and row[0] == r.sum and row[1] == r.sumsq and row[4] == r.last and row[3] == 0.0


# ---- eval_step against the oracle ----------------------------------------------------------------------------------------------
def _dev_batch(c, s, dev, N=None):
    past, fut = V.batch(c, s, N)
    return past, fut, past.to(dev), fut.to(dev)


def _check_terms(tag, got, ref, keys):
    assert set(got) == set(keys), (sorted(got), sorted(keys))
    worst = 0.0
    for k in keys:
        g, r = float(got[k]), ref[k]
        bound = TOL * abs(r) + 1e-6
        worst = max(worst, abs(g - r) / bound)
        print("%s %-8s got % .9e  oracle % .9e  |diff| %.3e  bound %.3e" % (tag, k, g, r, abs(g - r), bound))
    print("%s worst |diff| / bound = %.4f" % (tag, worst))
    for k in keys:
        assert got[k].dim() == 0 and got[k].dtype == torch.float32 and got[k].is_cuda and not got[k].requires_grad
        assert abs(float(got[k]) - ref[k]) < TOL * abs(ref[k]) + 1e-6, (tag, k, float(got[k]), ref[k])


def _keys(kind):
    if kind == "ae":
        return ["AEgan", "AE_MSE", "AE_GDL", "AE_total", "Dtotal", "Dfake", "Dreal"]
    base = ["T_total", "T_GDL", "T_MSE"] + (["T_bpc"] if kind.startswith("nar") else [])
    return base + (["T_gan", "Dtotal", "Dfake", "Dreal"] if kind.endswith("gan") else [])


@pytest.mark.parametrize("kind", V.KINDS)
def test_eval_step_matches_oracle(pkg, dev, kind):
    c = V.case(kind)
    tr = V.trainer(pkg, c, dev)
    past, fut, dpast, dfut = _dev_batch(c, 0, dev)
    if kind == "far_gan":
        assert past.shape[1] + fut.shape[1] - 1 != fut.shape[1]     # cal_lossD sees clips of unequal length, both flattened
    ref = V.oracle_eval(c, V.trainer_state(tr), past, fut)
    got = tr.eval_step(dpast, dfut)
    _check_terms("eval[%s]" % kind, got, ref, _keys(kind))
    mods = [m for m in (getattr(tr, "T", None), getattr(tr, "disc", None)) + ((tr.enc, tr.dec) if kind == "ae" else ()) if m is not None]
    assert all(not m.training for m in mods)
    out = tr.step(dpast, dfut)                       # the next step puts the modules back into train mode
    assert set(out) - {"grad_norm"} == set(_keys(kind))
    assert all(m.training for m in mods)


@pytest.mark.parametrize("kind", ["nar_gan", "far", "ae"])
def test_eval_step_after_two_steps_sees_stepped_state(pkg, dev, kind):
    """the oracle reads the stepped state_dict and buffers: a packed weight, plane or BatchNorm fold kept from before the optimizer
    steps (or running statistics the steps did not reach) would show here.  The learning rate is 30x the recipe's so that two steps
    move the terms well past the bar (asserted below); the oracle reads whatever state the steps left, no optimizer parity is involved."""
    c = V.case(kind)
    tr = V.trainer(pkg, c, dev, lr=3e-3)
    past, fut, dpast, dfut = _dev_batch(c, 2, dev)
    before = V.oracle_eval(c, V.trainer_state(tr), past, fut)
    tr.eval_step(dpast, dfut)                        # fills whatever an eval-mode forward would cache
    for s in range(2):
        _, _, p, f = _dev_batch(c, s, dev)
        tr.step(p, f)
    ref = V.oracle_eval(c, V.trainer_state(tr), past, fut)
    got = tr.eval_step(dpast, dfut)
    _check_terms("stepped[%s]" % kind, got, ref, _keys(kind))
    moved = [k for k in ref if abs(ref[k] - before[k]) > 4 * (TOL * abs(ref[k]) + 1e-6)]
    print("stepped[%s]: terms the two steps moved past the bar: %s" % (kind, moved))
    assert moved, "two steps did not move any term: this case could not see a stale cache"


# ---- non-interference --------------------------------------------------------------------------------------------------------------
def _full_state(tr, dev):
    from vptr_amd import ops
    opts = [o for o in (getattr(tr, "opt", None), getattr(tr, "opt_G", None), getattr(tr, "opt_D", None)) if o is not None]
    st = {}
    for i, o in enumerate(opts):
        st.update({"flat%d" % i: o.flat.clone(), "m%d" % i: o.m.clone(), "v%d" % i: o.v.clone(), "step%d" % i: o.step_dev.clone(),
                   "grad%d" % i: o.grad.clone()})
    for name in ("enc", "dec", "T", "disc"):
        m = getattr(tr, name, None)
        if m is not None:
            for k, b in m.named_buffers():
                st["%s.%s" % (name, k)] = b.detach().clone()
    st["seed"] = ops._master_seed(dev).clone()
    return st


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_eval_steps_leave_the_trajectory_bit_identical(pkg, dev, kind):
    from vptr_amd import ops
    c = V.case(kind)
    ops.unregister_flat_slabs()
    ops.set_deterministic(True)
    try:
        finals = []
        for with_eval in (True, False):
            ops.manual_seed(dev, 77)
            tr = V.trainer(pkg, c, dev)
            for s in range(3):
                _, _, p, f = _dev_batch(c, s, dev)
                tr.step(p, f)
                if with_eval and s < 2:
                    _, _, ep, ef = _dev_batch(c, 5 + s, dev)
                    grads = [q.grad for q in tr.dec.parameters()]
                    g0 = tr.opt.grad.clone()
                    a = tr.eval_step(ep, ef)
                    assert torch.equal(tr.opt.grad, g0)                                   # the gradient slab
                    assert ops.take_wgrads() == []                                        # the weight-gradient queue
                    assert all(x is y for x, y in zip(grads, [q.grad for q in tr.dec.parameters()]))
                    b = tr.eval_step(ep, ef)
                    assert all(torch.equal(a[k], b[k]) for k in a)
            st = _full_state(tr, dev)
            st.pop("grad0")
            finals.append(st)
            del tr
            ops.unregister_flat_slabs()
        assert finals[0].keys() == finals[1].keys()
        bad = [k for k in finals[0] if not torch.equal(finals[0][k], finals[1][k])]
        assert not bad, bad
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("kind", ["nar_gan", "far_gan", "ae"])
def test_eval_step_writes_nothing_a_step_owns(pkg, dev, kind):
    """every optimizer slab (parameters, moments, step count, gradients), every module buffer (BatchNorm running statistics and
    counters) and the dropout master seed, bit for bit, around an eval_step -- before any step and after one"""
    from vptr_amd import ops
    c = V.case(kind)
    tr = V.trainer(pkg, c, dev)
    _, _, p, f = _dev_batch(c, 0, dev)
    for stage in range(2):
        scope = ops._seed_scope.get(ops._dev_key(dev))
        grads = [q.grad for q in tr.dec.parameters()]
        st0 = _full_state(tr, dev)
        tr.eval_step(p, f)
        st1 = _full_state(tr, dev)
        bad = [k for k in st0 if not torch.equal(st0[k], st1[k])]
        assert not bad, (stage, bad)
        assert ops._seed_scope.get(ops._dev_key(dev)) is scope and ops.take_wgrads() == []
        assert all(x is y for x, y in zip(grads, [q.grad for q in tr.dec.parameters()]))
        tr.step(p, f)


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def _term_diff(a, b):
    from vptr_amd.train import NARTrainer
    return NARTrainer._term_diff(float(a), float(b))


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_capture_eval_replay_fallback_and_static_inputs(pkg, dev, kind, monkeypatch):
    c = V.case(kind)
    tr = V.trainer(pkg, c, dev)
    _, _, p0, f0 = _dev_batch(c, 0, dev)
    _, _, p1, f1 = _dev_batch(c, 1, dev)
    eager = {k: float(v) for k, v in tr.eval_step(p1, f1).items()}
    tr.capture_eval(p0, f0)
    assert set(tr.eval_graph_nodes) <= {"kernel", "memcpy", "empty"} and tr.eval_graph_nodes["kernel"] > 10
    for i in range(3):                               # consecutive replays
        out = tr.eval_step(p1, f1)
        assert out is tr._eval_out
        for k in eager:
            d = _term_diff(eager[k], out[k])
            print("replay[%s] %d %-8s eager % .9e replay % .9e rel %.3e" % (kind, i, k, eager[k], float(out[k]), d))
            assert d <= GRAPH_RTOL, (i, k, eager[k], float(out[k]))
    # a batch of another size runs eagerly
    _, _, ps, fs = _dev_batch(c, 3, dev, N=1)
    small = tr.eval_step(ps, fs)
    assert small is not tr._eval_out
    g, tr._eval_graph = tr._eval_graph, None
    ref_small = tr.eval_step(ps, fs)
    tr._eval_graph = g
    assert all(_term_diff(ref_small[k], small[k]) <= GRAPH_RTOL for k in small)
    # static inputs handed back: no copy
    sp, sf = tr.static_inputs(train=False)
    assert sp.shape == p0.shape and sf.shape == f0.shape
    with pytest.raises(RuntimeError):
        tr.static_inputs(train=True)
    copies = []
    real_copy = torch.Tensor.copy_

    def counting_copy(self, *a, **kw):
        if self is sp or self is sf:
            copies.append(self)
        return real_copy(self, *a, **kw)

    monkeypatch.setattr(torch.Tensor, "copy_", counting_copy)
    tr.eval_step(p1, f1)
    assert len(copies) == 2
    tr.eval_step(sp, sf)
    assert len(copies) == 2
    monkeypatch.undo()
    # ClipIngest writing into the static inputs == ingest into fresh tensors
    from vptr_amd.data import ClipIngest, IngestPlan
    HW = c["meta"]["HW"]
    Tp, Tf = p0.shape[1], f0.shape[1]
    raw = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(p0.shape[0], Tp + Tf, HW, HW, 1)).astype(np.uint8)).to(dev)
    ing = ClipIngest(IngestPlan((HW, HW), 1, (HW, HW), mean=V.NORM[0], std=V.NORM[1], device=dev), Tp, Tf)
    fp, ff = ing(raw)
    fresh = {k: v.clone() for k, v in tr.eval_step(fp, ff).items()}
    got_p, got_f = ing(raw, out=tr.static_inputs(train=False))
    assert got_p is sp and got_f is sf and torch.equal(sp, fp) and torch.equal(sf, ff)
    out = tr.eval_step(got_p, got_f)      # the same replay on bit-identical inputs (the default mode's forward sums are not bit-reproducible)
    assert all(_term_diff(fresh[k], out[k]) <= GRAPH_RTOL for k in fresh)
    # run_epoch with an ingest: full batches go through the static inputs and the graph, the short last batch runs eagerly
    from vptr_amd.meters import DeviceLossMeters
    from vptr_amd.train import run_epoch
    raws = [raw, raw.flip(0).contiguous(), raw[:1].contiguous()]
    expect = [{k: float(v) for k, v in tr.eval_step(*ing(r)).items()} for r in raws]
    res = run_epoch(tr, raws, False, DeviceLossMeters(list(fresh), dev), ingest=ing).compute()
    for k in fresh:
        mean = sum(e[k] for e in expect) / 3
        assert res[k]["count"] == 3.0 and abs(res[k]["avg"] - mean) <= GRAPH_RTOL * abs(mean), (k, res[k], mean)
        assert _term_diff(expect[-1][k], res[k]["last"]) <= GRAPH_RTOL


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_train_and_eval_graphs_alternate(pkg, dev, kind):
    """step, eval_step x 3 as replays of two coexisting graphs vs the same sequence run eagerly from the same state (deterministic
    mode, so that the train trajectory itself adds no run-to-run noise to the comparison; the bar is verify_graph's rtol)"""
    from vptr_amd import ops
    c = V.case(kind)
    ops.unregister_flat_slabs()
    ops.set_deterministic(True)
    try:
        tr = V.trainer(pkg, c, dev)
        batches = [_dev_batch(c, s, dev)[2:] for s in range(6)]
        snap = tr._snapshot()
        tr.capture(*batches[0], warmup=1)
        tr.capture_eval(*batches[1])
        assert tr.static_inputs(train=True)[0] is not tr.static_inputs(train=False)[0]
        graphs = (tr._graph, tr._eval_graph)
        runs = {}
        for mode in ("graph", "eager"):
            tr._restore(snap)
            tr._graph, tr._eval_graph = graphs if mode == "graph" else (None, None)
            seq = []
            for r in range(3):
                seq.append({k: float(v) for k, v in tr.step(*batches[2 * r]).items()})
                seq.append({k: float(v) for k, v in tr.eval_step(*batches[2 * r + 1]).items()})
            runs[mode] = seq
        tr._graph, tr._eval_graph = graphs
        for i, (a, b) in enumerate(zip(runs["eager"], runs["graph"])):
            assert a.keys() == b.keys()
            for k in a:
                d = _term_diff(a[k], b[k])
                print("alternate[%s] %d %-9s eager % .9e graph % .9e rel %.3e" % (kind, i, k, a[k], b[k], d))
                assert d <= GRAPH_RTOL, (i, k, a[k], b[k])
    finally:
        ops.set_deterministic(False)


# ---- meters end to end -------------------------------------------------------------------------------------------------------------
def test_run_epoch_meters_checkpoint_roundtrip(pkg, dev, tmp_path):
    from vptr_amd import ops
    from vptr_amd.checkpoint import init_loss_dict, resume_training, save_ckpt
    from vptr_amd.meters import DeviceLossMeters
    from vptr_amd.train import run_epoch
    c = V.case("nar")
    names = ["T_total", "T_MSE", "T_GDL", "T_bpc", "T_gan"]       # T_gan: a name of the script's list this run never feeds
    train_loader = [_dev_batch(c, s, dev)[2:] for s in range(7)]
    val_loader = [_dev_batch(c, 10 + s, dev)[2:] for s in range(7)]
    ops.unregister_flat_slabs()
    ops.set_deterministic(True)      # the twin run must reproduce the metered run's values bit for bit
    try:
        ops.manual_seed(dev, 5)
        tr = V.trainer(pkg, c, dev)
        m_train, m_val = DeviceLossMeters(names, dev), DeviceLossMeters(names, dev)
        assert run_epoch(tr, train_loader, True, m_train) is m_train
        assert run_epoch(tr, val_loader, False, m_val) is m_val
        got_train, got_val = m_train.compute(), m_val.compute()
        del tr
        ops.unregister_flat_slabs()
        ops.manual_seed(dev, 5)
        twin = V.trainer(pkg, c, dev)
        t_vals = [{k: float(v) for k, v in twin.step(p, f).items()} for p, f in train_loader]
        v_vals = [{k: float(v) for k, v in twin.eval_step(p, f).items()} for p, f in val_loader]
        for tag, got, vals in (("train", got_train, t_vals), ("val", got_val, v_vals)):
            for k in names[:4]:
                s = 0.0
                for it in vals:
                    s += it[k]
                mean = s / len(vals)
                print("epoch %-5s %-8s meter avg % .17e  twin mean % .17e" % (tag, k, got[k]["avg"], mean))
                assert abs(got[k]["avg"] - mean) <= 1e-12 * abs(mean)
                assert got[k]["count"] == 7.0 and got[k]["last"] == vals[-1][k] and got[k]["nonfinite"] == 0
            assert got["T_gan"]["count"] == 0.0 and got["T_gan"]["avg"] == 0
        loss_dict = init_loss_dict(names + ["Dtotal"])
        m_train.epoch_update(loss_dict, 1, train_flag=True)
        m_val.epoch_update(loss_dict, 1, train_flag=False)
        assert loss_dict["epochs"] == 1 and loss_dict["Dtotal"].train == [0] and loss_dict["Dtotal"].val == [0]
        assert loss_dict["T_MSE"].train == [got_train["T_MSE"]["avg"]] and loss_dict["T_MSE"].val == [got_val["T_MSE"]["avg"]]
        save_ckpt({"T": twin.T}, {"opt": twin.opt}, 1, loss_dict, tmp_path)
        back, epoch = resume_training({"T": twin.T}, {"opt": twin.opt}, tmp_path / "epoch_1.tar", names + ["Dtotal"])
        assert epoch == 1 and back["epochs"] == 1
        for k in names + ["Dtotal"]:
            assert back[k].train == loss_dict[k].train and back[k].val == loss_dict[k].val
        # a NaN in one term: counted, poisons that average only
        m_val.update({"T_MSE": torch.full((), float("nan"), device=dev), "T_GDL": torch.ones((), device=dev)})
        out = m_val.compute()
        assert out["T_MSE"]["nonfinite"] == 1 and math.isnan(out["T_MSE"]["avg"]) and out["T_MSE"]["count"] == 8.0
        assert all(math.isfinite(out[k]["avg"]) and out[k]["nonfinite"] == 0 for k in ("T_total", "T_GDL", "T_bpc"))
        m_val.reset()
        assert all(v["count"] == 0.0 for v in m_val.compute().values())
        with pytest.raises(KeyError):
            m_val.update({"AE_MSE": torch.ones((), device=dev)})
    finally:
        ops.set_deterministic(False)
