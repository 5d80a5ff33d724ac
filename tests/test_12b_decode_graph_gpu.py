"""KV-cached decoding at a device-held position (include/vptr_hip_decode.h): vptr_tattn_step_pos through the C ABI against
vptr_tattn_step bit for bit (every buffer NaN-filled inside NaN guard rows), vptr_decode_begin / _advance, the rejects, the three launches
captured once and replayed over the positions, `forward_cached` on a `FARCache(device_pos=True)` eager and replayed against the plain
cache, the graph rollouts of `CachedDecoder` / `far_rollout(graph=True)` / `FARTrainer.predict(graph=True)` and the host's ValueErrors."""
import pytest
import torch

import decode_graph_cases as D
import validation_cases as V
from helpers import build_transformer, jload, load, rel
from oracle import fill

pytestmark = pytest.mark.gpu

TOL = 1e-3    # the project's model bar: what tests/test_12_far_cache_gpu.py holds cached outputs and rollouts to


@pytest.fixture(scope="module")
def pkg():
    import vptr_amd.model as pkg
    return pkg


@pytest.fixture(autouse=True)
def _clean():
    from vptr_amd import ops
    yield
    ops.set_deterministic(False)
    ops.unregister_flat_slabs()


# ------------------------------------------------------------------------------------------------------ 1. the kernels, directly
def _abi():
    from vptr_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


def run_step_pos(q, kn, vn, kc, vc, o, rec, rows, Tcap, C, nh, p16):
    check, lib, ptr, stream = _abi()
    check(lib.vptr_tattn_step_pos(ptr(q), ptr(kn), ptr(vn), ptr(kc), ptr(vc), ptr(o), ptr(rec), rows, Tcap, C, nh, p16, stream()), "vptr_tattn_step_pos")
    torch.cuda.synchronize()


def step_reference(q, kfill, vfill, Tk, rows, Tcap, C, nh, p16, dev="cuda:0"):
    """vptr_tattn_step on a cache whose slot Tk - 1 was filled with knew / vnew"""
    check, lib, ptr, stream = _abi()
    qd, kd, vd = q.to(dev), kfill.to(dev), vfill.to(dev)
    o = torch.full(q.shape, float("nan"), device=dev)
    check(lib.vptr_tattn_step(ptr(qd), ptr(kd), ptr(vd), ptr(o), rows, Tk, Tcap, C, nh, p16, stream()), "vptr_tattn_step")
    return o


@pytest.mark.parametrize("case", D.STEP_CASES, ids=lambda c: "r%d-cap%d-pos%d-C%d-nh%d-p%d" % c)
def test_step_pos_is_bit_identical_to_step(dev, case):
    bad = D.check_step_case(run_step_pos, case, device=dev, reference=step_reference)
    assert bad == [], bad


def test_step_pos_vs_fp64(dev):
    bad = D.check_step_case(run_step_pos, D.FP64_CASE, device=dev, reference=None)
    assert bad == [], bad


def test_full_cache_is_left_alone(dev):
    """POS == Tcap: caches, o and guards untouched; the advance leaves POS alone and counts OVERFLOW"""
    check, lib, ptr, stream = _abi()
    bad = D.check_full_case(run_step_pos, 17, 5, 48, 4, device=dev)
    assert bad == [], bad
    rec = D.record(5, 5).to(dev)
    check(lib.vptr_decode_advance(ptr(rec), stream()), "vptr_decode_advance")
    assert rec.tolist()[:4] == [5, 5, 1, 0]


@pytest.mark.parametrize("C", [15, 528])
def test_decode_begin(dev, C):
    check, lib, ptr, stream = _abi()

    def run(rec, tpos, cur, Tmax, C_):
        check(lib.vptr_decode_begin(ptr(rec), ptr(tpos), ptr(cur), Tmax, C_, stream()), "vptr_decode_begin")
        torch.cuda.synchronize()
    bad = D.check_begin(run, C, 6, device=dev)
    assert bad == [], bad


def test_decode_advance(dev):
    check, lib, ptr, stream = _abi()
    bad = D.check_advance(lambda rec: check(lib.vptr_decode_advance(ptr(rec), stream()), "vptr_decode_advance"), 5, device=dev)
    assert bad == [], bad


REJECTS = [("null_rec", {}), ("null_knew", {}), ("null_vnew", {}), ("heads", dict(nh=5)), ("p16", dict(p16=1)), ("rows", dict(rows=0)),
           ("tcap", dict(Tcap=0))]


@pytest.mark.parametrize("what,kw", REJECTS, ids=[r[0] for r in REJECTS])
def test_step_pos_rejects(dev, what, kw):
    _, lib, ptr, stream = _abi()
    rows, Tcap, C, nh = 2, 3, 12, 2
    q = torch.zeros((rows, C), device=dev)
    kn, vn = torch.zeros_like(q), torch.zeros_like(q)
    kc = torch.full((Tcap, rows, C), 7.25, device=dev)
    vc, o = kc.clone(), torch.full((rows, C), 7.25, device=dev)
    rec = D.record(1, Tcap).to(dev)
    a = dict(rows=rows, Tcap=Tcap, C=C, nh=nh, p16=0)
    a.update(kw)
    rc = lib.vptr_tattn_step_pos(ptr(q), None if what == "null_knew" else ptr(kn), None if what == "null_vnew" else ptr(vn), ptr(kc), ptr(vc),
                                 ptr(o), None if what == "null_rec" else ptr(rec), a["rows"], a["Tcap"], a["C"], a["nh"], a["p16"], stream())
    assert rc != 0
    assert "tattn_step_pos" in lib.vptr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((o == 7.25).all()) and bool((kc == 7.25).all()) and bool((vc == 7.25).all())
    assert torch.equal(rec.cpu(), D.record(1, Tcap))


def test_begin_and_advance_reject(dev):
    _, lib, ptr, stream = _abi()
    rec = D.record(1, 4).to(dev)
    tpos, cur = torch.zeros((4, 8), device=dev), torch.full((8,), 7.25, device=dev)
    for args in ((None, ptr(tpos), ptr(cur), 4, 8), (ptr(rec), None, ptr(cur), 4, 8), (ptr(rec), ptr(tpos), None, 4, 8),
                 (ptr(rec), ptr(tpos), ptr(cur), 0, 8), (ptr(rec), ptr(tpos), ptr(cur), 4, 0)):
        assert lib.vptr_decode_begin(*args, stream()) != 0
        assert "decode_begin" in lib.vptr_last_error().decode()
    assert lib.vptr_decode_advance(None, stream()) != 0
    assert "decode_advance" in lib.vptr_last_error().decode()
    torch.cuda.synchronize()
    assert bool((cur == 7.25).all()) and torch.equal(rec.cpu(), D.record(1, 4))


# ------------------------------------------------------------------------------------------------------ 2. captured once
def test_three_launches_captured_once_serve_every_position(dev):
    from vptr_amd.train import graph_node_census
    check, lib, ptr, stream = _abi()
    rows, Tcap, C, nh, Tmax = 17, 6, 48, 4, 8
    q, kn, vn, kc, vc = D.step_inputs(rows, Tcap, 2, C)
    tpos = fill.rand_normal((Tmax, C), 820).to(dev)
    dq, dkn, dvn, dkc, dvc = (t.to(dev) for t in (q, kn, vn, kc, vc))
    o, cur = torch.full((rows, C), float("nan"), device=dev), torch.zeros(C, device=dev)
    rec = D.record(2, Tcap).to(dev)

    def body():
        check(lib.vptr_decode_begin(ptr(rec), ptr(tpos), ptr(cur), Tmax, C, stream()), "vptr_decode_begin")
        check(lib.vptr_tattn_step_pos(ptr(dq), ptr(dkn), ptr(dvn), ptr(dkc), ptr(dvc), ptr(o), ptr(rec), rows, Tcap, C, nh, 0, stream()),
              "vptr_tattn_step_pos")
        check(lib.vptr_decode_advance(ptr(rec), stream()), "vptr_decode_advance")
    body()                                                # one eager pass (loads the kernels), then everything it wrote is put back
    rec.copy_(D.record(2, Tcap)); dkc.copy_(kc); dvc.copy_(vc)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        body()
    assert graph_node_census(g) == {"kernel": 3}
    g.instantiate()
    kref, vref = kc.clone(), vc.clone()
    for pos in range(2, Tcap):
        qn, kk, vv = (fill.rand_normal((rows, C), 830 + 3 * pos + i, 0.5) for i in range(3))
        dq.copy_(qn); dkn.copy_(kk); dvn.copy_(vv)
        g.replay()
        kref[pos], vref[pos] = kk, vv
        ref = step_reference(qn, kref, vref, pos + 1, rows, Tcap, C, nh, 0)
        assert D.same_bits(o, ref), pos
        assert D.same_bits(cur, tpos[pos]), pos
        assert rec.tolist()[:4] == [pos + 1, Tcap, 0, pos - 1], pos
    assert D.same_bits(dkc, kref) and D.same_bits(dvc, vref)
    before = o.clone()
    g.replay()                                            # a full cache: refused on the device, nothing written
    assert rec.tolist()[:4] == [Tcap, Tcap, 1, Tcap - 2]
    assert D.same_bits(o, before) and D.same_bits(dkc, kref) and D.same_bits(dvc, vref)


# ------------------------------------------------------------------------------------------------------ 3. the model
CFG6 = dict(Tp=3, Tf=3, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=2, rpe=True)      # tests/test_12_far_cache_gpu.py
CFG6N = dict(CFG6, rpe=False)


@pytest.fixture(scope="module")
def far_models(pkg):
    out = {}
    for name, cfg, seed in (("rpe", CFG6, 730), ("norpe", CFG6N, 750)):
        m = build_transformer(pkg, cfg, True)
        fill.apply_fill(m, seed)
        feat = fill.rand_normal((2, cfg["Tp"] + cfg["Tf"], cfg["C"], cfg["H"], cfg["W"]), seed + 1).abs()
        out[name] = (m.to("cuda:0").eval(), feat.to("cuda:0"))
    return out


def _plain_frames(m, fd, prefill):
    cache = m.init_cache(fd.shape[0])
    outs = [m.forward_cached(fd[:, :prefill], cache)] if prefill else []
    return outs + [m.forward_cached(fd[:, t:t + 1], cache) for t in range(prefill, fd.shape[1])]


def _device_pos_frames(m, fd, prefill, replay):
    """the same sequence on a device_pos cache; replay: the single-frame steps are replays of ONE graph captured at the first of them"""
    cache = m.init_cache(fd.shape[0], device_pos=True)
    outs = [m.forward_cached(fd[:, :prefill], cache)] if prefill else []
    g, x, y = None, torch.zeros_like(fd[:, :1]), None
    for t in range(prefill, fd.shape[1]):
        if not replay:
            outs.append(m.forward_cached(fd[:, t:t + 1], cache))
        else:
            if g is None:
                m.forward_cached(x, cache)                # warm-up at this position, then rewind
                cache.len = t
                cache.put_pos(t)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    y = m.forward_cached(x, cache)
                cache.len = t
                cache.put_pos(t)
            x.copy_(fd[:, t:t + 1])
            g.replay()
            cache.len += 1
            outs.append(y.clone())
        assert cache.len == t + 1
    cache.check()
    c = cache.counters()
    assert c["pos"] == fd.shape[1] and c["overflow"] == 0
    return outs


@pytest.mark.parametrize("name", ["rpe", "norpe"])
@pytest.mark.parametrize("prefill", [0, 3])
def test_forward_cached_device_pos_matches_plain_cache(far_models, dev, name, prefill):
    m, fd = far_models[name]
    plain = _plain_frames(m, fd, prefill)
    for replay in (False, True):
        got = _device_pos_frames(m, fd, prefill, replay)
        for t, (a, b) in enumerate(zip(got, plain)):
            err = rel(a, b)
            print("device_pos %s prefill %d replay %s frame-block %d: rel %.3e" % (name, prefill, replay, t, err))
            assert a.shape == b.shape and err < TOL


def test_forward_cached_device_pos_bitwise_under_deterministic(far_models, dev):
    """torch.equal, PROVIDED two eager runs of the plain cached path are themselves bit-identical under set_deterministic(True) (the
    conv-FFN frame sums use fp32 atomics otherwise); the outcome of that premise is printed and recorded in profiles/decode_graph.md"""
    from vptr_amd import ops
    m, fd = far_models["rpe"]
    ops.set_deterministic(True)
    a, b = _plain_frames(m, fd, 3), _plain_frames(m, fd, 3)
    stable = all(torch.equal(x, y) for x, y in zip(a, b))
    print("plain cached path bit-stable under set_deterministic(True): %s" % stable)
    if not stable:
        return
    for replay in (False, True):
        got = _device_pos_frames(m, fd, 3, replay)
        assert all(torch.equal(x, y) for x, y in zip(got, a)), "replay %s" % replay


# ------------------------------------------------------------------------------------------------------ 4. rollouts
@pytest.fixture(scope="module")
def tiny(pkg):
    """the modules and inputs of tests/golden/rollouts_tiny.npz (horizon 3, five predictions: the window slides)"""
    z = load("rollouts_tiny")
    meta = jload(z, "meta")
    enc = pkg.VPTREnc(1, meta["feat"], 3, "reflect").eval()
    dec = pkg.VPTRDec(1, meta["feat"], 3, "Sigmoid", "reflect").eval()
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 1)
    far = build_transformer(pkg, jload(z, "cfg_far"), True)
    fill.apply_fill(far, meta["seed"] + 2)
    return enc.to("cuda:0"), dec.to("cuda:0"), far.to("cuda:0").eval(), torch.from_numpy(z["far_past"]).to("cuda:0"), z


@pytest.mark.parametrize("mode", ["train", "RIP", "RIL"])
def test_graph_rollout_matches_eager_cached_rollout(tiny, dev, mode):
    from vptr_amd.inference import CachedDecoder, far_rollout
    enc, dec, far, past, z = tiny
    n_pred = z["far_rip"].shape[1]
    assert n_pred > far.num_future_frames                       # past the horizon: the slide hand-over runs in 'RIP' / 'RIL'
    n_pred = min(n_pred, far.num_future_frames) if mode == "train" else n_pred      # 'train' never slides: its window is the cache
    ref = far_rollout(enc, dec, far, past, n_pred, mode=mode, kv_cache=True)
    got = far_rollout(enc, dec, far, past, n_pred, mode=mode, kv_cache=True, graph=True)
    pairs = list(zip(got, ref)) if mode == "train" else [(got, ref)]
    for a, b in pairs:
        err = rel(a, b)
        print("graph %s rollout vs eager cached: rel %.3e" % (mode, err))
        assert a.shape == b.shape and err < TOL
    if mode != "train":
        gold = z["far_rip" if mode == "RIP" else "far_ril"]
        err = rel(got, gold)
        print("graph %s rollout vs the reference's tensors: rel %.3e" % (mode, err))
        assert got.shape == tuple(gold.shape) and err < TOL
    # one decoder, two rollouts with different pasts: ONE capture, a chain of replay-safe nodes, the device record in step with the host
    d = CachedDecoder(enc, dec, far, past.shape[0], mode)
    first = d.rollout(past, n_pred)
    assert d.captures == 1 and d.graph_branches == 0 and "memset" not in d.graph_nodes and d.graph_nodes["kernel"] > 0, d.graph_nodes
    d.cache.check()
    past2 = past.flip(1).contiguous()
    second = d.rollout(past2, n_pred)
    assert d.captures == 1
    d.cache.check()
    ref2 = far_rollout(enc, dec, far, past2, n_pred, mode=mode, kv_cache=True)
    for a, b, c, e in (zip(first, ref, second, ref2) if mode == "train" else [(first, ref, second, ref2)]):
        assert rel(a, b) < TOL and rel(c, e) < TOL
    print("graph %s: nodes %s, capture %.3f s" % (mode, d.graph_nodes, d.capture_seconds))


def test_trainer_predict_graph_follows_the_weights(pkg, dev):
    """before and after a step(): the graph reads the parameter slab (and its P16 images) by address; weights='ema' swaps in place"""
    from vptr_amd import ops
    from vptr_amd.train import FARTrainer
    c = V.case("far")
    enc, dec, T, _ = V.modules(pkg, c)
    ops.manual_seed(dev, 77)
    tr = FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-2, max_grad_norm=1.0, ema_decay=0.5, ema_warmup=False)
    past, fut = (t.to(dev) for t in V.batch(c, 0))
    n_pred = min(3, tr.T.num_future_frames)

    def both(weights):
        ref = tr.predict(past, n_pred, kv_cache=True, weights=weights)
        got = tr.predict(past, n_pred, kv_cache=True, weights=weights, graph=True)
        for a, b in zip(got, ref):
            err = rel(a, b)
            print("trainer predict graph (%s): rel %.3e" % (weights, err))
            assert err < TOL
        return ref[1]
    before = both("raw")
    tr.step(past, fut)
    after = both("raw")
    assert rel(after, before) > 2 * TOL                     # the step moved the prediction, and the replays followed it
    ema = both("ema")
    assert rel(ema, after) > 0.0
    d = tr._decoders[(past.shape[0], "train")]
    assert d.captures == 1 and len(tr._decoders) == 1
    with pytest.raises(ValueError):
        tr.predict(past, n_pred, kv_cache=False, graph=True)


# ------------------------------------------------------------------------------------------------------ 5. the host's ValueErrors
def test_host_value_errors(tiny, far_models, dev):
    from vptr_amd.inference import CachedDecoder, far_rollout
    enc, dec, far, past, z = tiny
    m, fd = far_models["rpe"]
    cache = m.init_cache(fd.shape[0], device_pos=True)
    m.forward_cached(fd, cache)                                  # fills the cache to its capacity
    assert cache.len == fd.shape[1]
    with pytest.raises(ValueError):
        m.forward_cached(fd[:, :1], cache)                       # a step past Tcap: refused before any launch
    c = cache.counters()
    assert c["pos"] == cache.Tcap and c["overflow"] == 0 and c["steps"] == 0
    cache.reset()
    assert cache.counters()["pos"] == 0 and cache.len == 0
    with pytest.raises(ValueError):
        far_rollout(enc, dec, far, past, 3, kv_cache=False, graph=True)
    d = CachedDecoder(enc, dec, far, past.shape[0], "RIL")
    with pytest.raises(ValueError):
        d.rollout(past[:1], 3)                                   # another batch size than the decoder's
    d.cache.len = d.cache.Tcap
    d.graph = object()
    with pytest.raises(ValueError):
        d.step()                                                 # the replay path checks the capacity on the host as well
    far.train()
    try:
        with pytest.raises(ValueError):
            CachedDecoder(enc, dec, far, past.shape[0], "RIL")
    finally:
        far.eval()
