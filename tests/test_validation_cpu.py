"""CPU side of the validation pass and the epoch loss meters: the host meter classes against the reference's own classes, the rank
rules of `DeviceLossMeters.compute` on a 2-rank gloo group (a host emulation of the state update behind the meter's backend seam), the
additive ABI table, and the oracle's eval-mode losses that tests/test_16_validation_gpu.py compares `eval_step` with."""
import math
import os
import random
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import validation_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- host meter classes vs the reference ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_ts():
    from oracle.ref_import import REFERENCE_ROOT, import_reference
    if not os.path.isdir(REFERENCE_ROOT):
        pytest.skip("the reference checkout is not present")
    import importlib
    before = set(sys.modules)
    import_reference()                          # registers the stand-ins the reference's `utils` package needs, then imports it
    saved = list(sys.path)
    sys.path.insert(0, REFERENCE_ROOT)
    try:
        ts = importlib.import_module("utils.train_summary")
    finally:
        sys.path[:] = saved
    assert ts.__file__.startswith(REFERENCE_ROOT)
    yield ts
    for k in set(sys.modules) - before:         # later tests must not find the reference's `utils` / `model` packages
        if k.split(".")[0] in ("utils", "model"):
            del sys.modules[k]


NAMES = ["T_total", "T_MSE", "T_GDL", "T_bpc"]


def _sequence(seed, steps=23):
    rng = random.Random(seed)
    return [{k: rng.uniform(-2.0, 5.0) * 10.0 ** rng.randint(-6, 3) for k in NAMES} for _ in range(steps)]


def test_host_meters_match_reference(ref_ts):
    from vptr_amd import meters as M
    ours, ref = M.AverageMeters(NAMES), ref_ts.AverageMeters(NAMES)
    for it in _sequence(5):
        ours.iter_update(it)
        ref.iter_update(it)
    rng = random.Random(6)
    for it in _sequence(7, steps=9):           # BatchAverageMeter.update(val, n)
        n = rng.randint(1, 16)
        for k, v in it.items():
            ours.meters[k].update(v, n)
            ref.meters[k].update(v, n)
    for k in NAMES:
        a, b = ours.meters[k], ref.meters[k]
        assert (a.val, a.avg, a.sum, a.count) == (b.val, b.avg, b.sum, b.count)
        assert str(a) == str(b) and a.name == b.name and a.fmt == b.fmt
    fresh_a, fresh_b = M.BatchAverageMeter("x"), ref_ts.BatchAverageMeter("x")
    assert str(fresh_a) == str(fresh_b)
    fresh_a.update(1.5)
    fresh_a.reset()
    assert (fresh_a.val, fresh_a.avg, fresh_a.sum, fresh_a.count) == (0, 0, 0, 0)


def test_epoch_update_matches_reference(ref_ts):
    """the KeyError branch (a history with no meter gets 0), the AttributeError branch ('epochs' is an int) and 'epochs' = epoch"""
    from vptr_amd import checkpoint as C
    from vptr_amd import meters as M
    ours, ref = M.AverageMeters(NAMES), ref_ts.AverageMeters(NAMES)
    for it in _sequence(11):
        ours.iter_update(it)
        ref.iter_update(it)
    names = NAMES + ["Dtotal"]                  # no meter of that name
    ld_a, ld_b = C.init_loss_dict(names), ref_ts.init_loss_dict(names)
    for epoch, flag in ((1, True), (1, False), (2, True)):
        ra, rb = ours.epoch_update(ld_a, epoch, train_flag=flag), ref.epoch_update(ld_b, epoch, train_flag=flag)
        assert ra is ld_a and rb is ld_b
    assert ld_a["epochs"] == ld_b["epochs"] == 2
    for k in names:
        assert ld_a[k].train == ld_b[k].train and ld_a[k].val == ld_b[k].val
    assert ld_a["Dtotal"].train == [0, 0] and ld_a["Dtotal"].val == [0]
    assert C.AverageMeters is M.AverageMeters and C.BatchAverageMeter is M.BatchAverageMeter
    assert C.gather_AverageMeters is M.gather_AverageMeters


def test_gather_average_meters_matches_reference(ref_ts):
    from vptr_amd import meters as M
    ours, refs = [], []
    for r in range(3):
        a, b = M.AverageMeters(NAMES), ref_ts.AverageMeters(NAMES)
        for it in _sequence(20 + r, steps=5 + r):
            a.iter_update(it)
            b.iter_update(it)
        ours.append(a)
        refs.append(b)
    ga, gb = M.gather_AverageMeters(ours), ref_ts.gather_AverageMeters(refs)
    assert ga.loss_name_list == gb.loss_name_list
    for k in NAMES:
        assert ga.meters[k].avg == gb.meters[k].avg
        assert str(ga.meters[k]) == str(gb.meters[k])


# ---- DeviceLossMeters on the host backend ----------------------------------------------------------------------------------------
def _rank_values(rank):
    rng = random.Random(300 + rank)
    return [{"a": torch.tensor(rng.uniform(0.0, 3.0), dtype=torch.float32), "b": torch.tensor(rng.uniform(-1.0, 1.0), dtype=torch.float32)}
            for _ in range(4 + 3 * rank)]          # the ranks hold different numbers of batches


def test_device_meters_host_backend():
    from vptr_amd.meters import DeviceLossMeters
    m = DeviceLossMeters(["a", "b", "c"], "cpu", add=V.host_add)
    recs = {k: V.HostRecord() for k in "ab"}
    for i, it in enumerate(_rank_values(0)):
        n = 1 if i % 2 else 4
        m.update(dict(it, grad_norm=torch.tensor(1.0)), n=n)     # 'grad_norm' is ignored by default
        for k, t in it.items():
            recs[k].add(float(t), float(n))
    out = m.compute()
    for k in "ab":
        r = recs[k]
        assert out[k]["sum"] == r.sum and out[k]["count"] == r.count and out[k]["last"] == r.last and out[k]["nonfinite"] == 0
        assert out[k]["avg"] == r.sum / r.count
        assert abs(out[k]["std"] - math.sqrt(max(r.sumsq / r.count - (r.sum / r.count) ** 2, 0.0))) <= 1e-12
    assert out["c"] == {"avg": 0, "sum": 0.0, "count": 0.0, "std": 0.0, "last": 0.0, "nonfinite": 0}
    with pytest.raises(KeyError):
        m.update({"nope": torch.tensor(1.0)})
    with pytest.raises(TypeError):
        m.update({"a": torch.tensor(1.0, dtype=torch.float64)})
    with pytest.raises(TypeError):
        m.update({"a": 1.0})
    with pytest.raises(ValueError):
        m.update({"a": torch.tensor(1.0)}, n=0)
    with pytest.raises(ValueError):
        DeviceLossMeters(["n%d" % i for i in range(17)], "cpu", add=V.host_add)
    m.update({"b": torch.tensor(float("nan"))})
    out = m.compute()
    assert out["b"]["nonfinite"] == 1 and math.isnan(out["b"]["avg"]) and math.isfinite(out["a"]["avg"])
    m.reset()
    assert float(m.state.abs().sum()) == 0.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _meter_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vptr_amd.checkpoint import init_loss_dict
    from vptr_amd.meters import DeviceLossMeters
    m = DeviceLossMeters(["a", "b"], "cpu", add=V.host_add)
    for it in _rank_values(rank):
        m.update(it)
    res = {"mean": m.compute(dist.group.WORLD), "samples": m.compute(dist.group.WORLD, across="samples"), "own": m.compute()}
    ld = m.epoch_update(init_loss_dict(["a", "b", "zz"]), 3, train_flag=False, group=dist.group.WORLD)
    res["epoch"] = {k: (v if k == "epochs" else (v.train, v.val)) for k, v in ld.items()}
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_device_meters_compute_across_two_ranks_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_meter_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    vals = [_rank_values(r) for r in range(world)]
    for k in "ab":
        per_rank = [[float(it[k]) for it in v] for v in vals]
        sums = []
        for xs in per_rank:
            s = 0.0
            for x in xs:
                s += x
            sums.append(s)
        counts = [float(len(xs)) for xs in per_rank]
        mean_of_avgs = (sums[0] / counts[0] + sums[1] / counts[1]) / 2          # gather_AverageMeters' rule
        pooled = (sums[0] + sums[1]) / (counts[0] + counts[1])
        assert mean_of_avgs != pooled                                            # unequal shards: the two rules differ
        for r in range(world):
            assert res[r]["mean"][k]["avg"] == mean_of_avgs
            assert res[r]["samples"][k]["avg"] == pooled and res[r]["samples"][k]["count"] == counts[0] + counts[1]
            assert res[r]["own"][k]["avg"] == sums[r] / counts[r] and res[r]["mean"][k]["count"] == counts[r]
            assert res[r]["epoch"][k] == ([], [mean_of_avgs])
    for r in range(world):
        assert res[r]["epoch"]["zz"] == ([], [0]) and res[r]["epoch"]["epochs"] == 3


# ---- the additive ABI table ------------------------------------------------------------------------------------------------------
def test_ext_signatures_match_header_and_library():
    from vptr_amd import _lib
    text = open(os.path.join(ROOT, "include", "vptr_hip_ext.h")).read()
    assert '#include "vptr_hip.h"' in text
    declared = set(re.findall(r"\b(vptr_\w+)\s*\(", text))
    assert declared == set(_lib.EXT_SIGNATURES) == {"vptr_meters_add"}
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.EXPORTS)
    for name, argt in _lib.EXT_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == argt and fn.restype is _lib.c_int
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    from vptr_amd.build import SOURCES
    assert "meters.hip" in SOURCES


def test_meters_add_rejects_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device"""
    import ctypes
    from vptr_amd import _lib
    fn = _lib.lib.vptr_meters_add
    src = (ctypes.c_void_p * 16)()
    state = (ctypes.c_double * 17)()
    base = ctypes.addressof(state)
    bad = [(src, 0, base, 1.0), (src, 17, base, 1.0), (src, -1, base, 1.0), (None, 1, base, 1.0), (src, 1, None, 1.0),
           (src, 1, base + 4, 1.0), (src, 1, base, 0.0), (src, 1, base, -1.0), (src, 1, base, float("nan")), (src, 1, base, float("inf"))]
    for s, K, st, w in bad:
        assert fn(s, K, st, w, None) != 0, (K, st, w)
        assert _lib.lib.vptr_last_error().decode().startswith("meters_add")


# ---- the oracle's validation pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nar_gan", "ae"])
def test_oracle_eval_losses_reproducible_and_mode_sensitive(kind):
    """eval-mode losses are a function of (parameters, buffers, batch) alone, and differ from the train-mode ones where BatchNorm
    changes mode: the GPU cases can tell an `eval_step` that forgot `.eval()` from a correct one"""
    import vptr_amd.model as pkg
    c = V.case(kind)
    enc, dec, T, disc = V.modules(pkg, c)
    st = dict(enc=enc.state_dict(), dec=dec.state_dict(), T=T.state_dict() if T is not None else None, disc=disc.state_dict())
    past, fut = V.batch(c, 0)
    a, b = V.oracle_eval(c, st, past, fut), V.oracle_eval(c, st, past, fut)
    assert a == b
    t = V.oracle_eval(c, st, past, fut, training=True)
    assert set(t) == set(a)
    tol = 1e-3      # the bar of the GPU comparison: TOL * |ref| + 1e-6
    moved = [k for k in a if abs(t[k] - a[k]) > 4 * (tol * abs(a[k]) + 1e-6)]
    assert {"Dfake", "Dreal"} <= set(moved), (a, t)               # (their mean, Dtotal, can stay: the two may move against each other)
    if kind == "ae":
        assert {"AE_MSE", "AE_GDL", "AE_total"} <= set(moved), (a, t)
    else:
        # the NAR conv-FFNs hold BatchNorm too, but on this configuration their mode moves the frame losses by ~1e-3 only: a
        # transformer left in train mode is caught by the running statistics it updates (the GPU file's non-interference cases)
        assert "T_gan" in moved and t["T_GDL"] != a["T_GDL"] and t["T_MSE"] != a["T_MSE"], (a, t)
