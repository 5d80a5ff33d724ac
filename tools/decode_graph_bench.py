"""Measurements behind profiles/decode_graph.md (GPU box): FAR rollouts un-cached, KV-cached and KV-cached with the captured step graph
(`far_rollout(kv_cache=True, graph=...)`), alternating in one session; vptr_tattn_step_pos against vptr_tattn_step at the BAIR geometry;
the node census and capture time of the three step graphs.

    python tools/decode_graph_bench.py [--repeat 5] [--only rollouts|kernel|census] [--json FILE]

Per rollout call three clocks: `gpu` (events around the call), `host` (perf_counter until the call RETURNS, before any synchronisation:
the time the host needs to issue the call's work -- prefill, per-frame loop and final decoder pass) and `wall` (until the device is idle)."""
import argparse, contextlib, io, json, os, sys, time
import numpy as np
import torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import vptr_amd.model as M
from vptr_amd._lib import check, lib, ptr, stream
from vptr_amd.inference import CachedDecoder, far_rollout

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--only", choices=("rollouts", "kernel", "census"), default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
result = {}


def frames(n, t, c, seed):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.uniform(0, 1, size=(n, t, c, 64, 64)).astype(np.float32)).to(dev)


def clocks(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return {"gpu": e0.elapsed_time(e1), "host": host * 1e3, "wall": wall * 1e3}


def stats(xs):
    xs = sorted(xs)
    med = float(np.median(xs))
    return {"median": med, "min": xs[0], "max": xs[-1], "spread": xs[-1] - xs[0], "all": xs}


def rollouts(name, enc, dec, far, past, num_pred):
    far.eval()
    d = CachedDecoder(enc, dec, far, past.shape[0], "train")
    variants = {"kv_cache=False": lambda: far_rollout(enc, dec, far, past, num_pred),
                "kv_cache=True": lambda: far_rollout(enc, dec, far, past, num_pred, kv_cache=True),
                "kv_cache=True, graph": lambda: far_rollout(enc, dec, far, past, num_pred, kv_cache=True, graph=d)}
    for fn in variants.values():     # warm-up; the graph variant captures here
        fn()
    ref = variants["kv_cache=True"]()[1].double()
    got = variants["kv_cache=True, graph"]()[1].double()
    runs = {k: [] for k in variants}
    for _ in range(args.repeat):     # alternating
        for k, fn in variants.items():
            runs[k].append(clocks(fn))
    out = {"graph_nodes": d.graph_nodes, "capture_seconds": d.capture_seconds, "captures": d.captures,
           "graph_vs_eager_cached_rel_l2": float((got - ref).norm() / ref.norm())}
    print("\n%s (%d timings each, alternating; ms)" % (name, args.repeat))
    for k in variants:
        out[k] = {c: stats([r[c] for r in runs[k]]) for c in ("gpu", "host", "wall")}
        print("  %-22s " % k + "  ".join("%s median %9.2f [%9.2f .. %9.2f]" % (c, out[k][c]["median"], out[k][c]["min"], out[k][c]["max"])
                                        for c in ("gpu", "host", "wall")))
    e, g = out["kv_cache=True"]["wall"], out["kv_cache=True, graph"]["wall"]
    out["gain_ms"], out["eager_spread_ms"] = e["median"] - g["median"], e["spread"]
    out["accepted"] = bool(out["gain_ms"] > out["eager_spread_ms"])
    print("  graph faster than the eager cached rollout by %.2f ms (wall medians); run-to-run spread of the eager cached rollout %.2f ms -> %s"
          % (out["gain_ms"], out["eager_spread_ms"], "ACCEPTED" if out["accepted"] else "NOT faster by more than the spread"))
    print("  graph: %s, captured in %.3f s, %d capture(s); rel-L2 to the eager cached frames %.2e"
          % (d.graph_nodes, d.capture_seconds, d.captures, out["graph_vs_eager_cached_rel_l2"]))
    result[name] = out


def census():
    """the three step graphs of the tiny test model and of the BAIR model at batch 16"""
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        enc = M.VPTREnc(3, 528, 3, "zero").to(dev).eval(); dec = M.VPTRDec(3, 528, 3, "Tanh", "zero").to(dev).eval()
        M.init_weights(enc); M.init_weights(dec)
    far = M.VPTRFormerFAR(2, 28, 8, 8, 528, 8, 12, 0.1, 4, 4, True).to(dev).eval()
    past = frames(16, 2, 3, 6)
    print("\nstep graphs, BAIR model (12 layers) at batch 16")
    for mode in ("RIL", "RIP", "train"):
        d = CachedDecoder(enc, dec, far, 16, mode)
        with torch.no_grad():
            d.rollout(past, 4)
        out[mode] = {"nodes": d.graph_nodes, "branches": d.graph_branches, "capture_seconds": d.capture_seconds}
        print("  %-5s %s, %d nodes with parallel branches, captured in %.3f s (warm-up passes included)" % (mode, d.graph_nodes, d.graph_branches, d.capture_seconds))
        del d
    result["census"] = out


def kernel():
    C, nh, L, rows, Tcap = 528, 8, 12, 16 * 64, 30
    q, o = torch.randn(rows, C, device=dev), torch.empty(rows, C, device=dev)
    kn, vn = torch.randn(rows, C, device=dev), torch.randn(rows, C, device=dev)
    ks = [torch.randn(Tcap, rows, C, device=dev) for _ in range(L)]       # twelve caches in turn, as the layers visit them
    vs = [torch.randn(Tcap, rows, C, device=dev) for _ in range(L)]
    rec = torch.zeros(16, device=dev, dtype=torch.int32)
    rec[1] = Tcap

    def timed(fn, n=10 * L):
        for i in range(L):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    out = {}
    print("\nvptr_tattn_step_pos against vptr_tattn_step, rows %d, C %d, %d heads (us per call, %d timings each, alternating)" % (rows, C, nh, args.repeat))
    for Tk in (3, 15, 29):
        rec[0:1].fill_(Tk - 1)
        step = lambda i: check(lib.vptr_tattn_step(ptr(q), ptr(ks[i % L]), ptr(vs[i % L]), ptr(o), rows, Tk, Tcap, C, nh, 1, stream()), "vptr_tattn_step")
        pos = lambda i: check(lib.vptr_tattn_step_pos(ptr(q), ptr(kn), ptr(vn), ptr(ks[i % L]), ptr(vs[i % L]), ptr(o), ptr(rec), rows, Tcap, C, nh, 1,
                                                      stream()), "vptr_tattn_step_pos")
        a, b = [], []
        for _ in range(args.repeat):
            a.append(timed(step)); b.append(timed(pos))
        sa, sb = stats(a), stats(b)
        by_a, by_b = 2.0 * Tk * rows * C * 4, 2.0 * (Tk + 1) * rows * C * 4      # pos: Tk - 1 slots + staging read, one slot written
        ratio = sb["median"] / sa["median"]
        bar = (Tk + 2.0) / (Tk + 1.0) + sa["spread"] / sa["median"]
        out[Tk] = {"step_us": sa, "pos_us": sb, "step_TBps": by_a / sa["median"] / 1e6, "pos_TBps": by_b / sb["median"] / 1e6, "ratio": ratio,
                   "bytes_ratio": by_b / by_a, "bar": bar, "step_rel_spread": sa["spread"] / sa["median"], "within_bar": bool(ratio <= bar)}
        print("  Tk %2d: step %7.1f us [%7.1f .. %7.1f] %5.2f TB/s | pos %7.1f us [%7.1f .. %7.1f] %5.2f TB/s | time ratio %.3f, byte ratio (Tk+1)/Tk %.3f, "
              "bar (Tk+2)/(Tk+1) + spread = %.3f + %.3f -> %s"
              % (Tk, sa["median"], sa["min"], sa["max"], out[Tk]["step_TBps"], sb["median"], sb["min"], sb["max"], out[Tk]["pos_TBps"], ratio,
                 by_b / by_a, (Tk + 2.0) / (Tk + 1.0), sa["spread"] / sa["median"], "within" if ratio <= bar else "ABOVE"))
    result["kernel"] = out


torch.manual_seed(0)
if args.only in (None, "kernel"):
    kernel()
if args.only in (None, "census"):
    census()
if args.only in (None, "rollouts"):
    with contextlib.redirect_stdout(io.StringIO()):
        enc = M.VPTREnc(1, 528, 3).to(dev).eval(); dec = M.VPTRDec(1, 528, 3, out_layer="Sigmoid").to(dev).eval()
        M.init_weights(enc); M.init_weights(dec)
    far = M.VPTRFormerFAR(10, 10, 8, 8, 528, 8, 12, 0.1, 4, 4, False).to(dev)
    rollouts("FAR rollout 10->10 batch 8", enc, dec, far, frames(8, 10, 1, 5), 10)
    del far, enc, dec
    with contextlib.redirect_stdout(io.StringIO()):
        enc3 = M.VPTREnc(3, 528, 3, "zero").to(dev).eval(); dec3 = M.VPTRDec(3, 528, 3, "Tanh", "zero").to(dev).eval()
        M.init_weights(enc3); M.init_weights(dec3)
    bair = M.VPTRFormerFAR(2, 28, 8, 8, 528, 8, 12, 0.1, 4, 4, True).to(dev)
    rollouts("FAR rollout 2->28 batch 16", enc3, dec3, bair, frames(16, 2, 3, 6), 28)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1, default=str)
