"""Optimizer controls (GPU box): what `vptr_optim_prepare` + `vptr_adamw_ctl` cost against `vptr_adamw`, the numbers of profiles/optim_ctl.md.

  (a) kernels alone on a slab of the K64 transformer's size (118 368 576 floats: p, g, m, v = 1.9 GB): device events around one
      `vptr_adamw` call and around one `vptr_optim_prepare` + `vptr_adamw_ctl` pair, alternating in one process, clip active;
  (b) the same pair on a skipped step (sumsq = NaN, skip_nonfinite = 1): what a bad batch costs in the optimizer;
  (c) the captured K64 step of bench.py's configuration (batch 16, dropout 0.1) with a cosine schedule + skip_nonfinite against the
      uncontrolled captured step: two trainers in one process, alternating blocks of replays, a host clock around blocks that end in a
      device synchronise.
Medians, and the spread as min .. max, over `--repeats` samples each.

    python tools/optim_ctl_bench.py [--repeats 30] [--block 20] [--no-step] [--out DIR/optim_ctl_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench                                              # noqa: E402
from vptr_amd._lib import check, lib, ptr, stream          # noqa: E402
from vptr_amd.optim import LRSchedule, OptimControls       # noqa: E402

SLAB = 118368576


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def kernels(dev, repeats):
    n = SLAB
    p, m = torch.randn(n, device=dev) * 0.02, torch.zeros(n, device=dev)
    v, g = torch.zeros(n, device=dev), torch.randn(n, device=dev) * 1e-3
    sumsq = (g.double() ** 2).sum().float().reshape(1)
    nan = torch.full((1,), float("nan"), device=dev)
    step_a, step_b, step_c = (torch.zeros(1, device=dev) for _ in range(3))
    ctl = OptimControls(dev, 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0, LRSchedule("cosine", 100, 100000, 0.01), False)
    ctl_skip = OptimControls(dev, 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0, None, True)

    def plain():
        step_a.add_(1.0)
        check(lib.vptr_adamw(ptr(p), ptr(g), ptr(m), ptr(v), n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, ptr(step_a), ptr(sumsq), 1.0, 1.0, stream()), "vptr_adamw")

    def controlled():
        ctl.prepare(step_b, sumsq)
        ctl.update(p, g, m, v, n)

    def skipped():
        ctl_skip.prepare(step_c, nan)
        ctl_skip.update(p, g, m, v, n)

    rows = {"adamw_us": [], "prepare_adamw_ctl_us": [], "skipped_us": []}
    fns = (("adamw_us", plain), ("prepare_adamw_ctl_us", controlled), ("skipped_us", skipped))
    for _, fn in fns:
        for _ in range(3):
            fn()
    for _ in range(repeats):
        for key, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            rows[key].append(e0.elapsed_time(e1) * 1e3)
    assert float(step_c) == 0.0 and float(ctl_skip.word(3)) == repeats + 3
    out = {k: summary(x) for k, x in rows.items()}
    out["bytes_moved"] = 7 * 4 * n
    out["adamw_TBps"] = 7 * 4 * n / (out["adamw_us"]["median"] * 1e-6) / 1e12
    out["adamw_ctl_TBps"] = 7 * 4 * n / (out["prepare_adamw_ctl_us"]["median"] * 1e-6) / 1e12
    return out


def captured_step(dev, repeats, block):
    trainers = {}
    for key, kw_ctl in (("uncontrolled", {}), ("controlled", dict(schedule=LRSchedule("cosine", 100, 100000, 0.01), skip_nonfinite=True))):
        enc, dec, T, cls, kw, past, fut, workload = bench.build_job("k64", dev, 0.1, bench.JOBS["k64"]["batch"], 0)
        tr = cls(enc, dec, T, lr=1e-4, max_grad_norm=1.0, **kw, **kw_ctl)
        tr.capture(past, fut, warmup=3)
        trainers[key] = (tr, past, fut)
    rows = {k: [] for k in trainers}
    for tr, past, fut in trainers.values():
        for _ in range(5):
            tr.step(past, fut)
    for _ in range(repeats):
        for key, (tr, past, fut) in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                tr.step(past, fut)
            torch.cuda.synchronize()
            rows[key].append((time.perf_counter() - t0) * 1e3 / block)
    out = {k + "_ms_per_step": summary(x) for k, x in rows.items()}
    out["graph_nodes"] = {k: t[0].graph_nodes for k, t in trainers.items()}
    out["workload"], out["block"] = workload, block
    tr = trainers["controlled"][0]
    out["controlled_last"] = {"lr": float(tr.opt.lr_now()), "skipped": float(tr.opt.skipped()), "step": float(tr.opt.step_dev)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_ctl_bench: no GPU; these numbers are measured on an MI355X or not at all")
    dev = torch.device("cuda:0")
    res = {"slab_floats": SLAB, "kernels": kernels(dev, args.repeats)}
    torch.cuda.empty_cache()
    if not args.no_step:
        res["captured_step"] = captured_step(dev, max(5, args.repeats // 3), args.block)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
