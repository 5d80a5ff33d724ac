"""Epoch loop (GPU box): what the on-device loss meters and the validation pass cost on the K64 NAR configuration of bench.py (batch 16,
dropout 0.1, hipGraph replays), the numbers of profiles/validation.md.

Per repeat, alternating, a host clock around `--steps` iterations that end in a device synchronise:
  (a) the reference's procedure: `step()` and `.item()` on every returned term, each iteration (train_NAR.py:105);
  (b) `step(..., meters=m)` each iteration, one `m.compute()` at the end;
  (c) `eval_step` eager, (d) `eval_step` as replays of the `capture_eval` graph, both with `meters=` and one `compute()`;
  (e) `vptr_meters_add` alone: device events around 1000 `update()` calls on the step's static outputs.
The state is restored in front of every timing, so all of them run the same trajectory.

    python tools/epoch_bench.py [--steps 200] [--repeats 3] [--out DIR/epoch_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench                                              # noqa: E402
from vptr_amd.meters import DeviceLossMeters              # noqa: E402

NAMES = ["T_total", "T_GDL", "T_MSE", "T_bpc"]


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    enc, dec, T, cls, kw, past, fut, workload = bench.build_job("k64", dev, 0.1, bench.JOBS["k64"]["batch"], 0)
    tr = cls(enc, dec, T, lr=1e-4, max_grad_norm=1.0, **kw)
    snap = tr._snapshot()
    tr.capture(past, fut, warmup=2)
    tr.capture_eval(past, fut)
    tr._restore(snap)
    train_graph, eval_graph = tr._graph, tr._eval_graph

    def items(n):
        for _ in range(n):
            out = tr.step(past, fut)
            for v in out.values():
                v.item()

    def metered(n):
        m = DeviceLossMeters(NAMES, dev)
        for _ in range(n):
            tr.step(past, fut, meters=m)
        m.compute()

    def evaluate(n):
        m = DeviceLossMeters(NAMES, dev)
        for _ in range(n):
            tr.eval_step(past, fut, meters=m)
        m.compute()

    rows = {"a_item_per_term": [], "b_meters": [], "c_eval_eager": [], "d_eval_replay": []}
    for _ in range(args.repeats):
        for key, fn, eg in (("a_item_per_term", items, eval_graph), ("b_meters", metered, eval_graph), ("c_eval_eager", evaluate, None),
                            ("d_eval_replay", evaluate, eval_graph)):
            tr._restore(snap)
            tr._graph, tr._eval_graph = train_graph, eg
            fn(3)
            rows[key].append(timed(fn, args.steps))
    tr._graph, tr._eval_graph = train_graph, eval_graph
    m = DeviceLossMeters(NAMES, dev)
    out = tr.step(past, fut)
    m.update(out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(1000):
        m.update(out)
    e1.record()
    torch.cuda.synchronize()
    res = {"workload": workload, "steps": args.steps, "repeats": args.repeats, "ms_per_iteration": rows,
           "e_meters_add_us_per_call": e0.elapsed_time(e1), "eval_graph_nodes": tr.eval_graph_nodes}
    a, b = rows["a_item_per_term"], rows["b_meters"]
    res["b_minus_a_ms"] = sum(b) / len(b) - sum(a) / len(a)
    res["spread_ms"] = max(max(a) - min(a), max(b) - min(b))
    res["b_not_slower_than_a"] = res["b_minus_a_ms"] <= res["spread_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
