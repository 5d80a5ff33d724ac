"""Clip ingest (GPU box): time of vptr_clip_ingest at the batches of the bench configurations (per-GPU batch 16) and what it buys
between pinned host memory and device tensors.

Per batch:
  * kernel time: durations of the `clip_ingest_kernel` launches as the profiler records them (a pass of its own, `--iters` calls), and
    for comparison `--iters` eager calls between two device events (an upper bound: it contains the enqueue of a call);
  * achieved bytes/s = (cropped uint8 bytes read once + 4 bytes per output value written) / kernel time;
  * host -> device tensors, a host clock around `--iters` batches that end in a device synchronise, two ways, alternating, 5 timings
    each: (a) the uint8 batch uploaded from pinned memory, then the kernel; (b) the same batch already transformed, uploaded as fp32
    (past, future) from pinned memory -- what a user does without the kernel, host preparation NOT counted.

    python tools/ingest_bench.py [--iters 50] [--repeats 5] [--out DIR/ingest_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from vptr_amd import ops                                # noqa: E402
from vptr_amd.data import ClipIngest, IngestPlan        # noqa: E402

# name, plan constructor, (N, Tp, Tf): KTH 10 -> 10 @64, KTH 10 -> 40 @128, BAIR 2 -> 28
BATCHES = [("kth64", lambda d: IngestPlan.kth(64, device=d), (16, 10, 10)),
           ("kth128", lambda d: IngestPlan.kth(128, device=d), (16, 10, 40)),
           ("bair", lambda d: IngestPlan.bair(device=d), (16, 2, 28))]


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_durations(fn, iters):
    """device durations (us) of the clip_ingest_kernel launches of `iters` calls, from the profiler; [] if it records none"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    return [float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.events()
            if "clip_ingest_kernel" in e.name and str(getattr(e, "device_type", "")).endswith("CUDA")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    rows = []
    for name, make, (N, Tp, Tf) in BATCHES:
        plan = make(dev)
        (Hin, Win), C, (Hout, Wout) = plan.in_hw, plan.channels, plan.out_hw
        T = Tp + Tf
        raw_h = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(N, T, Hin, Win, C)).astype(np.uint8)).pin_memory()
        raw_d = raw_h.to(dev)
        ingest = ClipIngest(plan, Tp, Tf)
        past, future = ingest(raw_d)
        past_h, future_h = past.cpu().pin_memory(), future.cpu().pin_memory()      # the batch as a user holds it without the kernel
        outs = (torch.empty_like(past), torch.empty_like(future))

        def kernel_only():
            ops.ingest_clips(raw_d, plan, split=Tp, out=outs)

        def path_u8():
            return ingest(raw_h)

        def path_f32():
            return past_h.to(dev, non_blocking=True), future_h.to(dev, non_blocking=True)

        kernel_only(), path_u8(), path_f32()
        wall(kernel_only, 5), wall(path_u8, 5), wall(path_f32, 5)
        a, b = path_u8(), path_f32()
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        tu, tf = [], []
        for _ in range(args.repeats):                       # alternating
            tu.append(wall(path_u8, args.iters))
            tf.append(wall(path_f32, args.iters))
        ev = [events(kernel_only, args.iters) for _ in range(args.repeats)]
        kd = sorted(kernel_durations(kernel_only, args.iters))
        _, _, Hc, Wc = plan.crop
        nbytes = N * T * (Hc * Wc * C + 4 * C * Hout * Wout)
        kt = kd[len(kd) // 2] if kd else None
        row = {"batch": name, "raw_shape": [N, T, Hin, Win, C], "out_hw": [Hout, Wout], "bytes": nbytes,
               "upload_bytes_u8": N * T * Hin * Win * C, "upload_bytes_f32": 4 * N * T * C * Hout * Wout,
               "kernel_us_profiler": {"n": len(kd), "min": kd[0] if kd else None, "median": kt, "max": kd[-1] if kd else None},
               "eager_call_event_us": ev, "achieved_bytes_per_s": (nbytes / (kt * 1e-6)) if kt else None,
               "pinned_u8_upload_plus_kernel_us": tu, "pinned_f32_upload_us": tf}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| batch | raw (N,T,H,W,C) -> out | kernel us (profiler: min / median / max of n) | eager call, device events us (min of 5) | bytes | "
          "achieved bytes/s | uint8 upload + kernel us (5 timings) | fp32 upload us (5 timings) | ratio of medians |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        k = r["kernel_us_profiler"]
        mu, mf = sorted(r["pinned_u8_upload_plus_kernel_us"])[args.repeats // 2], sorted(r["pinned_f32_upload_us"])[args.repeats // 2]
        print("| %s | %s -> %s | %s | %.1f | %.1f MB | %s | %s | %s | %.2fx |" % (
            r["batch"], tuple(r["raw_shape"]), tuple(r["out_hw"]),
            ("%.1f / %.1f / %.1f of %d" % (k["min"], k["median"], k["max"], k["n"])) if k["n"] else "not measured", min(r["eager_call_event_us"]),
            r["bytes"] / 1e6, ("%.2f TB/s" % (r["achieved_bytes_per_s"] / 1e12)) if r["achieved_bytes_per_s"] else "not measured",
            " ".join("%.0f" % v for v in r["pinned_u8_upload_plus_kernel_us"]), " ".join("%.0f" % v for v in r["pinned_f32_upload_us"]), mf / mu))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
