"""Scoring one batch of a rollout (GPU box): the kernel path (FrameMetrics.update = vptr_frame_metrics + vptr_frame_metrics_accumulate, one
read-back at the end) against the loop over time indices built on vptr_amd.metrics with `.item()` after every call -- what an evaluation
had to do before the kernel existed (utils/metrics.py:108-137 calls one metric per pass; the notebook runs the three of them).

Per shape: 5 timings of each path, alternating, each a host clock around `--iters` batches that end in a device synchronise; the time of
the two kernel launches alone from device events; device launches per batch counted by the profiler in a pass of their own; achieved
bytes/s of the kernel with bytes = 2 * 4 * N*T*C*H*W (one read of both operands).

    python tools/metrics_bench.py [--iters 20] [--loop-iters 3] [--out DIR/metrics_bench.json]
"""
import argparse
import json
import os
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from vptr_amd import metrics as Mx          # noqa: E402
from vptr_amd import ops                    # noqa: E402
from vptr_amd.evaluate import FrameMetrics  # noqa: E402

SHAPES = [(16, 10, 1, 64, 64), (16, 28, 3, 64, 64), (16, 40, 1, 128, 128)]
KTH = (0.6013795, 2.7570653)
BAIR = ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673))


def parent_loop(pred, gt, mean_t, std_t, ssim, sums):
    """the evaluation loop on vptr_amd.metrics: per time index renormalise, then three metric calls, each ending in .item()"""
    N = pred.shape[0]
    for t in range(pred.shape[1]):
        a, b = pred[:, t] * std_t + mean_t, gt[:, t] * std_t + mean_t
        sums[t][0] += Mx.PSNR(a, b) * N
        sums[t][1] += Mx.MSEScore(a, b) * N
        sums[t][2] += float(ssim(a, b)) * N


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


def launches(fn):
    """device kernels + memcpys / memsets of one call, from the profiler (None if it records no device activity)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        N, T, C, H, W = shape
        mean, std = KTH if C == 1 else BAIR
        g = torch.Generator(device="cpu").manual_seed(1)
        img = torch.rand(shape, generator=g)
        tgt = 0.8 * img + 0.2 * torch.rand(shape, generator=g)
        m, s = torch.tensor(mean).reshape(1, 1, -1, 1, 1), torch.tensor(std).reshape(1, 1, -1, 1, 1)
        pred, gt = ((img - m) / s).to(dev), ((tgt - m) / s).to(dev)
        mean_t, std_t = m[0].to(dev), s[0].to(dev)          # [1, C, 1, 1] against (N, C, H, W)
        mean_c, std_c = mean_t.reshape(-1).expand(C).contiguous(), std_t.reshape(-1).expand(C).contiguous()
        ssim = Mx.SSIM().to(dev)
        fm = FrameMetrics(T, mean, std, device=dev)
        sums = [[0.0, 0.0, 0.0] for _ in range(T)]

        def kernel_path():
            fm.update(pred, gt)

        def kernel_only():
            ops.frame_metrics(pred, gt, mean_c, std_c)

        def loop_path():
            parent_loop(pred, gt, mean_t, std_t, ssim, sums)

        kernel_path(), kernel_only(), loop_path()           # warm-up of every path
        wall(kernel_path, 3), wall(loop_path, 1)
        tk, tl = [], []
        for _ in range(args.repeats):                       # alternating
            tk.append(wall(kernel_path, args.iters))
            tl.append(wall(loop_path, args.loop_iters))
        ev = [events(kernel_only, args.iters) for _ in range(args.repeats)]
        nk, nl = launches(kernel_path), launches(loop_path)
        # same numbers from both paths (how far apart: profiles/frame_metrics.md)
        fm.reset()
        fm.update(pred, gt)
        res = fm.compute()
        chk = [[0.0, 0.0, 0.0] for _ in range(T)]
        parent_loop(pred, gt, mean_t, std_t, ssim, chk)
        chk = torch.tensor(chk, dtype=torch.float64) / N
        diff = {"psnr_dB": float((torch.from_numpy(res["psnr"]) - chk[:, 0]).abs().max()),
                "mse_rel": float(((torch.from_numpy(res["mse"]) - chk[:, 1]).abs() / chk[:, 1]).max()),
                "ssim": float((torch.from_numpy(res["ssim"]) - chk[:, 2]).abs().max())}
        nbytes = 2 * 4 * N * T * C * H * W
        row = {"shape": list(shape), "bytes": nbytes, "kernel_path_us": tk, "parent_loop_us": tl, "two_launches_event_us": ev,
               "launches_kernel_path": nk, "launches_parent_loop": nl, "host_syncs_parent_loop": 3 * T,
               "achieved_bytes_per_s": nbytes / (min(ev) * 1e-6), "max_difference_between_paths": diff}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| shape (N,T,C,H,W) | kernel path us (5 timings) | parent-style loop us (5 timings) | speed-up (medians) | launches kernel / loop | "
          "two launches, device events us (min) | achieved bytes/s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        mk, ml = sorted(r["kernel_path_us"])[len(r["kernel_path_us"]) // 2], sorted(r["parent_loop_us"])[len(r["parent_loop_us"]) // 2]
        print("| %s | %s | %s | %.0fx | %s / %s | %.1f | %.3g TB/s |" % (
            tuple(r["shape"]), " ".join("%.0f" % v for v in r["kernel_path_us"]), " ".join("%.0f" % v for v in r["parent_loop_us"]), ml / mk,
            r["launches_kernel_path"] or "not measured", r["launches_parent_loop"] or "not measured", min(r["two_launches_event_us"]),
            r["achieved_bytes_per_s"] / 1e12))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
