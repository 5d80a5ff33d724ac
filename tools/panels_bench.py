"""Sample panels (GPU box): time of vptr_clip_panels at three sizes of the reference's visualize_batch_clips call (past | future | predicted)
and what it replaces between device tensors and uint8 images on the host.

Per size, all paths produce the same bytes (asserted):
  * kernel time: durations of the `clip_panels_kernel` launches as the profiler records them (a pass of its own, `--iters` calls), and
    `--iters` eager `ops.clip_panels` calls between two device events (an upper bound: it contains the enqueue of a call);
  * achieved bytes/s = (4 bytes per clip value read once + 1 byte per output value written) / kernel time;
  * to uint8 images on the host, a host clock around `--iters` repetitions that end in a device synchronise, three ways, alternating,
    `--repeats` timings each:
      (a) kernel: `clips_to_uint8(..., to_host=True)` -- one launch, one pinned uint8 copy;
      (b) torch device ops: append_frames' cat + repeat, cat along W, the two normalisations, clamp, mul(255), byte, permute to HWC, then the
          uint8 copy from the device (what a user writes by hand today);
      (c) the reference's procedure from device tensors: cat on the device, the fp32 panel copied to the host, then per frame the two
          normalisations, clamp, mul(255).byte() and HWC on the host (the GIF encoding that follows is common to all and not timed);
  * the bytes each way moves across the bus.

    python tools/panels_bench.py [--iters 20] [--repeats 5] [--out DIR/panels_bench.json]
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
from vptr_amd import ops                                            # noqa: E402
from vptr_amd.data import BAIR_MEAN, BAIR_STD, KTH_MEAN, KTH_STD    # noqa: E402
from vptr_amd.visualize import ReNorm, clips_to_uint8               # noqa: E402

# name, N, (T_past, T_future, T_pred), (C, H, W), (mean, std)
SIZES = [("4x(10,10,10)@64x64x1", 4, (10, 10, 10), (1, 64, 64), (KTH_MEAN, KTH_STD)),
         ("16x(10,40,40)@128x128x1", 16, (10, 40, 40), (1, 128, 128), (KTH_MEAN, KTH_STD)),
         ("16x(2,28,28)@64x64x3", 16, (2, 28, 28), (3, 64, 64), (BAIR_MEAN, BAIR_STD))]


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
    """device durations (us) of the clip_panels_kernel launches of `iters` calls, from the profiler; [] if it records none"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    return [float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.events()
            if "clip_panels_kernel" in e.name and str(getattr(e, "device_type", "")).endswith("CUDA")]


def append_frames(batch, length):
    d = length - batch.shape[1]
    return batch if d == 0 else torch.cat([batch, batch[:, -2:-1].repeat(1, d, 1, 1, 1)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panels_bench: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    rows = []
    for name, N, lengths, (C, H, W), (mean, std) in SIZES:
        rs = np.random.RandomState(1)
        m = torch.tensor([mean] * C if isinstance(mean, float) else mean).view(1, 1, C, 1, 1)
        s = torch.tensor([std] * C if isinstance(std, float) else std).view(1, 1, C, 1, 1)
        clips = [torch.from_numpy(rs.randint(0, 256, size=(N, T, C, H, W)).astype(np.float32)).div(255).sub(m).div(s).to(dev) for T in lengths]
        renorm = ReNorm(mean, std)
        a, b = renorm.tensors(C, dev)
        a3, b3 = a.view(C, 1, 1), b.view(C, 1, 1)
        zero, one = torch.zeros_like(a3), torch.ones_like(a3)
        L, K = max(lengths), len(lengths)
        out = torch.empty((N, L, H, K * W, C), dtype=torch.uint8, device=dev)
        host_u8 = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)

        def kernel_only():
            ops.clip_panels(clips, a, b, out=out)

        def path_kernel():
            return clips_to_uint8(clips, renorm, to_host=True)

        def torch_device():
            x = torch.cat([append_frames(c, L) for c in clips], dim=-1)
            x = x.sub_(zero).div_(a3).sub_(b3).div_(one)
            return torch.clamp(x, 0.0, 1.0).mul(255).byte().permute(0, 1, 3, 4, 2).contiguous()

        def path_torch():
            host_u8.copy_(torch_device(), non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return host_u8.numpy()

        def path_reference():
            batch = torch.cat([append_frames(c, L) for c in clips], dim=-1).cpu()
            res = np.empty((N, L, H, K * W, C), dtype=np.uint8)
            a_h, b_h, z_h, o_h = a3.cpu(), b3.cpu(), zero.cpu(), one.cpu()
            for n in range(N):
                for t in range(L):
                    img = batch[n, t].clone().sub_(z_h).div_(a_h)
                    img = img.clone().sub_(b_h).div_(o_h)
                    res[n, t] = torch.clamp(img, 0.0, 1.0).mul(255).byte().permute(1, 2, 0).numpy()
            return res

        ref = path_reference()
        assert np.array_equal(path_kernel(), ref) and np.array_equal(path_torch(), ref), "the three ways disagree"
        kernel_only()
        wall(kernel_only, 3), wall(path_kernel, 2), wall(path_torch, 2)
        tk, tt, tr = [], [], []
        for _ in range(args.repeats):                       # alternating
            tk.append(wall(path_kernel, args.iters))
            tt.append(wall(path_torch, args.iters))
            tr.append(wall(path_reference, max(1, args.iters // 10)))
        ev = [events(kernel_only, args.iters) for _ in range(args.repeats)]
        evt = [events(torch_device, args.iters) for _ in range(args.repeats)]
        kd = sorted(kernel_durations(kernel_only, args.iters))
        in_bytes = 4 * N * sum(lengths) * C * H * W
        out_bytes = N * L * H * K * W * C
        kt = kd[len(kd) // 2] if kd else None
        row = {"size": name, "clip_bytes_fp32": in_bytes, "panel_bytes_u8": out_bytes, "bus_bytes_kernel": out_bytes, "bus_bytes_torch": out_bytes,
               "bus_bytes_reference": 4 * out_bytes,
               "kernel_us_profiler": {"n": len(kd), "min": kd[0] if kd else None, "median": kt, "max": kd[-1] if kd else None},
               "eager_call_event_us": ev, "torch_device_ops_event_us": evt,
               "achieved_bytes_per_s": ((in_bytes + out_bytes) / (kt * 1e-6)) if kt else None,
               "to_host_kernel_us": tk, "to_host_torch_ops_us": tt, "to_host_reference_us": tr}
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    print("\n| size | kernel us (profiler: min / median / max of n) | eager call, device events us (min) | clips fp32 + panel u8 | achieved bytes/s | "
          "torch device ops, device events us (min) | to host: kernel / torch ops / reference us (medians) | bus bytes: kernel, torch ops / reference |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        k = r["kernel_us_profiler"]
        print("| %s | %s | %.1f | %.1f + %.1f MB | %s | %.1f | %.0f / %.0f / %.0f | %.1f MB / %.1f MB |" % (
            r["size"], ("%.1f / %.1f / %.1f of %d" % (k["min"], k["median"], k["max"], k["n"])) if k["n"] else "not measured",
            min(r["eager_call_event_us"]), r["clip_bytes_fp32"] / 1e6, r["panel_bytes_u8"] / 1e6,
            ("%.2f TB/s" % (r["achieved_bytes_per_s"] / 1e12)) if r["achieved_bytes_per_s"] else "not measured",
            min(r["torch_device_ops_event_us"]), med(r["to_host_kernel_us"]), med(r["to_host_torch_ops_us"]), med(r["to_host_reference_us"]),
            r["bus_bytes_kernel"] / 1e6, r["bus_bytes_reference"] / 1e6))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
