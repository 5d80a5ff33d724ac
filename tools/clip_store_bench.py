"""HBM-resident clip store (GPU box): what drawing and gathering a batch on the device costs, next to the dense ingest and next to a
host-side batch.  One session, one box; alternatives alternate, `--repeats` timings each.

  1. kernel time of `clip_ingest_gather_kernel` on clips drawn from a store against `clip_ingest_kernel` on the same frames laid out
     densely, at the three batches of profiles/ingest.md: device durations of `--iters` launches as the profiler records them, a pass of
     their own per timing, gather / dense alternating, the order rotating.  With --parent-lib FILE (a libvptr_hip.so built from the parent commit) the dense
     kernel of that build alternates as a third way: the shared body must not have changed its code generation.
  2. kernel time of `clip_draw_kernel` at N = 16 and 256, the same way.
  3. host clock per batch around `--iters` batches that end in a device synchronise, the host-side gather of the uint8 batch counted:
     (a) frames gathered on the host into pinned memory (two buffers), uploaded, `ClipIngest`; (b) `StoreLoader.draw()`.
  4. one K64 epoch (bench.py's model, per-GPU batch 16, one captured hipGraph per step) fed by (a) and by (b): steps / s over the epoch,
     and per step the time in the stream between the end of the previous replay and the moment the next batch is in the graph's static
     inputs (two device events).

    python tools/clip_store_bench.py [--iters 50] [--repeats 5] [--epoch-steps 60] [--parent-lib FILE] [--skip-epoch] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from vptr_amd import _lib, ops                                                  # noqa: E402
from vptr_amd.data import ClipIngest, DeviceClipStore, IngestPlan, StoreLoader  # noqa: E402

# name, plan constructor, (N, Tp, Tf), clips in the store: the batches of profiles/ingest.md
BATCHES = [("kth64", lambda d: IngestPlan.kth(64, device=d), (16, 10, 10), 960),
           ("kth128", lambda d: IngestPlan.kth(128, device=d), (16, 10, 40), 384),
           ("bair", lambda d: IngestPlan.bair(device=d), (16, 2, 28), 960)]


def wall(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def kernel_durations(fn, iters, name):
    """device durations (us) of the launches of kernel `name` in `iters` calls, from the profiler; [] if it records none"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    return sorted(float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.events()
                  if name in e.name and str(getattr(e, "device_type", "")).endswith("CUDA"))


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def dense_call(lib, raw, flips, plan, Tp, Tf, outs):
    """vptr_clip_ingest of library `lib` (this build's or the parent's) on a dense batch"""
    top, left, Hc, Wc = plan.crop
    Hout, Wout = plan.out_hw
    hp, vp = Wout != Wc, Hout != Hc
    p = _lib.ptr
    rc = lib.vptr_clip_ingest(p(raw), p(plan.kx) if hp else None, p(plan.bx) if hp else None, p(plan.ky) if vp else None, p(plan.by) if vp else None,
                              p(plan.lut), p(flips), p(outs[0]), p(outs[1]), int(raw.shape[0]), Tp + Tf, Tp, plan.in_hw[0], plan.in_hw[1],
                              plan.channels, top, left, Hc, Wc, Hout, Wout, plan.ksx if hp else 0, plan.ksy if vp else 0, _lib.stream())
    if rc != 0:
        raise RuntimeError("vptr_clip_ingest failed (%d)" % rc)


def load_parent(path):
    lib = ctypes.CDLL(path)
    lib.vptr_clip_ingest.argtypes = _lib.SIGNATURES["vptr_clip_ingest"]
    lib.vptr_clip_ingest.restype = ctypes.c_int
    return lib


def make_store(plan, Tp, Tf, n_clips, dev, seed=1):
    """random uint8 frames, n_clips clips of Tp + Tf frames each in one long video -> (DeviceClipStore, the frames on the host)"""
    (H, W), C = plan.in_hw, plan.channels
    frames = np.random.default_rng(seed).integers(0, 256, size=(n_clips * (Tp + Tf), H, W, C), dtype=np.uint8)
    return DeviceClipStore.from_videos([frames], Tp, Tf, device=dev), frames


class HostBatches:
    """way (a): the sampler's permutation on the host, the uint8 batch gathered from host memory into one of two pinned buffers, one
    upload, `ClipIngest`.  No worker processes: the gather runs in the training process while the device works on the previous step."""

    def __init__(self, frames, clips, plan, N, Tp, Tf, out=None, seed=0):
        self.frames, self.clips, self.N, self.T, self.Tp = frames, clips, N, Tp + Tf, Tp
        self.ingest = ClipIngest(plan, Tp, Tf)
        self.out = out
        self.rng = np.random.RandomState(seed)
        self.pinned = [torch.empty((N, Tp + Tf) + tuple(frames.shape[1:]), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.views = [p.numpy() for p in self.pinned]
        self.uploaded = [None, None]
        self.order, self.at, self.k = self.rng.permutation(len(clips)), 0, 0

    def draw(self):
        if self.at + self.N > len(self.order):
            self.order, self.at = self.rng.permutation(len(self.clips)), 0
        ids = self.order[self.at:self.at + self.N]
        self.at += self.N
        t = np.arange(self.T)
        idx = np.where(t[None, :] < self.Tp, self.clips[ids, 0, None] + t[None, :], self.clips[ids, 1, None] + (t[None, :] - self.Tp))
        b = self.k & 1
        self.k += 1
        if self.uploaded[b] is not None:
            self.uploaded[b].synchronize()                       # the previous upload from this buffer has left it
        np.take(self.frames, idx, axis=0, out=self.views[b], mode="clip")
        res = self.ingest(self.pinned[b], out=self.out)
        ev = torch.cuda.Event()
        ev.record()
        self.uploaded[b] = ev
        return res


def epoch(trainer, source, steps):
    """`steps` captured steps fed by `source.draw()` -> (steps / s, per-step feed time in the stream in us)"""
    ready = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    done = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        past, future = source.draw()
        ready[i].record()
        trainer.step(past, future)
        done[i].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return steps / dt, [done[i - 1].elapsed_time(ready[i]) * 1e3 for i in range(1, steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epoch-steps", type=int, default=60)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_store_bench: needs the GPU (no fallback)")
    dev = torch.device("cuda:0")
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    res = {"kernels": [], "draw": [], "host": [], "epoch": None}

    for name, make, (N, Tp, Tf), n_clips in BATCHES:
        plan = make(dev)
        store, frames = make_store(plan, Tp, Tf, n_clips, dev)
        loader = StoreLoader(store, plan, N, Tp, Tf, hflip_p=0.5, vflip_p=0.5, seed=11)
        outs = loader.draw()
        sel = loader.last_selection()
        t = torch.arange(Tp + Tf, device=dev)
        idx = torch.where(t[None, :] < Tp, sel[:, 0, None] + t[None, :], sel[:, 1, None] + (t[None, :] - Tp)).long()
        raw = store.frames[idx].contiguous()                     # the same frames laid out densely
        flips = sel[:, 2].contiguous()
        d_outs = (torch.empty_like(outs[0]), torch.empty_like(outs[1]))

        def gather():
            ops.ingest_gather(store.frames, sel, plan, (Tp, Tf), out=outs)

        def dense():
            dense_call(_lib.lib, raw, flips, plan, Tp, Tf, d_outs)

        def dense_parent():
            dense_call(parent, raw, flips, plan, Tp, Tf, d_outs)       # the same buffers as this build's

        ways = [("gather", gather, "clip_ingest_gather_kernel"), ("dense", dense, "clip_ingest_kernel")]
        if parent is not None:
            ways.append(("dense_parent", dense_parent, "clip_ingest_kernel"))
        for _, fn, _ in reversed(ways):                          # warm-up; the last writer of d_outs is this build's dense kernel
            wall(fn, 5)
            if fn is dense_parent:
                kept = (d_outs[0].clone(), d_outs[1].clone())
        torch.cuda.synchronize()
        assert torch.equal(outs[0], d_outs[0]) and torch.equal(outs[1], d_outs[1])
        if parent is not None:
            assert torch.equal(kept[0], d_outs[0]) and torch.equal(kept[1], d_outs[1])
        meds = {w: [] for w, _, _ in ways}
        spans = {w: [] for w, _, _ in ways}
        for rep in range(args.repeats):                          # alternating, the order rotating from pass to pass
            for w, fn, kname in ways[rep % len(ways):] + ways[:rep % len(ways)]:
                kd = kernel_durations(fn, args.iters, kname)
                meds[w].append(med(kd))
                spans[w].append([kd[0], kd[-1], len(kd)] if kd else None)
        row = {"batch": name, "N": N, "T": Tp + Tf, "store_frames": store.n_frames, "store_bytes": store.nbytes(), "median_kernel_us": meds,
               "min_max_n": spans}
        res["kernels"].append(row)
        print(json.dumps(row), flush=True)

        # 3. host clock per batch, the host-side gather counted
        host = HostBatches(frames, store.clips_host, plan, N, Tp, Tf)
        wall(host.draw, 5), wall(loader.draw, 5)
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(wall(host.draw, args.iters))
            tb.append(wall(loader.draw, args.iters))
        row = {"batch": name, "host_gather_pinned_upload_ingest_us": ta, "store_loader_us": tb}
        res["host"].append(row)
        print(json.dumps(row), flush=True)
        del store, loader, host, frames, raw
        torch.cuda.empty_cache()

    # 2. the draw alone
    table = torch.stack([torch.arange(20000, dtype=torch.int32) * 20, torch.arange(20000, dtype=torch.int32) * 20 + 10], dim=1).to(dev)
    cursor = torch.zeros(16, dtype=torch.int32, device=dev)
    for N in (16, 256):
        sel = torch.zeros((N, 4), dtype=torch.int32, device=dev)

        def draw():
            ops.clip_draw(cursor, table, sel, hflip_p=0.5, vflip_p=0.5)

        wall(draw, 5)
        kd = [kernel_durations(draw, args.iters, "clip_draw_kernel") for _ in range(args.repeats)]
        row = {"N": N, "n_clips": 20000, "median_kernel_us": [med(k) for k in kd], "min_max_n": [[k[0], k[-1], len(k)] if k else None for k in kd]}
        res["draw"].append(row)
        print(json.dumps(row), flush=True)

    # 4. one K64 epoch of captured steps
    if not args.skip_epoch:
        import bench
        from vptr_amd.train import NARTrainer
        N, Tp, Tf = 16, bench.TP, bench.TF
        enc, dec, T, _, tkw, past, fut, _ = bench.build_job("k64", dev, 0.1, N, 0)
        trainer = NARTrainer(enc, dec, T, lr=1e-4, max_grad_norm=1.0, **tkw)
        trainer.capture(past, fut, warmup=2)
        static = trainer.static_inputs()
        plan = IngestPlan.kth(64, device=dev)
        store, frames = make_store(plan, Tp, Tf, N * args.epoch_steps, dev)
        loader = StoreLoader(store, plan, N, Tp, Tf, hflip_p=0.5, vflip_p=0.5, seed=11, out=static)
        host = HostBatches(frames, store.clips_host, plan, N, Tp, Tf, out=static)
        assert len(loader) == args.epoch_steps
        epoch(trainer, host, 5), epoch(trainer, loader, 5)
        loader.seek(0, 0)
        rows = {"host": [], "store": []}
        for _ in range(args.repeats):                            # alternating
            for tag, src in (("host", host), ("store", loader)):
                rate, gaps = epoch(trainer, src, args.epoch_steps)
                gaps = sorted(gaps)
                rows[tag].append({"steps_per_s": rate, "feed_us_min": gaps[0], "feed_us_median": med(gaps), "feed_us_max": gaps[-1]})
        res["epoch"] = {"steps": args.epoch_steps, "batch": N, "graph_nodes": getattr(trainer, "graph_nodes", None), "ways": rows}
        print(json.dumps(res["epoch"]), flush=True)

    # ---- tables ---------------------------------------------------------------------------------------------------------------------
    f1 = lambda v: " ".join("n/a" if e is None else "%.1f" % e for e in v)      # noqa: E731
    print("\n| batch | store | gather kernel us (medians of %d launches) | dense kernel us | dense kernel us, parent build | gather / dense, medians |"
          % args.iters)
    print("|---|---|---|---|---|---|")
    for r in res["kernels"]:
        m = r["median_kernel_us"]
        g, d = med([e for e in m["gather"] if e is not None]), med([e for e in m["dense"] if e is not None])
        print("| %s | %d frames, %.0f MB | %s | %s | %s | %s |" % (r["batch"], r["store_frames"], r["store_bytes"] / 1e6, f1(m["gather"]), f1(m["dense"]),
                                                                  f1(m["dense_parent"]) if "dense_parent" in m else "not measured",
                                                                  "%.3f" % (g / d) if g and d else "not measured"))
    print("\n| draw | kernel us (medians of %d launches) | min / max / n of each pass |" % args.iters)
    print("|---|---|---|")
    for r in res["draw"]:
        print("| N = %d, %d clips | %s | %s |" % (r["N"], r["n_clips"], f1(r["median_kernel_us"]),
                                                 "; ".join("n/a" if s is None else "%.1f / %.1f / %d" % tuple(s) for s in r["min_max_n"])))
    print("\n| batch | (a) host gather + pinned upload + ClipIngest, us per batch | (b) StoreLoader, us per batch | (a) / (b), medians |")
    print("|---|---|---|---|")
    for r in res["host"]:
        a, b = r["host_gather_pinned_upload_ingest_us"], r["store_loader_us"]
        print("| %s | %s | %s | %.1fx |" % (r["batch"], " ".join("%.0f" % v for v in a), " ".join("%.0f" % v for v in b), med(a) / med(b)))
    if res["epoch"]:
        print("\n| K64 epoch of %d captured steps, fed by | steps / s | feed time in the stream, us: min / median / max per run |" % res["epoch"]["steps"])
        print("|---|---|---|")
        for tag, label in (("host", "(a) host batches"), ("store", "(b) StoreLoader")):
            rows = res["epoch"]["ways"][tag]
            print("| %s | %s | %s |" % (label, " ".join("%.3f" % r["steps_per_s"] for r in rows),
                                       "; ".join("%.0f / %.0f / %.0f" % (r["feed_us_min"], r["feed_us_median"], r["feed_us_max"]) for r in rows)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
