"""Measurements of gradient accumulation and EMA weights (csrc/optim.hip) -> profiles/accum_ema.md.

    python tools/accum_bench.py [--reps 20] [--out profiles/accum_ema.md]

One process, one session; the variants of each comparison ALTERNATE inside every repetition, each call between two HIP events on the
launch stream, and the table gives median, min and max of the repetitions (the run-to-run spread the conditions are judged against):

  1. vptr_accum_begin at the K64 slab size, zeroing, against grad.zero_() on the same buffer, and a hold call (MICRO != 0: no work);
  2. vptr_adamw_ctl_ema (9 slab streams) against vptr_adamw_ctl (7) on the same buffers: achieved bytes/s;
  3. the captured K64 step: a default trainer's replay against the hold replay and the closing replay of accum_steps=2 + ema_decay.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(variants, reps, warmup=3):
    """variants: [(name, fn)] -> {name: [ms per repetition]}; every repetition runs each variant once, in order"""
    out = {name: [] for name, _ in variants}
    for r in range(warmup + reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def row(name, ms, nbytes=None):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    bw = "" if nbytes is None else " %.2f |" % (nbytes / (med * 1e-3) / 1e12)
    return "| %s | %.4f | %.4f | %.4f | %.4f |%s" % (name, med, lo, hi, hi - lo, bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_ema.md"))
    args = ap.parse_args()
    import bench
    from vptr_amd import ops
    from vptr_amd._lib import check, lib, ptr, stream
    from vptr_amd.optim import W_MICRO
    from vptr_amd.train import NARTrainer
    dev = torch.device("cuda:0")
    lines = ["# Gradient accumulation and EMA weights: measurements", "",
             "`python tools/accum_bench.py --reps %d` on one MI355X, one process; variants alternate inside every repetition; times in ms "
             "between HIP events on the launch stream; spread = max - min over the repetitions." % args.reps, ""]

    # ---- 3 first (it builds the K64 model and tells the slab size) ---------------------------------------------------------------
    def trainer(**ctl):
        ops.manual_seed(dev, 5)
        enc, dec, T = bench.build_models(dev, 0.1)
        tr = NARTrainer(enc, dec, T, batch_size=16, lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **ctl)
        past, fut = bench.synth_batch(16, 0, dev)
        tr.capture(past, fut, warmup=3)
        return tr, tr.static_inputs()

    base, (bp, bf) = trainer()
    acc, (apast, afut) = trainer(accum_steps=2, ema_decay=0.999)
    acc.opt.reset_window()
    n = acc.opt.flat.numel()
    res = alternate([("default trainer, replay", lambda: base.step(bp, bf)), ("accum_steps=2 + EMA, hold replay", lambda: acc.step(apast, afut)),
                     ("accum_steps=2 + EMA, closing replay", lambda: acc.step(apast, afut))], args.reps)
    torch.cuda.synchronize()
    assert acc.opt.ctl.micro_host == 0 and float(acc.opt.micro()) == 0.0
    lines += ["## 3. Captured K64 step (batch 16, slab %d floats = %.1f MB)" % (n, n * 4 / 1e6), "",
              "| replay | median | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v) for k, v in res.items()]
    lines += ["", "The hold replay still runs `vptr_sumsq` and the plane refresh (reported, not removed); its update kernel and the zero-fill return "
              "at once.  Node census: default %r, accumulating %r." % (base.graph_nodes, acc.graph_nodes), ""]
    del base, acc
    ops.unregister_flat_slabs()
    torch.cuda.empty_cache()

    # ---- 1 -----------------------------------------------------------------------------------------------------------------------
    g = torch.randn(n, device=dev)
    w_zero, w_hold = torch.zeros(16, device=dev), torch.zeros(16, device=dev)
    w_hold[W_MICRO] = 1.0
    begin = lambda w: check(lib.vptr_accum_begin(ptr(g), n, ptr(w), stream()), "vptr_accum_begin")
    res = alternate([("grad.zero_()", g.zero_), ("vptr_accum_begin, MICRO = 0 (zeroing)", lambda: begin(w_zero)),
                     ("vptr_accum_begin, MICRO = 1 (hold)", lambda: begin(w_hold))], args.reps)
    assert float(g.abs().sum()) == 0.0
    lines += ["## 1. vptr_accum_begin against grad.zero_() (%d floats)" % n, "", "| call | median | min | max | spread | TB/s written |", "|---|---|---|---|---|---|",
              row("grad.zero_()", res["grad.zero_()"], 4 * n), row("vptr_accum_begin, MICRO = 0 (zeroing)", res["vptr_accum_begin, MICRO = 0 (zeroing)"], 4 * n),
              row("vptr_accum_begin, MICRO = 1 (hold)", res["vptr_accum_begin, MICRO = 1 (hold)"]) + " - |", ""]

    # ---- 2 -----------------------------------------------------------------------------------------------------------------------
    from vptr_amd.optim import OptimControls
    ctl = OptimControls(dev, 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0, accum_steps=1, ema_decay=0.999)
    p, m, v, e = (torch.randn(n, device=dev) * s for s in (0.1, 0.0, 0.0, 0.1))
    v.abs_()
    g = torch.randn(n, device=dev) * 1e-3
    step_dev, sumsq = torch.zeros(1, device=dev), (g.double() ** 2).sum().float().reshape(1)
    ctl.prepare(step_dev, sumsq)
    res = alternate([("vptr_adamw_ctl (7 streams)", lambda: ctl.update(p, g, m, v, n)), ("vptr_adamw_ctl_ema (9 streams)", lambda: ctl.update(p, g, m, v, n, ema=e))], args.reps)
    a, b = statistics.median(res["vptr_adamw_ctl (7 streams)"]), statistics.median(res["vptr_adamw_ctl_ema (9 streams)"])
    lines += ["## 2. vptr_adamw_ctl_ema against vptr_adamw_ctl (%d floats)" % n, "", "| kernel | median | min | max | spread | TB/s moved |", "|---|---|---|---|---|---|",
              row("vptr_adamw_ctl (7 streams)", res["vptr_adamw_ctl (7 streams)"], 7 * 4 * n), row("vptr_adamw_ctl_ema (9 streams)", res["vptr_adamw_ctl_ema (9 streams)"], 9 * 4 * n), "",
              "Time ratio %.3f; 9 / 7 = %.3f is the floor at equal bytes/s." % (b / a, 9 / 7), ""]
    lines += ["## Not measured", "", "`python bench.py` alternated between this commit's library and one built from the parent commit.  The benchmark constructs its "
              "trainer without the new arguments, and the node census of such a trainer is pinned unchanged by "
              "`tests/test_18_accum_ema_gpu.py::test_default_trainer_graph_census_is_unchanged`; multi-GPU exchange time under accumulation.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
