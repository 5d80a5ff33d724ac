"""Measurements of the parameter groups of the optimizer controls (csrc/optim.hip) -> the timing section of profiles/param_groups.md.

    python tools/param_groups_bench.py [--reps 20] [--out FILE] [--skip-step]

One process, one session; the variants of each comparison ALTERNATE inside every repetition, each call between two HIP events on the
launch stream, and the tables give median, min and max of the repetitions (the run-to-run spread the conditions are judged against):

  1. vptr_adamw_groups with 1, 2 and 16 groups against vptr_adamw_ctl on the same buffers, at the K64 slab size and at 118 M elements;
  2. its EMA form against vptr_adamw_ctl_ema, likewise;
  3. the captured K64 step: a trainer with plain controls (a constant schedule) against the same trainer with `no_decay_groups`.

The byte map adds one byte per element to 28 (36 with the EMA) moved by the ungrouped kernel: 29/28 (37/36) by the byte count; the
acceptance ratio set for the kernel is the tighter 33/32 (37/36), plus the spread of the ungrouped kernel in the same session.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.accum_bench import alternate, row   # noqa: E402

BIG = 118_000_000


def kernels(n, dev, reps, lines):
    from vptr_amd.optim import GroupTable, OptimControls
    ctl = OptimControls(dev, 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0, accum_steps=1, ema_decay=0.999)
    p, m, v, e = (torch.randn(n, device=dev) * s for s in (0.1, 0.0, 0.0, 0.1))
    v.abs_()
    g = torch.randn(n, device=dev) * 1e-3
    step_dev, sumsq = torch.zeros(1, device=dev), (g.double() ** 2).sum().float().reshape(1)
    ctl.prepare(step_dev, sumsq)
    tabs = {}
    for ng in (1, 2, 16):
        # contiguous runs of unequal length, as parameters lie in a slab; boundaries fall inside float4s
        gid = torch.zeros(n, dtype=torch.uint8, device=dev)
        for j in range(1, ng):
            gid[(j * n) // ng + (j % 3):] = j
        tabs[ng] = GroupTable(dev, gid, [(1.0 if j % 2 == 0 else 0.5, None if j % 3 else 0.0) for j in range(ng)], 1e-2)
        tabs[ng].scalars(ctl.state)
    for ema, ref_name, streams in ((None, "vptr_adamw_ctl", 7), (e, "vptr_adamw_ctl_ema", 9)):
        ref = lambda: ctl.update(p, g, m, v, n, ema=ema)
        variants = [(ref_name, ref)] + [("vptr_adamw_groups, %d group%s" % (ng, "" if ng == 1 else "s"),
                                         (lambda t: lambda: ctl.update(p, g, m, v, n, ema=ema, groups=t))(tabs[ng])) for ng in (1, 2, 16)]
        res = alternate(variants, reps)
        base = statistics.median(res[ref_name])
        spread = (max(res[ref_name]) - min(res[ref_name])) / base
        target = (33 / 32) if ema is None else (37 / 36)
        lines += ["### %s form, %d floats (%.1f MB per slab)" % ("EMA" if ema is not None else "plain", n, n * 4 / 1e6), "",
                  "| kernel | median | min | max | spread | TB/s moved | ratio to %s |" % ref_name, "|---|---|---|---|---|---|---|"]
        for name, _ in variants:
            nbytes = streams * 4 * n + (0 if name == ref_name else n)
            lines.append(row(name, res[name], nbytes) + " %.4f |" % (statistics.median(res[name]) / base))
        worst = max(statistics.median(res[name]) / base for name, _ in variants[1:])
        lines += ["", "Byte count %.4f; acceptance %.4f + the spread of %s in this session (%.4f of its median) = %.4f; worst measured ratio %.4f: %s." % (
            (streams * 4 + 1) / (streams * 4), target, ref_name, spread, target + spread, worst, "inside" if worst <= target + spread else "MISSED"), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true", help="kernels only (no K64 model)")
    args = ap.parse_args()
    from vptr_amd import ops
    dev = torch.device("cuda:0")
    lines = ["## Timings", "", "`python tools/param_groups_bench.py --reps %d` on one MI355X, one process; variants alternate inside every repetition; times "
             "in ms between HIP events on the launch stream; spread = max - min over the repetitions." % args.reps, ""]
    n = 26_000_000
    if not args.skip_step:
        import bench
        from vptr_amd.optim import LRSchedule, no_decay_groups
        from vptr_amd.train import NARTrainer

        def trainer(**ctl):
            ops.manual_seed(dev, 5)
            enc, dec, T = bench.build_models(dev, 0.1)
            tr = NARTrainer(enc, dec, T, batch_size=16, lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **ctl)
            past, fut = bench.synth_batch(16, 0, dev)
            tr.capture(past, fut, warmup=3)
            return tr, tr.static_inputs()

        base, (bp, bf) = trainer(schedule=LRSchedule())
        grp, (gp, gf) = trainer(param_groups=no_decay_groups)
        n = grp.opt.flat.numel()
        res = alternate([("plain controls, replay", lambda: base.step(bp, bf)), ("no_decay_groups, replay", lambda: grp.step(gp, gf))], args.reps)
        torch.cuda.synchronize()
        a, b = (statistics.median(res[k]) for k in ("plain controls, replay", "no_decay_groups, replay"))
        sizes = [int((grp.opt.groups.gid == g).sum()) for g in range(grp.opt.groups.ngroups)]
        lines += ["### Captured K64 step (batch 16, slab %d floats = %.1f MB)" % (n, n * 4 / 1e6), "", "| replay | median | min | max | spread |",
                  "|---|---|---|---|---|"] + [row(k, v) for k, v in res.items()]
        lines += ["", "Ratio %.4f.  Group sizes (elements): %r.  Node census: plain controls %r, grouped %r." % (b / a, sizes, base.graph_nodes, grp.graph_nodes), ""]
        del base, grp
        ops.unregister_flat_slabs()
        torch.cuda.empty_cache()
    for size in (n, BIG):
        kernels(size, dev, args.reps, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
