"""Measurements of the per-tensor statistics (csrc/tensor_stats.hip, vptr_amd/diagnostics.py) -> profiles/tensor_stats.md.

    python tools/tensor_stats_bench.py [--reps 20] [--out profiles/tensor_stats.md] [--skip-step]

One process, one session; the variants of each comparison ALTERNATE inside every repetition, each call between two HIP events on the
launch stream, and the tables give median, min and max of the repetitions (the run-to-run spread the expectations are judged against):

  1. the captured K64 step: a trainer with plain controls (a constant schedule) against the same trainer with `tensor_stats=` at
     every = 1 (every replay due) and at every = 50 (the median replay is not due);
  2. vptr_tensor_stats on the K64 trainer's own plan and on that plan tiled to 118.4 M elements: a due call with moments (four streams),
     without (two), and a call that is not due, beside vptr_sumsq (one stream) and vptr_adamw_ctl (seven) on the same buffers;
  3. the distance of the table from an fp64 reference computed on the device at those sizes, in units of the bars of
     tests/tensor_stats_cases.py.

Nothing here uses more than one GPU.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.accum_bench import alternate, row   # noqa: E402

BIG = 118_400_000
NORM_RTOL, DIR_RTOL = 2.0 ** -23, 2.0 ** -22 + 2.0 ** -26      # tests/tensor_stats_cases.py


def distances(ts, p, g, m, v, state):
    """worst |table - fp64| over all rows in units of the bars; the reference is torch.segment_reduce in fp64 on the device"""
    from vptr_amd import diagnostics as D
    from vptr_amd.optim import S_EPS, S_INV_SQRT_BC2
    lengths = torch.tensor(ts.sizes, device=p.device)
    n = ts.total

    def seg(x):
        per = torch.segment_reduce(x, "sum", lengths=lengths)
        return torch.cat([per, per.sum().reshape(1)])
    tab = ts.table.double()
    numel = torch.cat([lengths.double(), torch.tensor([float(n)], device=p.device, dtype=torch.float64)])
    gn, wn = seg(g[:n].double().pow(2)).sqrt(), seg(p[:n].double().pow(2)).sqrt()
    d = m[:n].double() / (v[:n].double().sqrt() * float(state[S_INV_SQRT_BC2]) + float(state[S_EPS]))
    dr = (seg(d.pow(2)) / numel).sqrt()
    rel = lambda a, b: float(((a - b).abs() / b.clamp_min(1e-300)).max())
    return rel(tab[:, D.GRAD_NORM], gn) / NORM_RTOL, rel(tab[:, D.WEIGHT_NORM], wn) / NORM_RTOL, rel(tab[:, D.DIR_RMS], dr) / DIR_RTOL


def kernels(sizes, dev, reps, lines, label):
    from vptr_amd import diagnostics as D
    from vptr_amd._lib import check, lib, ptr, stream
    from vptr_amd.optim import OptimControls
    n = sum(sizes)
    npad = n + (-n) % 4
    ctl = OptimControls(dev, 1e-4, (0.9, 0.999), 1e-8, 1e-2, 1.0)
    p, m = torch.randn(npad, device=dev) * 0.1, torch.randn(npad, device=dev) * 1e-3
    v = (torch.randn(npad, device=dev) * 1e-3).pow_(2)
    g = torch.randn(npad, device=dev) * 1e-3
    step_dev, sumsq = torch.full((1,), 2.0, device=dev), (g.double() ** 2).sum().float().reshape(1)
    ctl.prepare(step_dev, sumsq)
    scratch = torch.zeros(1, device=dev)
    full = D.TensorStatsState(dev, sizes, None, D.TensorStats(every=1))
    lean = D.TensorStatsState(dev, sizes, None, D.TensorStats(every=1, moments=False))
    idle = D.TensorStatsState(dev, sizes, None, D.TensorStats(every=(1 << 24) - 1))
    variants = [
        ("vptr_sumsq (1 stream)", lambda: check(lib.vptr_sumsq(ptr(g), npad, ptr(scratch), stream()), "vptr_sumsq")),
        ("vptr_adamw_ctl (7 streams)", lambda: ctl.update(p, g, m, v, npad)),
        ("vptr_tensor_stats, due, moments (4 streams)", lambda: full.launch(p, g, m, v, None, ctl.state)),
        ("vptr_tensor_stats, due, no moments (2 streams)", lambda: lean.launch(p, g, m, v, None, ctl.state)),
        ("vptr_tensor_stats, not due", lambda: idle.launch(p, g, m, v, None, ctl.state)),
    ]
    res = alternate(variants, reps)
    nbytes = [4 * npad, 28 * npad, 16 * n + full.items * D.PART_BYTES, 8 * n + full.items * D.PART_BYTES, None]
    lines += ["### %s: %d tensors, %d floats (%.1f MB per slab), %d items" % (label, len(sizes), n, n * 4 / 1e6, full.items), "",
              "| call | median | min | max | spread | TB/s moved |", "|---|---|---|---|---|---|"]
    lines += [row(name, res[name], b) + ("" if b is not None else " - |") for (name, _), b in zip(variants, nbytes)]
    full.launch(p, g, m, v, None, ctl.state)
    torch.cuda.synchronize()
    dg, dw, dd = distances(full, p, g, m, v, ctl.state.cpu())
    lines += ["", "Distance from the fp64 reference over all %d rows, in units of the bars (norms 2^-23, dir_rms 2^-22 + 2^-26): grad_norm %.3f, "
              "weight_norm %.3f, dir_rms %.3f.  Largest tensor: %d elements (%d items, added by one thread of stage 2)."
              % (len(sizes) + 1, dg, dw, dd, max(sizes), -(-max(sizes) // D.CHUNK)), ""]
    return {k: statistics.median(x) for k, x in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_stats.md"))
    ap.add_argument("--skip-step", action="store_true", help="kernels only (a synthetic plan, no K64 model)")
    args = ap.parse_args()
    from vptr_amd import ops
    from vptr_amd.diagnostics import TensorStats
    dev = torch.device("cuda:0")
    lines = ["# Per-tensor statistics: measurements", "",
             "`python tools/tensor_stats_bench.py --reps %d` on one MI355X, one process; variants alternate inside every repetition; times in ms "
             "between HIP events on the launch stream; spread = max - min over the repetitions.  Nothing was measured on more than one GPU." % args.reps, ""]
    sizes = [((i * 7919) % 4000 + 1) * 64 for i in range(200)]
    step = None
    if not args.skip_step:
        import bench
        from vptr_amd.optim import LRSchedule
        from vptr_amd.train import NARTrainer

        def trainer(**ctl):
            ops.manual_seed(dev, 5)
            enc, dec, T = bench.build_models(dev, 0.1)
            tr = NARTrainer(enc, dec, T, batch_size=16, lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **ctl)
            past, fut = bench.synth_batch(16, 0, dev)
            tr.capture(past, fut, warmup=3)
            return tr, tr.static_inputs()

        base, (bp, bf) = trainer(schedule=LRSchedule())
        one, (op, of) = trainer(tensor_stats=TensorStats(every=1))
        fifty, (fp, ff) = trainer(tensor_stats=TensorStats(every=50))
        sizes = list(one.opt.tensor_stats.sizes)
        names = ["plain controls, replay", "tensor_stats every=1, replay", "tensor_stats every=50, replay"]
        res = alternate(list(zip(names, (lambda: base.step(bp, bf), lambda: one.step(op, of), lambda: fifty.step(fp, ff)))), args.reps)
        torch.cuda.synchronize()
        due50 = -(-(args.reps + 3) // 50)   # how many of the every=50 trainer's replays here can be due at most; the median is not
        step = {k: statistics.median(v) for k, v in res.items()}
        spread = max(res[names[0]]) - min(res[names[0]])
        lines += ["## Captured K64 step (batch 16, %d tensors, slab %d floats = %.1f MB)" % (len(sizes), sum(sizes), sum(sizes) * 4 / 1e6), "",
                  "| replay | median | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v) for k, v in res.items()]
        lines += ["", "Node census: plain controls %r, with statistics %r.  Spread of the plain step: %.4f ms.  every=50 against plain: %+.4f ms "
                  "(median; at most %d of its timed replays is due); every=1 against plain: %+.4f ms." % (
                      base.graph_nodes, one.graph_nodes, spread, step[names[2]] - step[names[0]], due50, step[names[1]] - step[names[0]]), ""]
        rep = one.opt.tensor_stats.report(top=3)
        lines += ["The three largest gradient norms of the last replay: " + "; ".join("%s %.3e (update_ratio %.2e)" % (d["name"], d["grad_norm"], d["update_ratio"]) for d in rep) + ".", ""]
        del base, one, fifty
        ops.unregister_flat_slabs()
        torch.cuda.empty_cache()
    lines += ["## The call alone", ""]
    k64 = kernels(sizes, dev, args.reps, lines, "the K64 plan" if not args.skip_step else "a synthetic plan")
    torch.cuda.empty_cache()
    tiled = (sizes * (BIG // sum(sizes) + 1))
    while sum(tiled) > BIG:
        tiled.pop()
    if sum(tiled) < BIG:
        tiled.append(BIG - sum(tiled))
    kernels(tiled, dev, args.reps, lines, "that plan tiled to 118.4 M elements")
    if step is not None:
        due = k64["vptr_tensor_stats, due, moments (4 streams)"]
        lines += ["## Expectations", "",
                  "* a replay that is not due inside the spread of the plain step: %+.4f ms against a spread of %.4f ms: %s." % (
                      step[names[2]] - step[names[0]], spread, "inside" if abs(step[names[2]] - step[names[0]]) <= spread else "MISSED"),
                  "* a due replay costs no more than the stand-alone due call plus that spread: %+.4f ms against %.4f + %.4f ms: %s." % (
                      step[names[1]] - step[names[0]], due, spread, "inside" if step[names[1]] - step[names[0]] <= due + spread else "MISSED"), ""]
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
