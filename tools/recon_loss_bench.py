"""Measurements of the reconstruction-loss kernels (csrc/recon_loss.hip) -> profiles/recon_loss.md.

    python tools/recon_loss_bench.py [--reps 30] [--inner 20] [--skip-step] [--out profiles/recon_loss.md]

One process, one session; the variants of each comparison ALTERNATE inside every repetition.  A kernel measurement is `inner` back-to-back
calls between two HIP events on the launch stream, divided by `inner` (one call is a few microseconds, below what a pair of events
resolves); the tables give median, min and max over the repetitions and their spread (max - min), which is what "no slower than" is
judged against:

  1. vptr_recon_loss_fwd in four settings (defaults; both weight vectors; alpha 2; alpha 1.5) beside the untouched vptr_mse_gdl_fwd, at
     the K64 loss shape (160 planes of 64 x 64) and the KTH128 one (80 planes of 128 x 128: batch 2 x 40 frames);
  2. the same for vptr_recon_loss_bwd beside vptr_mse_gdl_bwd;
  3. the captured K64 step with recon=ReconLoss("l1", 2.0, "exp") against the default captured step.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"K64 (16 x 10 x 1 x 64 x 64: 160 planes)": (16, 10, 1, 64, 64), "KTH128 (2 x 40 x 1 x 128 x 128: 80 planes)": (2, 40, 1, 128, 128)}


def alternate(variants, reps, inner=1, warmup=3):
    """variants: [(name, fn)] -> {name: [ms per call, one entry per repetition]}; every repetition runs each variant, in order"""
    out = {name: [] for name, _ in variants}
    for r in range(warmup + reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                out[name].append(e0.elapsed_time(e1) / inner)
    return out


def row(name, ms, scale=1e3):
    med, lo, hi = statistics.median(ms) * scale, min(ms) * scale, max(ms) * scale
    return "| %s | %.2f | %.2f | %.2f | %.2f |" % (name, med, lo, hi, hi - lo)


def verdict(res, old, new):
    a, b = statistics.median(res[old]), statistics.median(res[new])
    spread = max(res[old]) - min(res[old])
    word = "no slower than" if b - a <= spread else "SLOWER than"
    return "Defaults against `%s`: median %+.2f us (%+.1f %%), the existing kernel's own spread is %.2f us: the default variant is %s the existing kernel by that measure." % (
        old, (b - a) * 1e3, 100.0 * (b - a) / a, spread * 1e3, word)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_loss.md"))
    args = ap.parse_args()
    from vptr_amd import ops
    from vptr_amd._lib import check, lib, ptr, stream
    from vptr_amd.model.criterion import temporal_weight_func
    dev = torch.device("cuda:0")
    lines = ["# Reconstruction losses with temporal weights, L1 and a GDL exponent: measurements", "",
             "`python tools/recon_loss_bench.py --reps %d --inner %d` on one MI355X, one process; variants alternate inside every repetition; a kernel "
             "time is %d back-to-back calls between two HIP events divided by %d, in microseconds; spread = max - min over the repetitions." % (
                 args.reps, args.inner, args.inner, args.inner), ""]

    for title, shape in SHAPES.items():
        N, T, C, H, W = shape
        planes = N * T * C
        torch.manual_seed(11)
        gt = torch.randn(shape, device=dev) * 0.3
        pred = gt + torch.randn(shape, device=dev) * 0.1
        wp, wg = temporal_weight_func(T).float().to(dev), torch.linspace(0.5, 1.5, T, device=dev)
        s_old, s_new = torch.empty(planes * ((H + 15) // 16) * 3, device=dev), torch.empty(planes * ((H + 15) // 16) * 4, device=dev)
        mse, gdl, out3, dpred = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.empty(3, device=dev), torch.empty_like(pred)
        g = [torch.full((1,), v, device=dev) for v in (0.7, 1.3, 1.9)]

        def old_fwd():
            check(lib.vptr_mse_gdl_fwd(ptr(pred), ptr(gt), ptr(s_old), ptr(mse), ptr(gdl), planes, H, W, stream()), "vptr_mse_gdl_fwd")

        def old_bwd():
            check(lib.vptr_mse_gdl_bwd(ptr(pred), ptr(gt), ptr(g[0]), ptr(g[2]), ptr(dpred), planes, H, W, stream()), "vptr_mse_gdl_bwd")

        def new_fwd(w, alpha):
            a, b = (wp, wg) if w else (None, None)
            return lambda: check(lib.vptr_recon_loss_fwd(ptr(pred), ptr(gt), ptr(a), ptr(b), ptr(s_new), ptr(out3), planes, C, T, H, W, alpha, stream()),
                                 "vptr_recon_loss_fwd")

        def new_bwd(w, alpha, l1):
            a, b = (wp, wg) if w else (None, None)
            return lambda: check(lib.vptr_recon_loss_bwd(ptr(pred), ptr(gt), ptr(a), ptr(b), ptr(g[0]), ptr(g[1] if l1 else None), ptr(g[2]), ptr(dpred),
                                                         planes, C, T, H, W, alpha, stream()), "vptr_recon_loss_bwd")

        fwd = [("vptr_mse_gdl_fwd", old_fwd), ("vptr_recon_loss_fwd, defaults", new_fwd(False, 1.0)), ("vptr_recon_loss_fwd, weights", new_fwd(True, 1.0)),
               ("vptr_recon_loss_fwd, alpha 2", new_fwd(False, 2.0)), ("vptr_recon_loss_fwd, alpha 1.5", new_fwd(False, 1.5))]
        bwd = [("vptr_mse_gdl_bwd", old_bwd), ("vptr_recon_loss_bwd, defaults", new_bwd(False, 1.0, False)),
               ("vptr_recon_loss_bwd, weights + L1", new_bwd(True, 1.0, True)), ("vptr_recon_loss_bwd, alpha 2", new_bwd(False, 2.0, False)),
               ("vptr_recon_loss_bwd, alpha 1.5", new_bwd(False, 1.5, False))]
        for what, variants in (("forward (two launches per call)", fwd), ("backward (one launch per call)", bwd)):
            res = alternate(variants, args.reps, args.inner)
            lines += ["## %s, %s" % (title, what), "", "| call | median us | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v) for k, v in res.items()]
            lines += ["", verdict(res, variants[0][0], variants[1][0]), ""]
        del gt, pred, dpred

    if not args.skip_step:
        import bench
        from vptr_amd.train import NARTrainer, ReconLoss

        def trainer(**kw):
            ops.manual_seed(dev, 5)
            enc, dec, T = bench.build_models(dev, 0.1)
            tr = NARTrainer(enc, dec, T, batch_size=16, lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, **kw)
            past, fut = bench.synth_batch(16, 0, dev)
            tr.capture(past, fut, warmup=3)
            return tr, tr.static_inputs()

        base, (bp, bf) = trainer()
        rec, (rp, rf) = trainer(recon=ReconLoss("l1", 2.0, "exp"))
        res = alternate([("default trainer, replay", lambda: base.step(bp, bf)), ("recon=ReconLoss(\"l1\", 2.0, \"exp\"), replay", lambda: rec.step(rp, rf))],
                        max(args.reps // 2, 5))
        torch.cuda.synchronize()
        lines += ["## Captured K64 step (batch 16)", "", "| replay | median ms | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v, 1.0) for k, v in res.items()]
        lines += ["", "Node census: default %r, with the ReconLoss %r." % (base.graph_nodes, rec.graph_nodes), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
