"""Measurements of the adversarial-loss kernels (csrc/gan_loss.hip) -> profiles/gan_loss_timings.md.

    python tools/gan_loss_bench.py [--reps 30] [--inner 20] [--seconds 1.0] [--skip-step] [--out profiles/gan_loss_timings.md]

One process, one session; the variants of each comparison ALTERNATE inside every repetition (tools/recon_loss_bench.py's method).  A
kernel measurement is `inner` back-to-back calls between two HIP events on the launch stream, divided by `inner`; the tables give median,
min and max over the repetitions and their spread (max - min), which is what a difference is judged against:

  1. vptr_gan_loss_fwd (two launches) and vptr_gan_loss_bwd (one launch) on a (fake, real) pair in the three modes, beside what the torch
     path issues for the same quantities -- GANLoss twice, (l_fake + l_real) * 0.5 * lam_gan, and autograd's backward of it -- at the K64
     logit count (80 x 6 x 6 = 2880 per tensor) and the KTH128 one (16 x 20 x 14 x 14 = 62 720);
  2. the eager stage-1 step, `AETrainer(gan_loss="torch")` against `gan_loss="fused"` on modules of their own, at batch 4 and 8 x 20 frames of
     64 x 64 with lam_gan = 0.01: device events around at least `seconds` of steps per repetition.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"K64 (80 x 1 x 6 x 6: 2880 logits per tensor)": 2880, "KTH128 (320 x 1 x 14 x 14: 62 720 logits per tensor)": 62720}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_loss_timings.md"))
    args = ap.parse_args()
    import vptr_amd.model as M
    from vptr_amd import ops
    from vptr_amd._lib import check, lib, ptr, stream
    from vptr_amd.model.criterion import GANLoss
    from vptr_amd.train import AETrainer
    dev = torch.device("cuda:0")
    lam = 0.01
    lines = ["# Adversarial-loss kernels: timings", "",
             "`python tools/gan_loss_bench.py --reps %d --inner %d --seconds %g` on one MI355X, one process; variants alternate inside every repetition; "
             "a kernel time is %d back-to-back calls between two HIP events divided by %d, in microseconds; spread = max - min over the repetitions."
             % (args.reps, args.inner, args.seconds, args.inner, args.inner), ""]

    for title, n in SIZES.items():
        torch.manual_seed(11)
        fake, real = torch.randn(n, device=dev) * 3.0, torch.randn(n, device=dev) * 3.0
        scratch, out3 = torch.empty(2 * (-(-n // 2048)), device=dev), torch.empty(3, device=dev)
        dxa, dxb, one = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.ones(1, device=dev)

        def fused_fwd(mode):
            return lambda: check(lib.vptr_gan_loss_fwd(ptr(fake), n, 1, 0, ptr(real), n, 1, 1, mode, 1.0, 0.0, 0.5 * lam, ptr(scratch), ptr(out3), stream()),
                                 "vptr_gan_loss_fwd")

        def fused_bwd(mode):
            return lambda: check(lib.vptr_gan_loss_bwd(ptr(fake), n, 1, 0, ptr(dxa), ptr(real), n, 1, 1, ptr(dxb), mode, 1.0, 0.0, 0.5 * lam, None, None, ptr(one),
                                                       stream()), "vptr_gan_loss_bwd")

        crit = GANLoss("vanilla").to(dev)
        f_leaf, r_leaf = fake.clone().requires_grad_(True), real.clone().requires_grad_(True)

        def torch_fwd():
            return (crit(f_leaf, False) + crit(r_leaf, True)) * 0.5 * lam

        def torch_fwd_bwd():
            f_leaf.grad = r_leaf.grad = None
            torch_fwd().backward()

        fwd = [("torch GANLoss x 2 + glue, forward (vanilla)", torch_fwd)] + [("vptr_gan_loss_fwd, %s" % k, fused_fwd(m)) for k, m in ops.GAN_MODES.items()]
        bwd = [("torch forward + autograd backward (vanilla)", torch_fwd_bwd)] + [("vptr_gan_loss_bwd, %s" % k, fused_bwd(m)) for k, m in ops.GAN_MODES.items()]
        for what, variants in (("forward of the pair", fwd), ("backward of the pair (the torch row includes its forward)", bwd)):
            res = alternate(variants, args.reps, args.inner)
            lines += ["## %s, %s" % (title, what), "", "| call | median us | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v) for k, v in res.items()] + [""]

    if not args.skip_step:
        def frames(nclips, seed):
            rs = np.random.RandomState(seed)
            return torch.from_numpy(rs.uniform(0, 1, size=(nclips, 10, 1, 64, 64)).astype(np.float32)).to(dev)

        def trainer(gan_loss):
            torch.manual_seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                enc, dec = M.VPTREnc(1, 528, 3).to(dev), M.VPTRDec(1, 528, 3, out_layer="Sigmoid").to(dev)
                disc = M.VPTRDisc(1, ndf=64, n_layers=3).to(dev)
                M.init_weights(enc), M.init_weights(dec), M.init_weights(disc)
            return AETrainer(enc, dec, disc, lr=2e-4, lam_gan=lam, gan_loss=gan_loss)

        trainers = {k: trainer(k) for k in ("torch", "fused")}
        for nclips in (4, 8):
            p, f = frames(nclips, 1), frames(nclips, 2)
            for tr in trainers.values():                         # warm-up; also sizes `inner` so that one repetition lasts `seconds`
                for _ in range(3):
                    tr.step(p, f)
            torch.cuda.synchronize()
            probe = alternate([(k, (lambda t=tr: t.step(p, f))) for k, tr in trainers.items()], 1, inner=5, warmup=0)
            inner = max(5, int(args.seconds * 1e3 / max(statistics.median(v) for v in probe.values())) + 1)
            res = alternate([("gan_loss=\"%s\", eager step" % k, (lambda t=tr: t.step(p, f))) for k, tr in trainers.items()], max(args.reps // 6, 5), inner=inner,
                            warmup=1)
            names = list(res)
            d = statistics.median(res[names[1]]) - statistics.median(res[names[0]])
            spread = max(max(v) - min(v) for v in res.values())
            lines += ["## Eager stage-1 step, batch %d x 20 frames of 64 x 64, lam_gan %g (%d steps per repetition)" % (nclips, lam, inner), "",
                      "| variant | median ms | min | max | spread |", "|---|---|---|---|---|"] + [row(k, v, 1.0) for k, v in res.items()]
            lines += ["", "fused - torch: %+.3f ms per step (median); the larger of the two variants' own spreads is %.3f ms." % (d, spread), ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
