"""On-device evaluation: vptr_frame_metrics / vptr_frame_metrics_accumulate through the C ABI and through ops.frame_metrics against the
fp64 builder of frame_metrics_ref.py (pinned to the reference's golden values by test_frame_metrics_cpu.py), FrameMetrics and
evaluate_rollout against vptr_amd.metrics on the same rollout outputs, and the guards.

Bars: the project's own for these metrics (test_02_model_gpu.py::test_metrics_on_device): |dSSIM| < 1e-5, |dPSNR| < 1e-4 dB, summed
squared error within 1e-5 relative.  The float32 torch formulation of exactly these shapes and image kinds sits at most 3.4e-7 (SSIM) and
2.1e-6 dB (PSNR) from fp64 on a CPU, so the bars leave >= 29x / >= 47x for a correct float32 kernel and still catch a wrong tap, halo or
normaliser.  The kernel's own worst distances are recorded in profiles/frame_metrics.md (4.9e-7 SSIM, 1.2e-6 dB, 1.6e-7 relative).
Every output and scratch buffer is NaN before each call."""
import numpy as np
import pytest
import torch

from frame_metrics_ref import BAR_MSE_REL, BAR_PSNR, BAR_SSIM, KINDS, KTH, assert_close, make_pair, norm_consts, ref_frame_metrics
from helpers import build_transformer, jload, load
from oracle import fill

pytestmark = pytest.mark.gpu

NAN = float("nan")


def abi_frame_metrics(pred, gt, mean, std, clamp=0, data_range=1.0, out=None):
    """one direct C-ABI call on contiguous device tensors (N, T, C, H, W); scratch and out start as NaN"""
    from vptr_amd._lib import check, lib, ptr, stream
    N, T, C, H, W = pred.shape
    dev = pred.device
    mean_d = torch.as_tensor(mean, dtype=torch.float32).reshape(-1).expand(C).contiguous().to(dev)
    std_d = torch.as_tensor(std, dtype=torch.float32).reshape(-1).expand(C).contiguous().to(dev)
    scratch = torch.full((N * T * C * ((H + 15) // 16) * 2,), NAN, device=dev)
    if out is None:
        out = torch.full((N, T, 3), NAN, device=dev)
    check(lib.vptr_frame_metrics(ptr(pred), ptr(gt), ptr(mean_d), ptr(std_d), ptr(scratch), ptr(out), N * T, C, H, W, clamp, data_range,
                                 stream()), "vptr_frame_metrics")
    return out


# ------------------------------------------------------------------------------------------------------ 1. the reference's values
@pytest.mark.parametrize("tag,T", [("a", 1), ("b", 1), ("b", 2)])
def test_reference_fixture(dev, tag, T):
    """metrics_tiny: "a" (3, 1, 32, 32) as N = 3, "b" (2, 3, 20, 28) as N = 2 and as N = 1, T = 2; mean 0, std 1"""
    import vptr_amd.ops as ops
    z = load("metrics_tiny")
    e = jload(z, "expected")[tag]
    x, y = torch.from_numpy(z["x:" + tag]), torch.from_numpy(z["y:" + tag])
    shape = (x.shape[0] // T, T) + tuple(x.shape[1:])
    xd, yd = x.reshape(shape).to(dev), y.reshape(shape).to(dev)
    for name, got, got255 in (("abi", abi_frame_metrics(xd, yd, 0.0, 1.0), abi_frame_metrics(xd * 255, yd * 255, 0.0, 1.0, 0, 255.0)),
                              ("op", ops.frame_metrics(xd, yd), ops.frame_metrics(xd * 255, yd * 255, data_range=255.0))):
        g, g255 = got.cpu().double().reshape(-1, 3), got255.cpu().double().reshape(-1, 3)
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(g255).all())
        ds = float((g[:, 2] - torch.tensor(e["ssim_each"], dtype=torch.float64)).abs().max())
        dp, dp255 = abs(float(g[:, 0].mean()) - e["psnr"]), abs(float(g255[:, 0].mean()) - e["psnr255"])
        dm = abs(float(g[:, 1].mean()) - e["mse"]) / abs(e["mse"])
        print("fixture %s T %d %s: ssim_each %.3e psnr %.3e psnr255 %.3e mse rel %.3e" % (tag, T, name, ds, dp, dp255, dm))
        assert ds < BAR_SSIM and dp < BAR_PSNR and dp255 < BAR_PSNR and dm < BAR_MSE_REL


# ------------------------------------------------------------------------------------------------------ 2. fp64 parity
SHAPES = [(2, 3, 1, 7, 7),       # smaller than the window: the zero padding carries the whole sum
          (1, 2, 1, 11, 13),
          (2, 2, 3, 20, 28),
          (1, 3, 3, 37, 50),     # odd sizes, a band tail
          (2, 2, 1, 64, 64),
          (1, 1, 1, 128, 128),
          (1, 1, 3, 5, 256),     # the width limit
          (1, 2, 1, 130, 9)]     # many bands, narrow


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp64_parity(dev, shape, kind):
    """through the C ABI and through the op; without the clamp, and with it on images stretched to [-0.1, 1.1]"""
    import vptr_amd.ops as ops
    seed = 900 + 10 * SHAPES.index(shape)
    for clamp in (False, True):
        pred, gt, mean, std = make_pair(shape, kind, seed, stretch=clamp)
        ref = ref_frame_metrics(pred, gt, mean, std, clamp=clamp)
        pd, gd = pred.to(dev), gt.to(dev)
        assert_close(abi_frame_metrics(pd, gd, mean, std, int(clamp)), ref, "abi %s %s clamp %d" % (shape, kind, clamp))
        got = ops.frame_metrics(pd, gd, mean, std, clamp=clamp)
        assert got.shape == shape[:2] + (3,) and got.dtype == torch.float32
        assert_close(got, ref, "op  %s %s clamp %d" % (shape, kind, clamp))


def test_four_dim_input_is_one_time_step(dev):
    import vptr_amd.ops as ops
    pred, gt, mean, std = make_pair((3, 1, 3, 20, 28), "smooth", 980)
    got = ops.frame_metrics(pred[:, 0].to(dev), gt[:, 0].to(dev), torch.tensor(mean), list(std))
    assert got.shape == (3, 1, 3)
    assert_close(got, ref_frame_metrics(pred, gt, mean, std), "4-d input")


@pytest.mark.parametrize("shape", [(2, 2, 1, 7, 7), (1, 2, 3, 37, 50), (1, 1, 1, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_identical_inputs(dev, shape):
    pred, _, mean, std = make_pair(shape, "saturated", 990)
    pd = pred.to(dev)
    got = abi_frame_metrics(pd, pd.clone(), mean, std).cpu().double().reshape(-1, 3)
    print("pred == gt %s: psnr %s sse %s 1 - ssim %s" % (shape, got[:, 0].tolist(), got[:, 1].tolist(), (1 - got[:, 2]).tolist()))
    assert bool((got[:, 1] == 0).all())
    assert float((got[:, 0] - 80.0).abs().max()) <= 1e-4
    assert float((got[:, 2] - 1.0).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------ 3. determinism, containment
def test_deterministic_and_contained(dev):
    shape = (2, 2, 3, 37, 50)
    pred, gt, mean, std = make_pair(shape, "noise", 1000)
    pd, gd = pred.to(dev), gt.to(dev)
    n, pad = shape[0] * shape[1] * 3, 64
    guard = torch.arange(n + 2 * pad, device=dev, dtype=torch.float32) * 0.37 + 1.0
    before = guard.clone()
    out = guard[pad:pad + n].view(shape[0], shape[1], 3)
    out.fill_(NAN)
    a = abi_frame_metrics(pd, gd, mean, std, out=out).clone()
    out.fill_(NAN)
    b = abi_frame_metrics(pd, gd, mean, std, out=out).clone()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(guard[:pad].view(torch.int32), before[:pad].view(torch.int32))
    assert torch.equal(guard[pad + n:].view(torch.int32), before[pad + n:].view(torch.int32))


def test_non_contiguous_input(dev):
    import vptr_amd.ops as ops
    frames, gts, mean, std = make_pair((2, 5, 1, 20, 28), "smooth", 1010)
    fd, gd = frames.to(dev), gts.to(dev)
    pv, gv = fd[:, -3:], gd[:, -3:]
    assert not pv.is_contiguous()
    a = ops.frame_metrics(pv, gv, mean, std)
    b = ops.frame_metrics(pv.contiguous(), gv.contiguous(), mean, std)
    assert torch.equal(a, b)
    assert_close(a, ref_frame_metrics(frames[:, -3:], gts[:, -3:], mean, std), "non-contiguous view")


# ------------------------------------------------------------------------------------------------------ 4. the accumulator
def test_accumulate_adds_to_acc(dev):
    """direct C-ABI call on a pre-loaded accumulator: the kernel adds, it does not overwrite"""
    from vptr_amd._lib import check, lib, ptr, stream
    N, T = 5, 7
    per = fill.rand_input((N, T, 3), 1020, 0.5, 40.0).to(dev)
    pre = fill.rand_input((T, 3), 1021, -5.0, 5.0).double()
    acc = pre.to(dev)
    check(lib.vptr_frame_metrics_accumulate(ptr(per), ptr(acc), N, T, stream()), "vptr_frame_metrics_accumulate")
    want = pre + per.cpu().double().sum(dim=0)
    assert float((acc.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())
    check(lib.vptr_frame_metrics_accumulate(ptr(per), ptr(acc), N, T, stream()), "vptr_frame_metrics_accumulate")
    want = want + per.cpu().double().sum(dim=0)
    assert float((acc.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_frame_metrics_class_three_updates(dev):
    from vptr_amd.evaluate import FrameMetrics
    fm = FrameMetrics(3, KTH[0], KTH[1], device=dev)
    refs = []
    for i, n in enumerate((2, 1, 3)):
        pred, gt, mean, std = make_pair((n, 3, 1, 20, 28), KINDS[i], 1030 + 10 * i)
        refs.append(ref_frame_metrics(pred, gt, mean, std))
        fm.update(pred.to(dev), gt.to(dev))
    res = fm.compute()
    want = torch.cat(refs, dim=0).mean(dim=0)                     # [T, 3]: per-time-index means over the 6 samples
    assert res["samples"] == 6
    got = torch.from_numpy(np.stack([res["psnr"], res["mse"], res["ssim"]], axis=1))
    assert_close(got, want, "FrameMetrics 2 + 1 + 3 samples")
    fm.reset()
    assert fm.samples == 0 and float(fm.acc.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------ 5. guards
@pytest.mark.parametrize("frames,C,H,W,word", [(1, 1, 8, 257, "256"), (1, 1, 0, 8, "H"), (0, 1, 8, 8, "frames"), (1, 0, 8, 8, "C")])
def test_c_abi_rejects_unsupported_sizes(dev, frames, C, H, W, word):
    from vptr_amd._lib import lib, ptr, stream
    x = torch.zeros(4096, device=dev)
    ms = torch.ones(4, device=dev)
    scratch = torch.full((64,), 7.25, device=dev)
    out = torch.full((16,), 7.25, device=dev)
    rc = lib.vptr_frame_metrics(ptr(x), ptr(x), ptr(ms), ptr(ms), ptr(scratch), ptr(out), frames, C, H, W, 0, 1.0, stream())
    assert rc != 0
    msg = lib.vptr_last_error().decode()
    assert "frame_metrics" in msg and word in msg, msg
    assert lib.vptr_frame_metrics(None, ptr(x), ptr(ms), ptr(ms), ptr(scratch), ptr(out), 1, 1, 8, 8, 0, 1.0, stream()) != 0
    assert "null" in lib.vptr_last_error().decode()
    acc = torch.full((3,), 7.25, device=dev, dtype=torch.float64)
    assert lib.vptr_frame_metrics_accumulate(ptr(out), ptr(acc), 0, 1, stream()) != 0
    assert lib.vptr_frame_metrics_accumulate(ptr(out), None, 1, 1, stream()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((scratch == 7.25).all()) and bool((acc == 7.25).all())      # nothing was launched


def test_op_guards(dev):
    import vptr_amd.ops as ops
    x = torch.zeros((2, 2, 3, 8, 12), device=dev)
    with pytest.raises(RuntimeError, match="share"):
        ops.frame_metrics(x, x[:, :1])                                        # mismatched shapes
    with pytest.raises(RuntimeError, match="share"):
        ops.frame_metrics(x[0, 0, 0], x[0, 0, 0])                             # neither 4-d nor 5-d
    with pytest.raises(RuntimeError, match="float32"):
        ops.frame_metrics(x.half(), x.half())
    with pytest.raises(RuntimeError, match="float32"):
        ops.frame_metrics(x, x.double())
    with pytest.raises(RuntimeError, match="mean has 2 entries for 3 channels"):
        ops.frame_metrics(x, x, mean=(0.1, 0.2))
    with pytest.raises(RuntimeError, match="std has 4 entries for 3 channels"):
        ops.frame_metrics(x, x, std=torch.ones(4))
    with pytest.raises(RuntimeError, match="256"):
        ops.frame_metrics(torch.zeros((1, 1, 1, 2, 257), device=dev), torch.zeros((1, 1, 1, 2, 257), device=dev))
    with pytest.raises(RuntimeError, match=">= 1"):
        ops.frame_metrics(torch.zeros((1, 1, 1, 0, 8), device=dev), torch.zeros((1, 1, 1, 0, 8), device=dev))
    with pytest.raises(RuntimeError, match="acc must be"):
        ops.frame_metrics(x, x, acc=torch.zeros((2, 3), device=dev))                          # float32
    with pytest.raises(RuntimeError, match="acc must be"):
        ops.frame_metrics(x, x, acc=torch.zeros((3, 3), device=dev, dtype=torch.float64))     # wrong T
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.frame_metrics(x, x, acc=torch.zeros((2, 3), dtype=torch.float64))                 # acc on the host
    acc = torch.zeros((2, 3), device=dev, dtype=torch.float64)
    y = x.clone().requires_grad_(True)
    out = ops.frame_metrics(y, x, acc=acc)
    assert not out.requires_grad                                                              # no autograd
    assert float((acc[:, 2] - 2.0).abs().max()) < 1e-5                                        # SSIM 1 for each of the 2 samples


# ------------------------------------------------------------------------------------------------------ 6. end to end
def test_evaluate_rollout_far_cached(dev):
    """evaluate_rollout over a two-batch loader of KV-cached FAR rollouts (the tiny configuration of test_12_far_cache_gpu.py) against the
    notebook-style loop: vptr_amd.metrics' PSNR / SSIM / MSEScore per time index on the same rollout outputs, weighted by batch size"""
    import vptr_amd.model as pkg
    from vptr_amd import metrics as Mx
    from vptr_amd.evaluate import evaluate_rollout
    from vptr_amd.inference import far_rollout
    feat, HW, num_pred = 48, 64, 3
    enc = pkg.VPTREnc(1, feat, 3, "reflect").eval()
    dec = pkg.VPTRDec(1, feat, 3, "Sigmoid", "reflect").eval()
    fill.apply_fill(enc, 71)
    fill.apply_fill(dec, 72)
    far = build_transformer(pkg, dict(Tp=3, Tf=3, H=8, W=8, C=feat, nhead=8, window_size=4, num_encoder_layers=2, rpe=True), True)
    fill.apply_fill(far, 75)
    enc, dec, far = enc.to(dev), dec.to(dev), far.to(dev)
    mean, std = KTH

    def predict(past):
        return far_rollout(enc, dec, far, past, num_pred, mode="train", kv_cache=True)[1]

    loader = [(fill.rand_input((n, 3, 1, HW, HW), 1100 + i), (fill.rand_input((n, num_pred, 1, HW, HW), 1110 + i) - mean) / std)
              for i, n in enumerate((2, 1))]
    res = evaluate_rollout(predict, loader, num_pred, mean, std, device=dev)
    assert res["samples"] == 3

    ssim = Mx.SSIM().to(dev)
    want = np.zeros((num_pred, 3))
    for past, future in loader:
        pred = predict(past.to(dev))
        fut = future.to(dev)
        for t in range(num_pred):
            a, b = pred[:, t] * std + mean, fut[:, t] * std + mean
            want[t] += np.array([Mx.PSNR(a, b), Mx.MSEScore(a, b), float(ssim(a, b))]) * past.shape[0]
    want /= 3
    got = np.stack([res["psnr"], res["mse"], res["ssim"]], axis=1)
    assert_close(torch.from_numpy(got), torch.from_numpy(want), "evaluate_rollout vs vptr_amd.metrics loop")
