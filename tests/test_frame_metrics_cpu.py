"""On-device evaluation, host side: the tests' fp64 reference builder against the reference-generated golden values, the presence of the
feature (C-ABI entry points, op, module) and the host logic of FrameMetrics."""
import ctypes

import numpy as np
import pytest
import torch

from frame_metrics_ref import BAR_MSE_REL, BAR_PSNR, BAR_SSIM, ref_frame_metrics
from helpers import jload, load


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_builder_matches_reference_golden(tag):
    """the conv2d-in-double builder reproduces what the reference's PSNR / MSEScore / SSIM returned for metrics_tiny"""
    z = load("metrics_tiny")
    e = jload(z, "expected")[tag]
    x, y = torch.from_numpy(z["x:" + tag]), torch.from_numpy(z["y:" + tag])
    r = ref_frame_metrics(x, y)[:, 0]                        # (N, C, H, W) = N samples of one frame
    r255 = ref_frame_metrics(x * 255, y * 255, data_range=255.0)[:, 0]
    dp, dp255 = abs(float(r[:, 0].mean()) - e["psnr"]), abs(float(r255[:, 0].mean()) - e["psnr255"])
    dm = abs(float(r[:, 1].mean()) - e["mse"]) / abs(e["mse"])
    ds = float((r[:, 2] - torch.tensor(e["ssim_each"], dtype=torch.float64)).abs().max())
    dsm = abs(float(r[:, 2].mean()) - e["ssim"])
    print("builder vs golden %s: psnr %.3e psnr255 %.3e mse rel %.3e ssim_each %.3e ssim %.3e" % (tag, dp, dp255, dm, ds, dsm))
    assert dp < BAR_PSNR and dp255 < BAR_PSNR
    assert dm < BAR_MSE_REL
    assert ds < BAR_SSIM and dsm < BAR_SSIM


def test_reference_builder_renormalises_and_clamps():
    """mean / std / clamp of the builder against the same metrics on images prepared by hand"""
    x, y = torch.rand(2, 3, 3, 9, 12) * 1.4 - 0.2, torch.rand(2, 3, 3, 9, 12) * 1.4 - 0.2
    mean, std = (0.1, 0.2, 0.3), (2.0, 0.5, 1.5)
    m, s = torch.tensor(mean).view(1, 1, 3, 1, 1), torch.tensor(std).view(1, 1, 3, 1, 1)
    a = ref_frame_metrics((x - m) / s, (y - m) / s, mean, std, clamp=True)
    b = ref_frame_metrics(x.clamp(0, 1), y.clamp(0, 1))
    assert float((a - b).abs().max()) < 1e-4       # float32 round trip of (x - m) / s * s + m
    assert tuple(a.shape) == (2, 3, 3)


def test_feature_is_present():
    from vptr_amd import _lib
    for name in ("vptr_frame_metrics", "vptr_frame_metrics_accumulate"):
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert len(_lib.SIGNATURES["vptr_frame_metrics"]) == 13 and len(_lib.SIGNATURES["vptr_frame_metrics_accumulate"]) == 5
    assert _lib.lib.vptr_abi_version() == 10
    import vptr_amd.evaluate as E
    import vptr_amd.ops as ops
    assert callable(E.evaluate_rollout) and callable(E.FrameMetrics) and callable(ops.frame_metrics)
    x = torch.zeros(1, 2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.frame_metrics(x, x)


def test_frame_metrics_host_logic(monkeypatch):
    """samples count, the division by it and reset(), with update() replaced by one that adds known per-frame values"""
    from vptr_amd.evaluate import FrameMetrics
    T = 4

    def fake_update(self, pred, gt):
        self.acc += pred.double().sum(dim=0)          # pred: [N, T, 3] of (psnr, sse, ssim) per frame
        self.samples += int(pred.shape[0])

    monkeypatch.setattr(FrameMetrics, "update", fake_update)
    fm = FrameMetrics(T, device="cpu")
    assert fm.samples == 0 and tuple(fm.acc.shape) == (T, 3) and fm.acc.dtype == torch.float64
    with pytest.raises(RuntimeError):
        fm.compute()
    rs = np.random.RandomState(5)
    batches = [torch.from_numpy(rs.uniform(0.5, 30.0, size=(n, T, 3)).astype(np.float32)) for n in (2, 1, 3)]
    for b in batches:
        fm.update(b, None)
    out = fm.compute()
    allv = torch.cat(batches, dim=0).double().mean(dim=0).numpy()
    assert out["samples"] == 6 and set(out) == {"psnr", "ssim", "mse", "samples"}
    for key, col in (("psnr", 0), ("mse", 1), ("ssim", 2)):
        assert out[key].shape == (T,) and out[key].dtype == np.float64
        assert np.allclose(out[key], allv[:, col], rtol=1e-12, atol=0)
    fm.reset()
    assert fm.samples == 0 and float(fm.acc.abs().sum()) == 0.0
    fm.update(batches[1], None)
    assert fm.compute()["samples"] == 1 and np.allclose(fm.compute()["ssim"], batches[1][0, :, 2].double().numpy(), rtol=1e-12)
