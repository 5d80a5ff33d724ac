"""fp64 reference builder and test images shared by tests/test_frame_metrics_cpu.py and tests/test_13_frame_metrics_gpu.py.

The builder is a second formulation of the metrics, independent of the banded matrix products of vptr_amd.metrics and of the separable
kernel under test: renormalisation, optional clamp, and ONE grouped F.conv2d in double with the 11 x 11 window and padding 5 per blurred
quantity.  test_frame_metrics_cpu.py pins it to the reference-generated values of tests/golden/metrics_tiny.npz."""
import math

import torch
import torch.nn.functional as F

from oracle import fill

KTH = (0.6013795, 2.7570653)                                                             # utils/dataset.py:19-33
BAIR = ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673))          # utils/dataset.py:49-50

# the project's bars for these metrics (tests/test_02_model_gpu.py::test_metrics_on_device)
BAR_SSIM, BAR_PSNR, BAR_MSE_REL = 1e-5, 1e-4, 1e-5


def window2d():
    """the reference's float32 11 x 11 window (utils/metrics.py:75-84), as double"""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / float(2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).double()


def _chan(v, C):
    t = torch.as_tensor(v, dtype=torch.float32).reshape(-1).double()   # the values the kernel sees are float32
    return (t.expand(C) if t.numel() == 1 else t).view(1, C, 1, 1)


def ref_frame_metrics(pred, gt, mean=0.0, std=1.0, clamp=False, data_range=1.0):
    """pred, gt (N, T, C, H, W) or (N, C, H, W) float32 -> double [N, T, 3] of (psnr dB, sse, ssim) per frame"""
    if pred.dim() == 4:
        pred, gt = pred.unsqueeze(1), gt.unsqueeze(1)
    N, T, C, H, W = pred.shape
    x = pred.detach().cpu().double().reshape(N * T, C, H, W) * _chan(std, C) + _chan(mean, C)
    y = gt.detach().cpu().double().reshape(N * T, C, H, W) * _chan(std, C) + _chan(mean, C)
    if clamp:
        x, y = x.clamp(0.0, 1.0), y.clamp(0.0, 1.0)
    sse = ((x - y) ** 2).sum(dim=(1, 2, 3))
    psnr = -10.0 * torch.log10(((x / data_range - y / data_range) ** 2).mean(dim=(1, 2, 3)) + 1e-8)
    w = window2d().expand(C, 1, 11, 11).contiguous()

    def blur(t):
        return F.conv2d(t, w, padding=5, groups=C)

    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return torch.stack([psnr, sse, m.mean(dim=(1, 2, 3))], dim=1).reshape(N, T, 3)


def assert_close(got, ref, what):
    """got, ref [..., 3] (psnr, sse, ssim) at the project's bars; prints the distances before it asserts; returns them"""
    got, ref = torch.as_tensor(got).detach().cpu().double().reshape(-1, 3), torch.as_tensor(ref).double().reshape(-1, 3)
    assert bool(torch.isfinite(got).all()), what
    dp = float((got[:, 0] - ref[:, 0]).abs().max())
    dm = float(((got[:, 1] - ref[:, 1]).abs() / ref[:, 1].abs().clamp_min(1e-300)).max())
    ds = float((got[:, 2] - ref[:, 2]).abs().max())
    print("frame_metrics %s: |dPSNR| %.3e dB  rel dSSE %.3e  |dSSIM| %.3e" % (what, dp, dm, ds))
    assert dp < BAR_PSNR and dm < BAR_MSE_REL and ds < BAR_SSIM, (what, dp, dm, ds)
    return dp, dm, ds


KINDS = ("noise", "smooth", "saturated")


def norm_consts(C):
    return KTH if C == 1 else BAIR


def make_pair(shape, kind, seed, stretch=False):
    """(pred, gt, mean, std): images in [0, 1] of one of three kinds, gt = 0.8 img + 0.2 noise, both mapped into the model's range with
    the dataset constants (KTH for C = 1, BAIR for C = 3).  stretch: images stretched to [-0.1, 1.1] first, so that a clamp matters."""
    N, T, C, H, W = shape
    u = fill.rand_input(shape, seed)
    if kind == "noise":
        img = u
    else:
        low = fill.rand_input((N * T, C, max(2, (H + 7) // 8), max(2, (W + 7) // 8)), seed + 1)
        img = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).reshape(shape)
        if kind == "saturated":
            img = torch.sigmoid(8.0 * (img - 0.5))      # decoder-like frames: most pixels near 0 or 1
        elif kind != "smooth":
            raise ValueError(kind)
    gt = 0.8 * img + 0.2 * fill.rand_input(shape, seed + 2)
    if stretch:
        img, gt = img * 1.2 - 0.1, gt * 1.2 - 0.1
    mean, std = norm_consts(C)
    m = torch.tensor(mean, dtype=torch.float32).reshape(1, 1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).reshape(1, 1, -1, 1, 1)
    return ((img - m) / s).float().contiguous(), ((gt - m) / s).float().contiguous(), mean, std
