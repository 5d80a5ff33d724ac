"""Plain-torch CPU builder of the sample panels (tests/test_panels_cpu.py, tests/test_15_panels_gpu.py): a transcription, operation by
operation, of what the reference runs per frame -- append_frames' torch.cat with a repeat of batch[:, -2:-1], torch.cat(dim=-1), the two
transforms.Normalize calls of VidReNormalize (tensor.sub_(mean).div_(std) with (C, 1, 1) fp32 tensors of the constants), torch.clamp and
ToPILImage's mul(255).byte() -- written from those semantics (torchvision is not installed).  Literal on purpose: no fused or reordered
arithmetic, one frame at a time."""
import numpy as np
import torch

KTH = (0.6013795, 2.7570653)
BAIR = ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673))
MNIST = (0.0, 1.0)


def consts(C):
    return KTH if C == 1 else BAIR


def per_channel(v, C):
    return [float(v)] * C if isinstance(v, (int, float)) else [float(e) for e in v]


def renorm_constants(mean, std, C):
    """(inv_std, inv_mean) as VidReNormalize holds them: python floats 1.0 / s and -m"""
    return [1.0 / s for s in per_channel(std, C)], [-m for m in per_channel(mean, C)]


def normalize(img, mean, std):
    """transforms.Normalize on one (C, H, W) fp32 image: a clone, then sub_(mean).div_(std) with the constants as (C, 1, 1) fp32 tensors"""
    img = img.clone()
    m = torch.as_tensor(mean, dtype=img.dtype).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=img.dtype).view(-1, 1, 1)
    return img.sub_(m).div_(s)


def frame_bytes(img, inv_std=None, inv_mean=None, clamp=False, nearest=False, saturate=False):
    """one (C, H, W) fp32 frame -> uint8 (H, W, C).  saturate: q < 0 -> 0, q > 255 -> 255, NaN -> 0 before the cast, which changes nothing
    where .byte() is defined (test_panels_cpu.py) and defines it elsewhere"""
    C = img.shape[0]
    if inv_std is not None:
        img = normalize(img, [0.0] * C, inv_std)           # Normalize(mean=0, std=inv_std)
        img = normalize(img, inv_mean, [1.0] * C)          # Normalize(mean=inv_mean, std=1)
    if clamp:
        img = torch.clamp(img, min=0.0, max=1.0)
    q = img.mul(255)
    if nearest:
        q = q.add(0.5)
    if saturate:
        q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 255.0)
    return q.byte().permute(1, 2, 0).contiguous()


def append_frames(batch, length, pad):
    d = length - batch.shape[1]
    if d == 0:
        return batch
    if pad == "reference":
        assert batch.shape[1] >= 2
        return torch.cat([batch, batch[:, -2:-1, :, :, :].repeat(1, d, 1, 1, 1)], dim=1)
    if pad == "last":
        return torch.cat([batch, batch[:, -1:, :, :, :].repeat(1, d, 1, 1, 1)], dim=1)
    return torch.cat([batch, torch.zeros_like(batch[:, :1]).repeat(1, d, 1, 1, 1)], dim=1)     # "blank": the bytes are zeroed below


def ref_panels(clips, mean=None, std=None, clamp=None, quantize="floor", layout="frames", pad="reference", gray_to_rgb=False,
               saturate=False):
    """clips: fp32 CPU tensors [N, T_k, C, H, W] -> uint8 tensor, frames [N, L, H, K W, Cout] or sheet [N, K H, L W, Cout]"""
    clips = [c.detach().cpu().float() for c in clips]
    N, _, C, H, W = clips[0].shape
    K, L = len(clips), max(c.shape[1] for c in clips)
    inv_std = inv_mean = None
    if mean is not None:
        inv_std, inv_mean = renorm_constants(mean, std, C)
    if clamp is None:
        clamp = mean is not None
    lengths = [c.shape[1] for c in clips]
    batch = torch.cat([append_frames(c, L, pad) for c in clips], dim=-1)           # (N, L, C, H, K W)
    out = torch.empty((N, L, H, K * W, C), dtype=torch.uint8)
    for n in range(N):
        for t in range(L):
            out[n, t] = frame_bytes(batch[n, t], inv_std, inv_mean, clamp, quantize == "nearest", saturate)
    if pad == "blank":
        for k, T in enumerate(lengths):
            out[:, T:, :, k * W:(k + 1) * W, :] = 0
    if gray_to_rgb and C == 1:
        out = out.repeat(1, 1, 1, 1, 3)
    if layout == "sheet":                                                          # clip k: one row of its L frames
        Cout = out.shape[-1]
        out = out.reshape(N, L, H, K, W, Cout).permute(0, 3, 2, 1, 4, 5).reshape(N, K * H, L * W, Cout)
    return out.contiguous()


# ---------------------------------------------------------------------------------------------------------------- test images
def grid_clip(shape, seed, mean=None, std=None):
    """(fp32 clip [N, T, C, H, W], its bytes uint8 [N, T, H, W, C]): random bytes v through v / 255 -> (. - mean) / std in fp32, ToTensor +
    Normalize as ClipIngest runs them.  The decisive kind: on this grid a reordered, fused or reciprocal renormalisation changes bytes."""
    N, T, C, H, W = shape
    if mean is None:
        mean, std = consts(C)
    v = np.random.RandomState(seed).randint(0, 256, size=(N, T, H, W, C)).astype(np.uint8)
    x = torch.from_numpy(v).permute(0, 1, 4, 2, 3).float().div(255)
    m = torch.tensor(per_channel(mean, C), dtype=torch.float32).view(1, 1, C, 1, 1)
    s = torch.tensor(per_channel(std, C), dtype=torch.float32).view(1, 1, C, 1, 1)
    return x.sub(m).div(s).contiguous(), v


def spread_clip(shape, seed, mean=None, std=None):
    """(u - mean) / std with u ~ U(-0.1, 1.2): about 8 % of the values below 0 and 15 % above 1, so the clamp and both ends matter"""
    N, T, C, H, W = shape
    if mean is None:
        mean, std = consts(C)
    u = torch.from_numpy(np.random.RandomState(seed).uniform(-0.1, 1.2, size=shape).astype(np.float32))
    m = torch.tensor(per_channel(mean, C), dtype=torch.float32).view(1, 1, C, 1, 1)
    s = torch.tensor(per_channel(std, C), dtype=torch.float32).view(1, 1, C, 1, 1)
    return u.sub(m).div(s).contiguous()


def special_values():
    """NaN, +-inf, +-0, exactly 1, its two neighbours, values just outside [0, 1] and far outside"""
    one = np.float32(1.0)
    return torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, float(np.nextafter(one, np.float32(0))),
                         float(np.nextafter(one, np.float32(2))), -1e-6, 1.0 + 1e-6, -0.003, 1.003, -1.5, 3.0, 0.5, 254.5 / 255, 1e30, -1e30],
                        dtype=torch.float32)
