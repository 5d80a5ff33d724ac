"""Reference builder for the clip-ingest tests: crop, PIL's two integer resize passes with the rounding to uint8 between them, the
flips, then float32 / 255, - mean, / std with torch fp32 operations.  Vectorised numpy, written from Pillow's algorithm
(precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc) and pinned against PIL
itself and against a PIL-written fixture by test_ingest_cpu.py.  It does not use vptr_amd.data."""
import numpy as np
import torch

KINDS = ("random", "binary", "ramp")

# (Hin, Win, C, crop box or None, (Hout, Wout)): the geometries the tables and the builder are checked on against PIL
PIL_GEOMETRIES = [
    (120, 120, 1, None, (64, 64)),
    (120, 120, 1, None, (128, 128)),
    (120, 160, 1, None, (64, 64)),
    (64, 64, 3, None, (64, 64)),
    (37, 53, 3, None, (16, 24)),
    (9, 7, 1, None, (20, 13)),
    (120, 120, 3, None, (64, 64)),
    (5, 300, 1, None, (3, 64)),
    (240, 240, 1, None, (64, 64)),
    (64, 64, 3, None, (128, 128)),
]

# tag -> geometry of the PIL-written fixture tests/golden/ingest_pil.npz (tools/make_ingest_golden.py holds the same list)
GOLDEN_GEOMETRIES = {
    "kth64": (120, 160, 1, (0, 20, 120, 120), (64, 64)),
    "kth128": (120, 160, 1, (0, 20, 120, 120), (128, 128)),
    "bair": (64, 64, 3, None, (64, 64)),
    "odd": (37, 53, 3, (3, 5, 31, 41), (16, 24)),
    "down4": (240, 240, 1, None, (64, 64)),
}


def make_raw(shape, kind, seed):
    """uint8 [N, T, H, W, C]: uniform random bytes, random 0 / 255, or a diagonal ramp that differs per frame and channel"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randint(0, 256, size=shape).astype(np.uint8)
    if kind == "binary":
        return (rs.randint(0, 2, size=shape) * 255).astype(np.uint8)
    if kind == "ramp":
        N, T, H, W, C = shape
        n, t, y, x, c = np.meshgrid(np.arange(N), np.arange(T), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        return ((3 * x + 5 * y + 41 * c + 17 * t + 29 * n) % 256).astype(np.uint8)
    raise ValueError(kind)


def ref_tables(in_size, out_size):
    """(k int64 [out, ksize], first int64 [out], count int64 [out]) in float64, sums in index order as the C loop runs them"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    first = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    last = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = last - first
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(((j + first[:, None]) - center[:, None] + 0.5) * (1.0 / fs)))
    w[j >= count[:, None]] = 0.0
    ww = np.cumsum(w, axis=1)[:, -1:]                      # sequential, like the C loop (trailing zeros change nothing)
    k = np.trunc(0.5 + (w / ww) * float(1 << 22)).astype(np.int64)
    return k, first, count


def _resize_last_axis(a, out_size):
    """a: uint8 [..., in] -> uint8 [..., out]: one PIL pass along the last axis"""
    in_size = a.shape[-1]
    k, first, count = ref_tables(in_size, out_size)
    idx = np.minimum(first[:, None] + np.arange(k.shape[1])[None, :], in_size - 1)     # [out, ksize]; taps past the count have k = 0
    g = a[..., idx].astype(np.int64)                                                   # [..., out, ksize]
    ss = (1 << 21) + (g * k).sum(axis=-1)
    return np.clip(ss >> 22, 0, 255).astype(np.uint8)


def ref_resize_u8(raw, crop, out_hw):
    """raw: uint8 [N, T, H, W, C] -> uint8 [N, T, Hout, Wout, C]: crop, horizontal pass, vertical pass (a pass that keeps the size is
    not run)"""
    if crop is not None:
        top, left, th, tw = crop
        raw = raw[:, :, top:top + th, left:left + tw, :]
    Hout, Wout = out_hw
    a = raw
    if Wout != a.shape[3]:
        a = np.moveaxis(_resize_last_axis(np.moveaxis(a, 3, -1), Wout), -1, 3)
    if Hout != a.shape[2]:
        a = np.moveaxis(_resize_last_axis(np.moveaxis(a, 2, -1), Hout), -1, 2)
    return np.ascontiguousarray(a)


def normalise_u8(img, mean, std):
    """uint8 [N, T, H, W, C] -> fp32 torch [N, T, C, H, W]: ToTensor and Normalize as fp32 torch operations"""
    C = img.shape[-1]
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(0, 1, 4, 2, 3).contiguous().to(torch.float32).div(255)
    m = torch.tensor([float(mean)] * C if isinstance(mean, (int, float)) else [float(e) for e in mean], dtype=torch.float32)
    s = torch.tensor([float(std)] * C if isinstance(std, (int, float)) else [float(e) for e in std], dtype=torch.float32)
    return x.sub(m.view(1, 1, C, 1, 1)).div(s.view(1, 1, C, 1, 1))


def ref_ingest(raw, crop, out_hw, mean=0.0, std=1.0, flips=None):
    """the whole transform: fp32 torch [N, T, C, Hout, Wout]; flips: int [N], bit 0 horizontal, bit 1 vertical, after the resize"""
    img = ref_resize_u8(raw, crop, out_hw).copy()
    if flips is not None:
        for n, f in enumerate(np.asarray(flips).tolist()):
            if f & 1:
                img[n] = img[n, :, :, ::-1, :]
            if f & 2:
                img[n] = img[n, :, ::-1, :, :]
    return normalise_u8(img, mean, std)
