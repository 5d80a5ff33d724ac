"""Sample panels, host side: the tests' literal builder (panels_ref.py) against a second, vectorised formulation, the ReNorm constants,
the pad rules, what the two quantisations return of frames that came from uint8 data, a GIF round trip through PIL, the presence of the
feature (C-ABI entry point, op, module) and the argument guards that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vptr_amd.ops.panels import pad_indices, panel_shape          # the module under test: without it nothing in this file can pass
from panels_ref import BAIR, KTH, MNIST, consts, frame_bytes, grid_clip, per_channel, ref_panels, renorm_constants, special_values, spread_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    """a float64 result rounded to fp32: for one +, -, * or / of two fp32 values this IS the fp32 operation (53 >= 2 * 24 + 2 bits)"""
    return x.to(torch.float32)


def vector_panels(clips, mean=None, std=None, clamp=None, quantize="floor", layout="frames", pad="reference", gray_to_rgb=False):
    """the independent formulation: frames gathered by an index table instead of cat + repeat, every fp32 operation as a float64 operation
    rounded once, the truncation as numpy's float -> int64 cast, the panel filled cell by cell"""
    N, _, C, H, W = clips[0].shape
    K, L = len(clips), max(c.shape[1] for c in clips)
    Cout = 3 if gray_to_rgb and C == 1 else C
    cells = np.zeros((K, N, L, H, W, Cout), dtype=np.uint8)
    for k, c in enumerate(clips):
        T = c.shape[1]
        src = [t if t < T else {"reference": T - 2, "last": T - 1, "blank": -1}[pad] for t in range(L)]
        z = c[:, [max(s, 0) for s in src]]
        if mean is not None:
            a = torch.tensor([1.0 / s for s in per_channel(std, C)], dtype=torch.float64).to(torch.float32).view(1, 1, C, 1, 1)
            b = torch.tensor([-m for m in per_channel(mean, C)], dtype=torch.float64).to(torch.float32).view(1, 1, C, 1, 1)
            z = f32(f32(z.double() / a.double()).double() - b.double())
        if (mean is not None) if clamp is None else clamp:
            z = z.clamp(0.0, 1.0)
        q = f32(z.double() * 255.0)
        if quantize == "nearest":
            q = f32(q.double() + 0.5)
        by = q.numpy().astype(np.int64).astype(np.uint8)                  # (N, L, C, H, W), truncated
        by = np.moveaxis(by, 2, -1)
        by[:, [i for i, s in enumerate(src) if s < 0]] = 0
        cells[k] = np.repeat(by, 3, axis=-1) if Cout != C else by
    if layout == "frames":
        return torch.from_numpy(np.concatenate(list(cells), axis=3))      # along W
    return torch.from_numpy(np.concatenate([np.concatenate(list(cells[k].transpose(1, 0, 2, 3, 4)), axis=2) for k in range(K)], axis=1))


CASES = [((2, 3, 1, 5, 7), (3, 3, 3)), ((1, 5, 3, 4, 6), (2, 5, 5)), ((3, 7, 1, 3, 4), (3, 7, 6)), ((2, 4, 3, 2, 2), (4,)),
         ((1, 3, 1, 6, 5), (3, 3, 3, 3))]


@pytest.mark.parametrize("shape,lengths", CASES, ids=lambda v: "x".join(str(e) for e in v))
def test_builder_matches_the_vectorised_formulation(shape, lengths):
    N, _, C, H, W = shape
    mean, std = consts(C)
    clips = [grid_clip((N, T, C, H, W), 8000 + 10 * len(lengths) + k)[0] if k % 2 == 0 else spread_clip((N, T, C, H, W), 8100 + k)
             for k, T in enumerate(lengths)]
    for layout in ("frames", "sheet"):
        for pad in ("reference", "last", "blank"):
            for quantize in ("floor", "nearest"):
                for rgb in (False, True):
                    got = ref_panels(clips, mean, std, quantize=quantize, layout=layout, pad=pad, gray_to_rgb=rgb)
                    want = vector_panels(clips, mean, std, quantize=quantize, layout=layout, pad=pad, gray_to_rgb=rgb)
                    assert tuple(got.shape) == panel_shape(N, lengths, C, H, W, layout, rgb) and got.dtype == torch.uint8
                    assert torch.equal(got, want), (layout, pad, quantize, rgb)
    unit = [c.sub(c.min()).div(c.max() - c.min()) for c in clips]                                  # no renormalisation: values in [0, 1]
    assert torch.equal(ref_panels(unit), vector_panels(unit)) and torch.equal(ref_panels(unit, clamp=True), vector_panels(unit, clamp=True))


def test_builder_is_the_reference_layout():
    """on values whose bytes can be read off: cat along W, HWC, pad = frame T - 2"""
    past = torch.arange(2 * 2 * 1 * 2 * 3, dtype=torch.float32).reshape(2, 2, 1, 2, 3) / 255
    fut = (100 + torch.arange(2 * 4 * 1 * 2 * 3, dtype=torch.float32).reshape(2, 4, 1, 2, 3)) / 255
    out = ref_panels([past, fut, fut], quantize="nearest")
    assert tuple(out.shape) == (2, 4, 2, 9, 1)
    assert out[1, 1, 1, :, 0].tolist() == [21, 22, 23, 133, 134, 135, 133, 134, 135]
    assert torch.equal(out[:, 2:, :, :3], out[:, 0:1, :, :3].repeat(1, 2, 1, 1, 1))               # 2 past frames: frame 0 is repeated
    sheet = ref_panels([past, fut], quantize="nearest", layout="sheet", pad="blank", gray_to_rgb=True)
    assert tuple(sheet.shape) == (2, 4, 12, 3)
    assert sheet[0, 1, :, 1].tolist() == [3, 4, 5, 9, 10, 11, 0, 0, 0, 0, 0, 0] and sheet[0, 2, :4, 2].tolist() == [100, 101, 102, 106]


def test_saturation_only_acts_where_the_cast_is_undefined():
    """frame_bytes(saturate=True) equals the literal mul(255).byte() wherever -1 < q < 256 (C's float -> integer conversion is defined when
    the truncated value fits), and gives 0 / 255 / 0 for q <= -1, q >= 256, NaN"""
    x = torch.cat([special_values(), torch.linspace(-1.0 / 255 + 1e-6, 256.0 / 255 - 1e-6, 4001)]).view(1, 1, -1)
    q = x.mul(255)
    defined = (q > -1) & (q < 256)
    assert int(defined.sum()) > 4000
    lit, sat = frame_bytes(x)[..., 0].view(-1), frame_bytes(x, saturate=True)[..., 0].view(-1)
    assert torch.equal(lit[defined.view(-1)], sat[defined.view(-1)])
    vals = dict(zip(special_values().tolist()[1:], sat.tolist()[1:]))
    assert sat[0] == 0 and vals[float("inf")] == 255 and vals[float("-inf")] == 0 and vals[3.0] == 255 and vals[-1.5] == 0 and vals[1.0] == 255
    assert vals[float(np.nextafter(np.float32(1), np.float32(0)))] == 254 and vals[0.5] == 127
    assert frame_bytes(torch.tensor([0.5]).view(1, 1, 1), nearest=True).item() == 128


@pytest.mark.parametrize("mean,std,C", [KTH + (1,), BAIR + (3,), MNIST + (1,), (0.5, 0.25, 3)])
def test_renorm_constants(mean, std, C):
    from vptr_amd.visualize import ReNorm
    inv_std, inv_mean = renorm_constants(mean, std, C)
    a, b = ReNorm(mean, std).constants(C)
    assert a.dtype == b.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (C,)
    assert torch.equal(a, torch.as_tensor(inv_std, dtype=torch.float32)) and torch.equal(b, torch.as_tensor(inv_mean, dtype=torch.float32))
    for c in range(C):                                              # 1.0 / std in double, rounded once; not the fp32 reciprocal of fp32(std)
        assert float(a[c]) == float(np.float32(1.0 / per_channel(std, C)[c])) and float(b[c]) == float(np.float32(-per_channel(mean, C)[c]))

    class Theirs:                                                   # the attributes of a VidReNormalize instance
        pass
    t = Theirs()
    t.inv_std, t.inv_mean = (inv_std, inv_mean) if isinstance(mean, tuple) else (inv_std[0], inv_mean[0])
    a2, b2 = ReNorm(t).constants(C)
    assert torch.equal(a2, a) and torch.equal(b2, b) and ReNorm.of(t).inv_std == t.inv_std and ReNorm.of(None) is None
    with pytest.raises(ValueError):
        ReNorm(BAIR[0], BAIR[1]).constants(1)
    with pytest.raises(ValueError):
        ReNorm(0.5)


def test_pad_rules():
    assert pad_indices([10, 10, 10]) == [-1, -1, -1]
    assert pad_indices([2, 5, 5]) == [0, -1, -1]                    # two past frames: frame 0, as the reference does for BAIR
    assert pad_indices([3, 7, 6]) == [1, -1, 4]
    assert pad_indices([3, 7, 6], "last") == [2, -1, 5] and pad_indices([3, 7, 6], "blank") == [-1, -1, -1]
    assert pad_indices([1, 1]) == [-1, -1] and pad_indices([1, 3], "last") == [0, -1]
    with pytest.raises(RuntimeError, match="T = 1 < 2"):
        pad_indices([1, 3])                                         # batch[:, -2:-1] of one frame is empty
    with pytest.raises(RuntimeError, match=">= 1"):
        pad_indices([0, 3])
    with pytest.raises(ValueError, match="pad must be"):
        pad_indices([2, 3], "edge")
    assert panel_shape(2, [2, 5, 5], 1, 8, 4) == (2, 5, 8, 12, 1) and panel_shape(2, [2, 5, 5], 1, 8, 4, "sheet", True) == (2, 24, 20, 3)
    assert panel_shape(1, [4], 3, 8, 4, gray_to_rgb=True) == (1, 4, 8, 4, 3)


# levels (of 256 per channel) that ingest -> renormalise -> quantise returns unchanged
FLOOR_SHARES = {"kth": 210, "bair": 586, "mnist": 256}


@pytest.mark.parametrize("name,ms,C", [("kth", KTH, 1), ("bair", BAIR, 3), ("mnist", MNIST, 1)])
def test_nearest_returns_every_level_floor_does_not(name, ms, C):
    """all 256 levels per channel through ToTensor + Normalize and back: round-to-nearest returns every one, ToPILImage's truncation 82 % of
    them with the KTH constants (210 of 256) and 76 % with BAIR's (586 of 768); MovingMNIST's (0, 1) lose nothing (v / 255 * 255 == v)"""
    v = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16, 1), C, axis=4)
    x = torch.from_numpy(v).permute(0, 1, 4, 2, 3).float().div(255)
    x = torch.stack([x[:, :, c].sub(torch.tensor(per_channel(ms[0], C)[c])).div(torch.tensor(per_channel(ms[1], C)[c])) for c in range(C)], dim=2)
    near = ref_panels([x], ms[0], ms[1], quantize="nearest")
    assert torch.equal(near, torch.from_numpy(v))
    kept = int((ref_panels([x], ms[0], ms[1]) == torch.from_numpy(v)).sum())
    print("%s: floor returns %d of %d levels (%.1f %%)" % (name, kept, 256 * C, 100.0 * kept / (256 * C)))
    assert kept == FLOOR_SHARES[name]
    assert int((ref_panels([x], ms[0], ms[1]).int() - torch.from_numpy(v).int()).abs().max()) <= 1


def test_spread_images_reach_both_ends():
    for C in (1, 3):
        out = ref_panels([spread_clip((2, 3, C, 16, 16), 8200 + C)], *consts(C))
        lo, hi = float((out == 0).float().mean()), float((out == 255).float().mean())
        assert 0.02 < lo < 0.20 and 0.02 < hi < 0.20, (lo, hi)


def test_grid_images_see_every_arithmetic_shortcut():
    """why the GPU tests use grid images with the KTH / BAIR constants: each of the four arithmetic-only changes a kernel could make moves
    bytes on them, and none of them moves a byte with MovingMNIST's constants (0, 1)"""
    for C, ms in ((1, KTH), (3, BAIR), (1, MNIST)):
        x = grid_clip((2, 3, C, 16, 16), 8400 + C, *ms)[0]
        ref = ref_panels([x], *ms)
        a = torch.tensor([1.0 / s for s in per_channel(ms[1], C)], dtype=torch.float64).to(torch.float32).view(1, 1, C, 1, 1)
        b = torch.tensor([-m for m in per_channel(ms[0], C)], dtype=torch.float64).to(torch.float32).view(1, 1, C, 1, 1)
        std = torch.tensor(per_channel(ms[1], C), dtype=torch.float32).view(1, 1, C, 1, 1)
        mutants = {"x * std + mean": x * std - b,
                   "fused multiply-add": f32(x.double() * std.double() - b.double()),
                   "x * (1 / a)": x * (1.0 / a) - b,
                   "+ 0.5 in floor mode": None}
        for name, z in mutants.items():
            q = ((x / a) - b).clamp(0.0, 1.0).mul(255).add(0.5) if z is None else z.clamp(0.0, 1.0).mul(255)
            share = float((q.byte().permute(0, 1, 3, 4, 2) != ref).float().mean())
            print("C %d mean %s: %-20s changes %.1f %% of the bytes" % (C, ms[0], name, 100 * share))
            assert (share == 0.0) if ms is MNIST else (share > 0.03), (C, name, share)
        assert torch.equal(((x / a) - b).clamp(0.0, 1.0).mul(255).byte().permute(0, 1, 3, 4, 2), ref)      # the chain itself, vectorised


def test_gif_round_trip(tmp_path):
    """a GIF written from builder arrays re-opens to the same frames in mode L"""
    Image = pytest.importorskip("PIL.Image")
    from vptr_amd.visualize import save_gifs
    clips = [grid_clip((2, T, 1, 8, 8), 8300 + T)[0] for T in (2, 4, 4)]
    panels = ref_panels(clips, *KTH).numpy()
    paths = save_gifs(panels, tmp_path / "gifs", desc="pred")
    assert [p.name for p in paths] == ["pred_clip_0.gif", "pred_clip_1.gif"]
    for n, p in enumerate(paths):
        with Image.open(p) as im:
            assert im.n_frames == 4
            for t in range(4):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("L")), panels[n, t, :, :, 0]), (n, t)
    with pytest.raises(ValueError):
        save_gifs(panels[..., 0], tmp_path, "x")


def test_feature_is_present():
    from vptr_amd import _lib
    from vptr_amd.build import SOURCES
    assert "panels.hip" in SOURCES
    assert "vptr_clip_panels" in _lib.SIGNATURES and "vptr_clip_panels" in _lib.EXPORTS
    assert len(_lib.SIGNATURES["vptr_clip_panels"]) == 18 and len(_lib.EXPORTS) == 77
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vptr_clip_panels")
    with open(os.path.join(ROOT, "include", "vptr_hip.h")) as f:
        assert re.search(r"\bint\s+vptr_clip_panels\s*\(", f.read())
    assert _lib.lib.vptr_abi_version() == 10
    import vptr_amd.ops as ops
    import vptr_amd.visualize as V
    assert callable(ops.clip_panels) and ops.PANELS_MAX_CLIPS == 4
    for name in ("ReNorm", "clips_to_uint8", "visualize_batch_clips", "nar_show_samples", "far_show_samples", "ae_show_samples", "export_rollout"):
        assert callable(getattr(V, name)), name


def test_c_abi_guards_without_a_device():
    """every check comes before the launch, so the host-side ones can be reached with pointers that are never dereferenced on a device"""
    from vptr_amd._lib import lib
    K = 2
    clips, T = (ctypes.c_void_p * K)(4096, 8192), (ctypes.c_int32 * K)(3, 5)
    sn, st, pad = (ctypes.c_int64 * K)(64, 64), (ctypes.c_int64 * K)(16, 16), (ctypes.c_int32 * K)(1, -1)
    out = ctypes.c_void_p(4096)
    good = dict(clips=clips, T=T, sn=sn, st=st, pad=pad, a=None, b=None, out=out, K=K, N=1, C=1, H=4, W=4, clamp=0, nearest=0, rgb=0, layout=0)

    def call(**change):
        a = dict(good, **change)
        rc = lib.vptr_clip_panels(a["clips"], a["T"], a["sn"], a["st"], a["pad"], a["a"], a["b"], a["out"], a["K"], a["N"], a["C"], a["H"],
                                  a["W"], a["clamp"], a["nearest"], a["rgb"], a["layout"], None)
        assert rc != 0
        msg = lib.vptr_last_error().decode()
        assert "clip_panels" in msg
        return msg

    assert "null" in call(out=None) and "null" in call(clips=None) and "null" in call(pad=None)
    assert "clip 1 is a null" in call(clips=(ctypes.c_void_p * K)(4096, None))
    assert "K 0" in call(K=0) and "K 5" in call(K=5)
    assert "C 2" in call(C=2) and "C 4" in call(C=4)
    assert ">= 1" in call(N=0) and ">= 1" in call(H=0) and ">= 1" in call(W=-3)
    assert "T 0" in call(T=(ctypes.c_int32 * K)(3, 0))
    assert "pad 3" in call(pad=(ctypes.c_int32 * K)(3, -1)) and "pad -2" in call(pad=(ctypes.c_int32 * K)(1, -2))
    assert "negative stride" in call(sn=(ctypes.c_int64 * K)(64, -64)) and "negative stride" in call(st=(ctypes.c_int64 * K)(-1, 16))
    assert "together" in call(a=ctypes.c_void_p(4096))
    assert "layout 2" in call(layout=2)
    assert "workgroups" in call(N=2 ** 31 - 1, H=64, W=64)
    assert "quads" in call(H=2 ** 20, W=2 ** 20)


def test_op_guards_without_a_device():
    import vptr_amd.ops as ops
    from vptr_amd.visualize import clips_to_uint8
    x = torch.zeros((1, 2, 1, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.clip_panels([x])
    with pytest.raises(RuntimeError, match="MI355X only"):
        clips_to_uint8([x], renorm=None)
    with pytest.raises(RuntimeError, match="between 1 and 4"):
        ops.clip_panels([])
    with pytest.raises(RuntimeError, match="between 1 and 4"):
        ops.clip_panels([x] * 5)
    for kw in (dict(quantize="round"), dict(layout="grid"), dict(pad="edge")):
        with pytest.raises(ValueError, match="must be one of"):
            ops.clip_panels([x], **kw)
