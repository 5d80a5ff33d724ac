"""Clip ingest, host side: the coefficient tables of vptr_amd.data and the tests' reference builder against PIL itself and against the
PIL-written fixture (uint8 images equal), the crop rule, the normalisation table, the presets, ClipIngest's flag drawing, and the
presence of the feature (C-ABI entry point, op, module)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import jload, load
from vptr_amd.data import resize_tables          # the module under test: without it nothing in this file can pass
from ingest_ref import GOLDEN_GEOMETRIES, KINDS, PIL_GEOMETRIES, make_raw, normalise_u8, ref_ingest, ref_resize_u8, ref_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data_resize_u8(raw, crop, out_hw):
    """crop + the two integer passes driven by vptr_amd.data.resize_tables, tap by tap as the kernel runs them (plain loops over the
    table entries, vectorised over everything else)"""
    def one_pass(a, out_size):                               # along the last axis
        k, b = resize_tables(a.shape[-1], out_size)
        assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape[0] == out_size and b.shape == (out_size, 2)
        res = np.empty(a.shape[:-1] + (out_size,), dtype=np.uint8)
        a64 = a.astype(np.int64)
        for xo in range(out_size):
            ss = np.full(a.shape[:-1], 1 << 21, dtype=np.int64)
            for j in range(int(b[xo, 1])):
                ss += a64[..., int(b[xo, 0]) + j] * int(k[xo, j])
            assert int(np.abs(ss).max()) < 2 ** 31                # the kernel's int32 accumulator
            res[..., xo] = np.clip(ss >> 22, 0, 255)
        return res

    if crop is not None:
        top, left, th, tw = crop
        raw = raw[:, :, top:top + th, left:left + tw, :]
    a = raw
    if out_hw[1] != a.shape[3]:
        a = np.moveaxis(one_pass(np.moveaxis(a, 3, -1), out_hw[1]), -1, 3)
    if out_hw[0] != a.shape[2]:
        a = np.moveaxis(one_pass(np.moveaxis(a, 2, -1), out_hw[0]), -1, 2)
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("geom", PIL_GEOMETRIES, ids=lambda g: "%dx%dx%d-%dx%d" % (g[0], g[1], g[2], g[4][0], g[4][1]))
def test_tables_and_builder_match_pil(geom):
    """Image.resize(..., BILINEAR) on random, binary 0 / 255 and ramp images: every uint8 value equal, for the tables of vptr_amd.data
    and for the tests' own builder"""
    Image = pytest.importorskip("PIL.Image")
    Hin, Win, C, crop, out_hw = geom
    for i, kind in enumerate(KINDS):
        raw = make_raw((1, 1, Hin, Win, C), kind, 5000 + 10 * PIL_GEOMETRIES.index(geom) + i)
        f = raw[0, 0]
        img = Image.fromarray(f[:, :, 0], "L") if C == 1 else Image.fromarray(f, "RGB")
        if (Hin, Win) != tuple(out_hw):
            img = img.resize((out_hw[1], out_hw[0]), Image.BILINEAR)
        want = np.asarray(img).reshape(out_hw[0], out_hw[1], C)
        assert np.array_equal(data_resize_u8(raw, crop, out_hw)[0, 0], want), (geom, kind, "vptr_amd.data tables")
        assert np.array_equal(ref_resize_u8(raw, crop, out_hw)[0, 0], want), (geom, kind, "reference builder")


@pytest.mark.parametrize("tag", sorted(GOLDEN_GEOMETRIES))
def test_tables_and_builder_match_pil_fixture(tag):
    """the same check against images PIL wrote into tests/golden/ingest_pil.npz (tools/make_ingest_golden.py), crop included"""
    z = load("ingest_pil")
    meta = jload(z, "meta")[tag]
    Hin, Win, C, crop, out_hw = GOLDEN_GEOMETRIES[tag]
    assert (meta["crop"] is None and crop is None or tuple(meta["crop"]) == crop) and tuple(meta["out"]) == out_hw
    raw, want = z["raw:" + meta["raw"]], z["pil:" + tag]
    assert raw.shape == (1, 3, Hin, Win, C) and raw.dtype == np.uint8 and want.shape == (1, 3) + out_hw + (C,)
    assert np.array_equal(data_resize_u8(raw, crop, out_hw), want)
    assert np.array_equal(ref_resize_u8(raw, crop, out_hw), want)


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ingest_pil.npz")) < 200 * 1000


@pytest.mark.parametrize("sizes", [(120, 64), (120, 128), (160, 64), (41, 24), (9, 20), (300, 64), (240, 64), (300, 256), (64, 8), (7, 7)])
def test_resize_tables_shape_and_sum(sizes):
    n_in, n_out = sizes
    k, b = resize_tables(n_in, n_out)
    k2, first, count = ref_tables(n_in, n_out)
    assert k.shape[1] == int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    assert np.array_equal(k, k2) and np.array_equal(b[:, 0], first) and np.array_equal(b[:, 1], count)
    assert int(b[:, 0].min()) >= 0 and int((b[:, 0] + b[:, 1]).max()) <= n_in and int(b[:, 1].min()) >= 1
    assert int(np.abs(k.sum(axis=1) - (1 << 22)).max()) <= k.shape[1]          # each weight is rounded once
    for xo in range(n_out):
        assert not k[xo, b[xo, 1]:].any()


def test_center_crop_box():
    from vptr_amd.data import center_crop_box
    assert center_crop_box(120, 160, 120, 120) == (0, 20, 120, 120)
    assert center_crop_box(240, 240, 120, 120) == (60, 60, 120, 120)
    assert center_crop_box(37, 53, 31, 41) == (3, 6, 31, 41)
    assert center_crop_box(10, 11, 7, 8) == (2, 2, 7, 8)          # round(1.5) = 2: Python rounds half to even
    assert center_crop_box(10, 11, 5, 6) == (2, 2, 5, 6)          # round(2.5) = 2
    assert center_crop_box(9, 9, 9, 9) == (0, 0, 9, 9)
    for bad in [(10, 10, 11, 5), (10, 10, 5, 11), (10, 10, 0, 5)]:
        with pytest.raises(ValueError):
            center_crop_box(*bad)


@pytest.mark.parametrize("mean,std,C", [(0.0, 1.0, 1), (0.6013795, 2.7570653, 1), (0.5, 0.25, 3),
                                        ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673), 3)])
def test_normalize_lut(mean, std, C):
    """all 256 values against the op chain of ToTensor + Normalize on an image that holds every value"""
    from vptr_amd.data import normalize_lut
    lut = normalize_lut(mean, std, C)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (C, 256)
    img = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16, 1), C, axis=4)
    want = normalise_u8(img, mean, std)[0, 0].reshape(C, 256)
    assert torch.equal(lut, want)
    m = [mean] * C if isinstance(mean, float) else list(mean)
    s = [std] * C if isinstance(std, float) else list(std)
    for c in range(C):       # Normalize's own form: fp32 tensors of the constants
        x = torch.arange(256, dtype=torch.float32).div(255)
        assert torch.equal(lut[c], x.sub(torch.tensor(m[c], dtype=torch.float32)).div(torch.tensor(s[c], dtype=torch.float32)))
    with pytest.raises(ValueError):
        normalize_lut((0.1, 0.2), 1.0, 3)


def test_presets():
    from vptr_amd.data import IngestPlan
    for size in (64, 128):
        p = IngestPlan.kth(size, device="cpu")
        assert p.in_hw == (120, 160) and p.channels == 1 and p.crop == (0, 20, 120, 120) and p.out_hw == (size, size)
        assert (p.mean, p.std) == (0.6013795, 2.7570653)
        assert p.ksx == p.ksy == (5 if size == 64 else 3) and tuple(p.kx.shape) == (size, p.ksx) and tuple(p.by.shape) == (size, 2)
        assert p.kx.dtype == torch.int32 and torch.equal(p.kx, p.ky)
    b = IngestPlan.bair(device="cpu")
    assert b.in_hw == b.out_hw == (64, 64) and b.channels == 3 and b.crop == (0, 0, 64, 64) and b.kx is None and b.ky is None
    assert b.mean == (0.61749697, 0.6050092, 0.52180636) and b.std == (2.1824553, 2.1553133, 1.9115673)
    assert tuple(b.lut.shape) == (3, 256)
    m = IngestPlan.mnist(device="cpu")
    assert m.in_hw == m.out_hw == (64, 64) and m.channels == 1 and m.kx is None and (m.mean, m.std) == (0.0, 1.0)
    assert torch.equal(m.lut[0], torch.arange(256, dtype=torch.float32).div(255))
    one_axis = IngestPlan((120, 64), 1, (64, 64), device="cpu")
    assert one_axis.kx is None and one_axis.ksx == 0 and one_axis.ksy == 5
    for bad in [dict(in_hw=(8, 8), channels=2, out_hw=(8, 8)), dict(in_hw=(8, 8), channels=1, out_hw=(8, 8), crop=(9, 8)),
                dict(in_hw=(8, 8), channels=1, out_hw=(8, 8), crop=(1, 1, 8, 8))]:
        with pytest.raises(ValueError):
            IngestPlan(device="cpu", **bad)


def test_clip_ingest_flag_drawing(monkeypatch):
    """same seed -> same flags; p = 0 and p = 1; explicit flags pass through; the op is replaced by a recorder"""
    import vptr_amd.ops as ops
    from vptr_amd.data import ClipIngest, IngestPlan
    calls = []

    def fake(raw, plan, flips=None, split=None, out=None):
        calls.append((tuple(raw.shape), None if flips is None else flips.clone(), split, out))
        return "past", "future"

    monkeypatch.setattr(ops, "ingest_clips", fake)
    plan = IngestPlan.mnist(device="cpu")
    raw = np.zeros((6, 5, 64, 64, 1), dtype=np.uint8)
    a, b = ClipIngest(plan, 2, 3, 0.5, 0.5, seed=11), ClipIngest(plan, 2, 3, 0.5, 0.5, seed=11)
    seen = []
    for _ in range(4):
        assert a(raw) == ("past", "future")
        b(torch.from_numpy(raw))
        assert np.array_equal(a.last_flips, b.last_flips) and a.last_flips.dtype == np.int32 and a.last_flips.shape == (6,)
        assert torch.equal(calls[-1][1], torch.from_numpy(b.last_flips)) and calls[-1][1].dtype == torch.int32
        assert calls[-1][0] == (6, 5, 64, 64, 1) and calls[-1][2] == (2, 3)
        seen.extend(a.last_flips.tolist())
    assert set(seen) <= {0, 1, 2, 3} and len(set(seen)) > 1                      # 24 draws at p = 0.5
    assert not np.array_equal(ClipIngest(plan, 2, 3, 0.5, 0.5, seed=12).draw_flips(64), ClipIngest(plan, 2, 3, 0.5, 0.5, seed=11).draw_flips(64))
    none = ClipIngest(plan, 2, 3, seed=1)
    none(raw)
    assert calls[-1][1] is None and np.array_equal(none.last_flips, np.zeros(6, dtype=np.int32))
    assert np.array_equal(ClipIngest(plan, 2, 3, 1.0, 1.0, seed=1).draw_flips(9), np.full(9, 3, dtype=np.int32))
    assert np.array_equal(ClipIngest(plan, 2, 3, 1.0, 0.0, seed=1).draw_flips(9), np.full(9, 1, dtype=np.int32))
    assert np.array_equal(ClipIngest(plan, 2, 3, 0.0, 1.0, seed=1).draw_flips(9), np.full(9, 2, dtype=np.int32))
    given = [3, 0, 1, 2, 0, 1]
    out = (object(), object())
    a(raw, flips=given, out=out)
    assert calls[-1][1].tolist() == given and a.last_flips.tolist() == given and calls[-1][3] is out
    a(raw, flips=torch.tensor(given, dtype=torch.int32))
    assert calls[-1][1].tolist() == given
    with pytest.raises(RuntimeError, match=r"\(N, 5, H, W, C\)"):
        a(raw[:, :4])
    with pytest.raises(ValueError):
        ClipIngest(plan, 2, 3, hflip_p=1.5)


def test_reference_builder_flips_and_layout():
    """the builder's own conventions on an image where they can be read off: HWC -> CHW, flips after the resize, per clip"""
    raw = make_raw((2, 2, 6, 8, 3), "random", 5300)
    plain = ref_ingest(raw, None, (6, 8))
    assert tuple(plain.shape) == (2, 2, 3, 6, 8)
    assert torch.equal(plain, torch.from_numpy(raw).permute(0, 1, 4, 2, 3).float().div(255))
    fl = ref_ingest(raw, None, (6, 8), flips=[1, 2])
    assert torch.equal(fl[0], plain[0].flip(-1)) and torch.equal(fl[1], plain[1].flip(-2))
    both = ref_ingest(raw, (1, 2, 4, 5), (3, 7), 0.5, 2.0, flips=[3, 0])
    assert torch.equal(both[0], ref_ingest(raw, (1, 2, 4, 5), (3, 7), 0.5, 2.0)[0].flip(-1).flip(-2))


def test_feature_is_present():
    from vptr_amd import _lib
    from vptr_amd.build import SOURCES
    assert "ingest.hip" in SOURCES
    assert "vptr_clip_ingest" in _lib.SIGNATURES and "vptr_clip_ingest" in _lib.EXPORTS
    assert len(_lib.SIGNATURES["vptr_clip_ingest"]) == 24
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vptr_clip_ingest")
    with open(os.path.join(ROOT, "include", "vptr_hip.h")) as f:
        assert re.search(r"\bint\s+vptr_clip_ingest\s*\(", f.read())
    assert _lib.lib.vptr_abi_version() == 10
    import vptr_amd.data as D
    import vptr_amd.ops as ops
    assert callable(ops.ingest_clips) and callable(D.ClipIngest) and callable(D.DeviceClipLoader) and callable(D.IngestPlan.kth)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ingest_clips(torch.zeros((1, 2, 64, 64, 1), dtype=torch.uint8), D.IngestPlan.mnist(device="cpu"))
