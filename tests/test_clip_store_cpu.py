"""CPU side of the HBM-resident clip store: the ABI table of include/vptr_hip_data.h, the host-side rejects of its two entry points, the
integer emulation of tests/clip_store_cases.py (bijection, epochs, rank partition, wrap, flips), the emulated gather on every GPU case,
seven named mutations of the emulation, each of which must fail the cases listed for it, and the host rules of vptr_amd.data: the two
store builders against a literal restatement of the reference's slicing, and every ValueError."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clip_store_cases as K
from ingest_ref import ref_ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vptr_clip_draw", "vptr_clip_ingest_gather"}


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_data_signatures_match_header_and_library():
    from vptr_amd import _lib, data
    text = open(os.path.join(ROOT, "include", "vptr_hip_data.h")).read()
    assert '#include "vptr_hip.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(decls) == set(_lib.DATA_SIGNATURES) == NAMES
    kind = {"int": _lib.c_int, "float": _lib.c_float}
    for name, args in decls.items():
        kinds = [_lib.c_void_p if "*" in a or "vptr_stream_t" in a else kind[a.split()[0]] for a in args.split(",")]
        assert kinds == _lib.DATA_SIGNATURES[name], name                                    # the stream included
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == _lib.DATA_SIGNATURES[name] and fn.restype is _lib.c_int
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES), set(_lib.ACCUM_SIGNATURES),
              set(_lib.LOSS_SIGNATURES), set(_lib.GAN_SIGNATURES), set(_lib.GROUP_SIGNATURES)]
    assert all(not NAMES & o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    from vptr_amd.build import SOURCES
    assert "clipstore.hip" in SOURCES and "ingest.hip" in SOURCES
    # the record layouts: header, host layer and the cases agree
    for prefix, table in (("CUR", K.CUR), ("SEL", K.SEL), ("DRAW", K.DRAW)):
        defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_%s_(\w+) (\d+)" % prefix, text)}
        assert defs == table, (prefix, defs)
    assert (data.CUR_SEED_LO, data.CUR_SEED_HI, data.CUR_EPOCH, data.CUR_BATCH, data.CUR_BPE, data.CUR_DRAWN_LO, data.CUR_DRAWN_HI,
            data.CUR_WORDS) == tuple(K.CUR[k] for k in ("SEED_LO", "SEED_HI", "EPOCH", "BATCH", "BPE", "DRAWN_LO", "DRAWN_HI", "WORDS"))
    assert (data.SEL_PAST, data.SEL_FUTURE, data.SEL_FLIPS, data.SEL_CLIP, data.SEL_WORDS) == tuple(
        K.SEL[k] for k in ("PAST", "FUTURE", "FLIPS", "CLIP", "WORDS"))
    from vptr_amd import ops
    assert ops.CURSOR_WORDS == K.CUR["WORDS"] and ops.SEL_WORDS == K.SEL["WORDS"]
    # one kernel body: both translation units take it from the shared header, neither holds the passes itself
    csrc = os.path.join(ROOT, "vptr_amd", "csrc")
    for src in ("ingest.hip", "clipstore.hip"):
        t = open(os.path.join(csrc, src)).read()
        assert '#include "ingest_body.h"' in t and "ig_kernel_body(" in t and "ig_clip8" not in t, src
    assert "ig_clip8" in open(os.path.join(csrc, "ingest_body.h")).read()


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_int32 * 4096)()
    base = (ctypes.addressof(buf) + 63) & ~63
    cursor, table, sel = base, base + 64, base + 1024

    def bad(fn, word, *args):
        assert fn(*args, None) != 0, (word, args)
        msg = L.vptr_last_error().decode()
        assert word in msg, (word, msg)

    good = dict(cursor=cursor, table=table, sel=sel, n=17, N=4, rank=0, world=1, shuffle=1, hp=0.5, vp=0.5)
    for change, word in ((dict(cursor=None), "null"), (dict(table=None), "null"), (dict(sel=None), "null"), (dict(cursor=cursor + 4), "aligned"),
                         (dict(sel=sel + 4), "aligned"), (dict(table=table + 4), "aligned"), (dict(n=0), "n_clips 0"), (dict(N=0), "N 0"), (dict(world=0), "world 0"),
                         (dict(rank=-1), "rank -1"), (dict(rank=1), "rank 1"), (dict(rank=2, world=2), "rank 2"), (dict(N=18), "batches_per_epoch"),
                         (dict(N=9, world=2, rank=1), "batches_per_epoch"), (dict(hp=-0.01), "[0, 1]"), (dict(vp=1.01), "[0, 1]"),
                         (dict(hp=float("nan")), "[0, 1]")):
        a = dict(good, **change)
        bad(L.vptr_clip_draw, word, a["cursor"], a["table"], a["sel"], a["n"], a["N"], a["rank"], a["world"], a["shuffle"], a["hp"], a["vp"])
        assert L.vptr_last_error().decode().startswith("clip_draw:")
    assert all(v == 0 for v in buf)

    g = dict(store=base, n_frames=9, sel=sel, kx=table, bx=table, ky=table, by=table, lut=table, out0=base + 2048, out1=base + 4096, N=1, T=3,
             Tp=2, Hin=20, Win=40, C=1, top=2, left=4, Hc=16, Wc=32, Hout=8, Wout=16, ksx=5, ksy=5)
    order = ("store", "n_frames", "sel", "kx", "bx", "ky", "by", "lut", "out0", "out1", "N", "T", "Tp", "Hin", "Win", "C", "top", "left", "Hc",
             "Wc", "Hout", "Wout", "ksx", "ksy")
    for change, word in ((dict(store=None), "null"), (dict(sel=None), "null"), (dict(lut=None), "null"), (dict(n_frames=0), "n_frames 0"),
                         (dict(n_frames=-5), "n_frames -5"), (dict(C=2), "C 2"), (dict(N=0), "N 0"), (dict(T=0), "T 0"), (dict(Wout=257), "256"),
                         (dict(Hout=0), "256"), (dict(left=30), "crop box"), (dict(top=-1), "crop box"), (dict(Hc=0), "crop box"),
                         (dict(ksx=19), "8x"), (dict(ksy=19), "8x"), (dict(Tp=4), "Tp"), (dict(Tp=-1), "Tp"), (dict(out1=None), "out1"),
                         (dict(out0=None), "null output"), (dict(kx=None), "horizontal"), (dict(by=None), "vertical"),
                         (dict(N=1 << 20, T=1 << 10, Tp=2, Hin=64, Win=64, left=0, top=0, Hc=64, Wc=64, Hout=8, Wout=16), "too large"),
                         (dict(N=1 << 20, T=1 << 12, Hin=1, Win=1, top=0, left=0, Hc=1, Wc=1, Hout=1, Wout=1), "workgroups of one launch")):
        a = dict(g, **change)
        bad(L.vptr_clip_ingest_gather, word, *[a[k] for k in order])
        assert L.vptr_last_error().decode().startswith("clip_ingest_gather:")
    assert all(v == 0 for v in buf)


# ---- perm and the draw --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17, 255, 257, 4097, 65537])
def test_perm_is_a_bijection_and_epochs_differ(n):
    i = torch.arange(n)
    walks = []
    p0 = K.perm_emu(i, n, K.SEED0, 0, count=walks)
    p1 = K.perm_emu(i, n, K.SEED0, 1)
    for p in (p0, p1, K.perm_emu(i, n, K.SEEDS["high"], 0)):
        assert int(p.min()) == 0 and int(p.max()) == n - 1 and torch.equal(torch.sort(p).values, i)
    assert 1 << K.perm_bits(n) >= n and (n < 2 or 1 << K.perm_bits(n) < 4 * n) and K.perm_bits(n) % 2 == 0
    assert float(walks[0].double().mean()) <= 4.0
    if n >= 16:
        assert not torch.equal(p0, p1) and not torch.equal(p0, i)
        # the per-position evaluation is the whole-epoch one: any subset of positions gives the same clips
        sub = torch.tensor([n - 1, 0, n // 2])
        assert torch.equal(K.perm_emu(sub, n, K.SEED0, 0), p0[sub])


def _drive(c, calls, cursor=None, hp=K.SWEEP_FLIPS[0], vp=K.SWEEP_FLIPS[1], mut=None, seed=K.SEED0):
    cursor = K.cursor0(seed) if cursor is None else cursor
    return K.drive_emu(cursor, K.clip_table_for(c["n"]), c["N"], c["rank"], c["world"], c["shuffle"], hp, vp, calls, mut)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,N", [(17, 3), (257, 16), (4097, 300), (5, 1)])
def test_ranks_partition_the_epoch(n, N, world):
    bpe = n // (N * world)
    assert bpe >= 1
    for shuffle in (1, 0):
        for epoch in (0, 3):
            clips = []
            for rank in range(world):
                sel, _ = _drive(dict(n=n, N=N, rank=rank, world=world, shuffle=shuffle), bpe, cursor=K.cursor0(K.SEED0, epoch=epoch))
                clips.append(sel[..., K.SEL["CLIP"]].long())
            allc = torch.stack(clips, dim=1).reshape(-1)                    # [batch][rank][j]: the epoch's order
            assert allc.numel() == bpe * N * world and allc.unique().numel() == allc.numel()
            want = torch.arange(bpe * N * world)
            want = K.perm_emu(want, n, K.SEED0, epoch) if shuffle else want
            assert torch.equal(allc, want)


def test_wrap_at_exactly_batches_per_epoch():
    c = dict(n=17, N=3, rank=0, world=1, shuffle=1)                          # bpe 5
    sel, cur = _drive(c, 11, cursor=K.cursor0(K.SEED0, epoch=7, drawn=(1 << 32) - 3))
    assert cur[:, K.CUR["BATCH"]].tolist() == [1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert cur[:, K.CUR["EPOCH"]].tolist() == [7, 7, 7, 7, 8, 8, 8, 8, 8, 9, 9]
    assert cur[:, K.CUR["BPE"]].tolist() == [5] * 11
    drawn = [(int(lo) & K.M32) | ((int(hi) & K.M32) << 32) for lo, hi in cur[:, K.CUR["DRAWN_LO"]:K.CUR["DRAWN_HI"] + 1].tolist()]
    assert drawn == [(1 << 32) - 2 + k for k in range(11)]                   # the carry into the high word
    assert torch.equal(cur[:, 7:], torch.tensor([K.RESERVED + k for k in range(7, 16)], dtype=torch.int32).expand(11, 9))
    assert not torch.equal(sel[0], sel[5]) and sel[..., 3].max() < 17        # batch 0 of two epochs
    # a batch word past the epoch is reduced modulo bpe; the record stays as the device would leave it
    a, _ = _drive(c, 1, cursor=K.cursor0(K.SEED0, batch=13))
    b, _ = _drive(c, 1, cursor=K.cursor0(K.SEED0, batch=3))
    assert torch.equal(a, b)
    # the seed's words are both read
    sels = {k: _drive(c, 2, seed=s)[0] for k, s in K.SEEDS.items()}
    assert all(not torch.equal(sels[a], sels[b]) for a in sels for b in sels if a < b)


def test_flips_follow_the_clip_not_the_position():
    n, N = 257, 16
    per_world = {}
    for world in (1, 2):
        bpe = n // (N * world)
        seen = {}
        for rank in range(world):
            sel, _ = _drive(dict(n=n, N=N, rank=rank, world=world, shuffle=1), bpe, hp=0.5, vp=0.5)
            for clip, fl in zip(sel[..., 3].reshape(-1).tolist(), sel[..., 2].reshape(-1).tolist()):
                assert seen.setdefault(clip, fl) == fl
        per_world[world] = seen
    common = set(per_world[1]) & set(per_world[2])
    assert len(common) >= 200 and all(per_world[1][c] == per_world[2][c] for c in common)
    assert len({per_world[1][c] for c in common}) == 4


@pytest.mark.parametrize("p", [0.0, 1.0, 0.5, 0.25, 0.9])
def test_flip_shares(p):
    n = 100000
    clips = torch.arange(n)
    fl = K.flips_emu(clips, K.SEED0, 2, p, 1.0 - p)
    h, v = int((fl & 1).sum()), int((fl >> 1).sum())
    if p in (0.0, 1.0):
        assert h == int(p * n) and v == int((1.0 - p) * n)                   # exact
    else:
        sigma = (n * p * (1.0 - p)) ** 0.5
        assert abs(h - n * p) <= 3 * sigma and abs(v - n * (1.0 - p)) <= 3 * sigma, (h, v, sigma)
        both, q = int((fl == 3).sum()), p * (1.0 - p)                        # the two sites are independent
        assert abs(both - n * q) <= 4 * (n * q * (1.0 - q)) ** 0.5


def test_sweep_cases_are_consistent():
    """every case of the GPU sweep, driven for two epochs and one call more: clip ids inside the list, rows copied from the table, each
    epoch of a rank without repetition"""
    cases = K.draw_sweep()
    assert len(cases) >= 60 and {c["n"] for c in cases} == {1, 5, 17, 257, 4097} and {c["N"] for c in cases} == {1, 3, 16, 300}
    for c in cases:
        calls = K.draw_calls(c)
        bpe = c["n"] // (c["N"] * c["world"])
        sel, cur = _drive(c, calls)
        table = K.clip_table_for(c["n"])
        clip = sel[..., 3].long()
        assert int(clip.min()) >= 0 and int(clip.max()) < c["n"]
        assert torch.equal(sel[..., :2], table[clip]) and int(sel[..., 2].min()) >= 0 and int(sel[..., 2].max()) <= 3
        for e in range(2):
            ids = clip[e * bpe:(e + 1) * bpe].reshape(-1)
            assert ids.unique().numel() == ids.numel()
        assert cur[-1, K.CUR["EPOCH"]] == calls // bpe and cur[-1, K.CUR["BATCH"]] == calls % bpe and cur[-1, K.CUR["DRAWN_LO"]] == calls


# ---- the gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.GATHER_CASES))
def test_gather_cases_are_consistent(name):
    Hin, Win, C, crop, out_hw, F, Tp, Tf, rows = K.GATHER_CASES[name]
    store, sel = K.gather_store(name), K.gather_sel(name)
    assert store.shape == (F, Hin, Win, C)
    f = K.gather_index(sel, Tp, Tf, F, mut="no_clamp")
    assert int(f.min()) >= 0 and int(f.max()) <= F - 1                       # what the GPU is handed stays inside the store
    ref = K.gather_ref(name)
    assert tuple(ref.shape) == (len(rows), Tp + Tf, C, out_hw[0], out_hw[1])
    # the literal gather: clip by clip, frame by frame
    for n, (p, fu, fl) in enumerate(rows):
        raw = np.concatenate([store[p:p + Tp], store[fu:fu + Tf]], axis=0)[None]
        assert torch.equal(ref[n:n + 1], ref_ingest(raw, crop, out_hw, *K.consts(C), flips=[fl]))


def test_gather_cases_cover_what_the_issue_lists():
    rows = K.GATHER_CASES["kth64"][8]
    Tp, Tf, F = K.GATHER_CASES["kth64"][6], K.GATHER_CASES["kth64"][7], K.GATHER_CASES["kth64"][5]
    assert {r[2] for r in rows} == {0, 1, 2, 3}                              # all four flip combinations in one batch
    assert any(r[1] != r[0] + Tp for r in rows)                              # independent past / future starts
    assert len({r[:2] for r in rows}) < len(rows)                            # the same clip twice
    assert any(a != b and abs(a[0] - b[0]) < Tp + Tf for a in rows for b in rows)   # overlapping clips
    assert any(r[1] + Tf == F for r in rows)                                 # a clip ending on the store's last frame
    assert K.GATHER_CASES["Tp0"][6] == 0 and K.GATHER_CASES["TpT"][7] == 0
    assert K.GATHER_CASES["odd"][4][1] % 4 != 0 and K.GATHER_CASES["upscale"][4][0] > K.GATHER_CASES["upscale"][0]


def test_frame_clamp():
    Hin, Win, C, crop, out_hw, F, Tp, Tf, rows = K.CLAMP_CASE
    store = K.gather_store("clamp")
    f = K.gather_index(K.gather_sel("clamp"), Tp, Tf, F)
    assert f.tolist() == [[7, 7, 7, 7], [0, 0, 6, 7], [7, 7, 0, 0]]
    ref = K.gather_ref("clamp")
    assert torch.equal(ref[0, 1], ref[0, 0]) and torch.equal(ref[0, 3], ref[0, 0])
    want = ref_ingest(store[[7, 7, 0, 0]][None], crop, out_hw, *K.consts(C), flips=[2])
    assert torch.equal(ref[2:3], want)


# ---- mutations ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", K.MUTATIONS)
def test_mutations_fail_their_cases(mut):
    assert K.MUTATION_CASES[mut]
    for what in K.MUTATION_CASES[mut]:
        if what[0] == "draw":
            _, c, calls = what
            good, bad = _drive(c, calls), _drive(c, calls, mut=mut)
            assert not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])), (mut, what)
        elif what[0] == "perm":
            i = torch.arange(what[1])
            bad = K.perm_emu(i, what[1], K.SEED0, 0, mut=mut)
            assert not torch.equal(K.perm_emu(i, what[1], K.SEED0, 0), bad) and int(bad.max()) >= what[1], (mut, what)
        elif mut == "no_clamp":
            with pytest.raises(IndexError):
                K.gather_ref(what[1], mut=mut)
        else:
            assert not torch.equal(K.gather_ref(what[1]), K.gather_ref(what[1], mut=mut)), (mut, what)
    # every mutation leaves the cases it is not listed for runnable: the emulation itself has no other branch on `mut`
    assert set(K.MUTATION_CASES) == set(K.MUTATIONS)


# ---- the host layer -------------------------------------------------------------------------------------------------------------------
def _video(n, seed, hw=(6, 5), C=1):
    return np.random.RandomState(seed).randint(0, 256, size=(n,) + hw + (C,)).astype(np.uint8)


def test_from_videos_follows_the_reference_slicing():
    from vptr_amd.data import DeviceClipStore
    Tp, Tf = 12, 8
    L = Tp + Tf
    videos = [_video(n, 40 + k) for k, n in enumerate((19, 20, 21, 41, 3))]
    want = []                                                                # utils/dataset.py __getClips__, on frames instead of files
    for img_files in videos:
        clip_num = len(img_files) // L
        rem_num = len(img_files) % L
        img_files = img_files[rem_num // 2: rem_num // 2 + clip_num * L]
        for i in range(clip_num):
            want.append(img_files[i * L: (i + 1) * L])
    assert len(want) == 4                                                    # 0 + 1 + 1 + 2 + 0
    store = DeviceClipStore.from_videos(videos, Tp, Tf, device="cpu")
    assert store.n_clips == 4 and store.n_frames == 80 and store.frame_shape == (6, 5, 1) and (store.num_past, store.num_future) == (Tp, Tf)
    assert store.frames.dtype == torch.uint8 and store.clip_table.dtype == torch.int32 and tuple(store.clip_table.shape) == (4, 2)
    frames = store.frames.numpy()
    for (p, f), clip in zip(store.clip_table.tolist(), want):
        assert f == p + Tp
        assert np.array_equal(frames[p:p + Tp], clip[:Tp]) and np.array_equal(frames[f:f + Tf], clip[Tp:])
    assert np.array_equal(frames[20:40], videos[2][0:20]) and np.array_equal(frames[40:80], videos[3][0:40])   # rem 1 -> offset 0
    with pytest.raises(ValueError, match="no video"):
        DeviceClipStore.from_videos([_video(3, 1)], Tp, Tf, device="cpu")
    with pytest.raises(ValueError, match="frame shape"):
        DeviceClipStore.from_videos([_video(20, 1), _video(20, 2, hw=(6, 6))], Tp, Tf, device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        DeviceClipStore.from_videos([_video(20, 1).astype(np.float32)], Tp, Tf, device="cpu")
    # a remainder of 5 frames: 2 dropped in front
    v = _video(25, 77)
    s = DeviceClipStore.from_videos([v], Tp, Tf, device="cpu")
    assert np.array_equal(s.frames.numpy(), v[2:22])


def test_from_moving_mnist_follows_the_reference_getitem():
    from vptr_amd.data import DeviceClipStore
    raw = np.random.RandomState(5).randint(0, 256, size=(40, 1, 8, 8)).astype(np.uint8)
    clips = np.zeros((2, 3, 2), dtype=np.int32)
    clips[0, :, 0], clips[0, :, 1] = (0, 25, 7), 4                          # past: start, length
    clips[1, :, 0], clips[1, :, 1] = (4, 3, 37), 3                          # future: an independent start
    data = {"clips": clips, "input_raw_data": raw, "dims": np.array([[1, 8, 8]])}
    store = DeviceClipStore.from_moving_mnist(data, device="cpu")
    assert (store.num_past, store.num_future) == (4, 3) and store.n_clips == 3 and store.frame_shape == (8, 8, 1)
    for index in range(3):                                                   # MovingMNISTDataset.__getitem__
        clip_index = data["clips"][:, index, :]
        psi, pei = clip_index[0, 0], clip_index[0, 0] + clip_index[0, 1]
        past_clip = data["input_raw_data"][psi:pei, ...]
        fsi, fei = clip_index[1, 0], clip_index[1, 0] + clip_index[1, 1]
        future_clip = data["input_raw_data"][fsi:fei, ...]
        p, f = store.clip_table[index].tolist()
        assert np.array_equal(store.frames[p:p + 4].numpy()[..., 0], past_clip[:, 0])
        assert np.array_equal(store.frames[f:f + 3].numpy()[..., 0], future_clip[:, 0])
    bad = dict(data, clips=clips.copy())
    bad["clips"][1, 2, 0] = 38                                               # 38 + 3 > 40
    with pytest.raises(ValueError, match="leave"):
        DeviceClipStore.from_moving_mnist(bad, device="cpu")
    bad["clips"][1, 2] = (30, 2)
    with pytest.raises(ValueError, match="lengths"):
        DeviceClipStore.from_moving_mnist(bad, device="cpu")
    with pytest.raises(ValueError, match="clips must be"):
        DeviceClipStore.from_moving_mnist(dict(data, clips=clips[0]), device="cpu")


def test_store_and_loader_value_errors():
    from vptr_amd.data import DeviceClipStore, IngestPlan, StoreLoader
    frames = _video(30, 9, hw=(12, 10))
    clips = np.array([[0, 3], [5, 8], [10, 13], [20, 23], [24, 27]])
    store = DeviceClipStore(frames, clips, device="cpu")
    assert store.n_clips == 5 and store.nbytes() == 30 * 120 and torch.equal(store.frames, torch.from_numpy(frames))
    listed = DeviceClipStore([frames[:11], frames[11:]], clips, device="cpu")        # per-video arrays, one after the other
    assert torch.equal(listed.frames, store.frames)
    plan = IngestPlan((12, 10), 1, (6, 5), device="cpu")
    ok = StoreLoader(store, plan, 2, 3, 3)
    assert len(ok) == 2 and ok.batches_per_epoch == 2 and tuple(ok.last_selection().shape) == (2, 4)
    assert len(StoreLoader(store, plan, 2, 3, 3, shuffle=False, drop_last=False)) == 3 and len(StoreLoader(store, plan, 2, 3, 3, world=2, rank=1)) == 1
    cur = ok.cursor.tolist()
    assert cur[K.CUR["BPE"]] == 2 and cur[K.CUR["EPOCH"]] == 0 and cur[K.CUR["BATCH"]] == 0
    big = StoreLoader(store, plan, 1, 3, 3, seed=K.SEED0)
    assert big.cursor.tolist()[:2] == [K.s32(K.SEED0), K.s32(K.SEED0 >> 32)] == K.cursor0(K.SEED0)[:2]
    for kw, word in ((dict(N=6), "fewer"), (dict(N=3, world=2), "fewer"), (dict(num_future=4), "leave the store"), (dict(num_past=28), "leave the store"),
                     (dict(hflip_p=1.5), "flip"), (dict(vflip_p=-0.1), "flip"), (dict(hflip_p=float("nan")), "flip"), (dict(rank=1), "rank"),
                     (dict(N=0), "N 0"), (dict(shuffle=True, drop_last=False), "sequential"), (dict(seed=-1), "seed")):
        a = dict(dict(N=2, num_past=3, num_future=3), **kw)
        with pytest.raises(ValueError, match=word):
            StoreLoader(store, plan, a.pop("N"), a.pop("num_past"), a.pop("num_future"), **a)
    with pytest.raises(ValueError, match="plan expects"):
        StoreLoader(store, IngestPlan((12, 12), 1, (6, 5), device="cpu"), 2, 3, 3)
    with pytest.raises(ValueError, match="plan expects"):
        StoreLoader(DeviceClipStore(_video(30, 9, hw=(12, 10), C=3), clips, device="cpu"), plan, 2, 3, 3)
    with pytest.raises(ValueError, match="built for"):
        StoreLoader(DeviceClipStore.from_videos([frames], 3, 3, device="cpu"), plan, 2, 3, 2)
    for bad_clips, word in ((np.array([[0, 30]]), "outside the store"), (np.array([[-1, 3]]), "outside the store"), (np.zeros((0, 2), dtype=np.int64), "n_clips"),
                            (np.array([0, 3]), "n_clips"), (np.array([[0.0, 3.0]]), "integers")):
        with pytest.raises(ValueError, match=word):
            DeviceClipStore(frames, bad_clips, device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        DeviceClipStore(frames[..., 0], clips, device="cpu")
    with pytest.raises(ValueError):
        ok.seek(0, 2)
    with pytest.raises(ValueError):
        ok.seek(-1, 0)
    ok.seek(3, 1)
    assert ok.state_dict() == dict(seed=0, epoch=3, batch=1, drawn=0, batches_per_epoch=2)
    big.load_state_dict(dict(seed=K.SEEDS["both"], epoch=9, batch=4, drawn=(1 << 33) + 5, batches_per_epoch=5))
    assert big.state_dict() == dict(seed=K.SEEDS["both"], epoch=9, batch=4, drawn=(1 << 33) + 5, batches_per_epoch=5)
    with pytest.raises(ValueError, match="batches per epoch"):
        ok.load_state_dict(big.state_dict())
    with pytest.raises(RuntimeError, match="MI355X only"):                   # no CPU fallback: the launches need the device
        next(iter(ok))
