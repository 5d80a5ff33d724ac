"""Cases and integer emulation of the HBM-resident clip store (include/vptr_hip_data.h, csrc/clipstore.hip), shared by
test_clip_store_cpu.py (which proves the cases consistent and sensitive to seven named mutations) and test_14b_clip_store_gpu.py.

The emulation is read off the header: `perm` (4-round balanced Feistel network over b bits on vptr_hash3 with cycle walking), the rows
of `sel`, the flip bits keyed on the clip, the cursor's advance -- torch int64 arithmetic on helpers.hash3_emu, vectorised over a whole
sequence of draws -- and the gather as index arithmetic in front of ingest_ref.ref_ingest.  It does not use vptr_amd.data.

Mutations (argument `mut`): each breaks one rule; the CPU test asserts that every case listed for it in MUTATION_CASES then gives
another result (or raises, for "no_clamp")."""
import numpy as np
import torch

from helpers import hash3_emu
from ingest_ref import make_raw, ref_ingest

M32 = 0xFFFFFFFF
# the header's #defines
CUR = dict(SEED_LO=0, SEED_HI=1, EPOCH=2, BATCH=3, BPE=4, DRAWN_LO=5, DRAWN_HI=6, WORDS=16)
SEL = dict(PAST=0, FUTURE=1, FLIPS=2, CLIP=3, WORDS=4)
DRAW = dict(SITE_ROUND0=0, ROUNDS=4, SITE_HFLIP=4, SITE_VFLIP=5)
GUARD = 0xA5A5A5A5 - (1 << 32)         # the int32 whose bits are 0xA5A5A5A5
RESERVED = 0x5EED0000                  # what the tests put into the cursor's reserved words: it must stay

MUTATIONS = ("rank_stride", "future_from_past", "flip_by_position", "late_wrap", "no_clamp", "one_walk", "no_epoch_key")

SEED0 = 0x0123456789ABCDEF
SEEDS = {"base": SEED0, "low": SEED0 ^ 0x00000100, "high": SEED0 ^ (0x00000100 << 32), "both": SEED0 ^ 0x0000010000000100}
KTH = (0.6013795, 2.7570653)
BAIR = ((0.61749697, 0.6050092, 0.52180636), (2.1824553, 2.1553133, 1.9115673))


def s32(v):
    v = int(v) & M32
    return v - (1 << 32) if v >= (1 << 31) else v


# ---- perm -------------------------------------------------------------------------------------------------------------------------
def perm_bits(n):
    b = max(2, (int(n) - 1).bit_length())
    return b + (b & 1)


def feistel_emu(x, seed, epoch, h, mut=None):
    """E(x): x int64 tensor below 2^(2 h), epoch an int or an int64 tensor of x's shape (below 2^31)"""
    mask = (1 << h) - 1
    ehi = torch.as_tensor(epoch, dtype=torch.int64) << 32
    if mut == "no_epoch_key":
        ehi = ehi * 0
    L, R = x >> h, x & mask
    for r in range(DRAW["ROUNDS"]):
        L, R = R, L ^ (hash3_emu(seed, DRAW["SITE_ROUND0"] + r, ehi | R) & mask)
    return (L << h) | R


def perm_emu(i, n, seed, epoch, mut=None, count=None):
    """perm(i) for an int64 tensor of positions below n.  count: a list that receives the number of applications per position."""
    h = perm_bits(n) // 2
    i = torch.as_tensor(i, dtype=torch.int64)
    epoch = torch.as_tensor(epoch, dtype=torch.int64).expand_as(i)
    x = feistel_emu(i, seed, epoch, h, mut)
    walks = torch.ones_like(x)
    if mut != "one_walk":
        while True:
            m = x >= n
            if not bool(m.any()):
                break
            x = torch.where(m, feistel_emu(x, seed, epoch, h, mut), x)
            walks += m.long()
    if count is not None:
        count.append(walks)
    return x


def flip_threshold(p):
    return int(float(np.float32(p)) * 4294967296.0)        # the ABI takes a float; the launcher widens it to double


def flips_emu(key, seed, epoch, hp, vp):
    idx = (torch.as_tensor(epoch, dtype=torch.int64) << 32) | torch.as_tensor(key, dtype=torch.int64)
    return ((hash3_emu(seed, DRAW["SITE_HFLIP"], idx) < flip_threshold(hp)).long()
            | ((hash3_emu(seed, DRAW["SITE_VFLIP"], idx) < flip_threshold(vp)).long() << 1))


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def clip_table_for(n, Tp=3):
    """int32 [n, 2]: arbitrary but distinct rows (the draw only copies them)"""
    c = torch.arange(n, dtype=torch.int64)
    return torch.stack([(c * 7 + 3) % 100003, (c * 7 + 3) % 100003 + Tp + (c % 5)], dim=1).to(torch.int32)


def cursor0(seed, epoch=0, batch=0, drawn=0, bpe=0):
    w = [RESERVED + k for k in range(CUR["WORDS"])]
    w[CUR["SEED_LO"]], w[CUR["SEED_HI"]] = s32(seed), s32(seed >> 32)
    w[CUR["EPOCH"]], w[CUR["BATCH"]], w[CUR["BPE"]] = s32(epoch), s32(batch), s32(bpe)
    w[CUR["DRAWN_LO"]], w[CUR["DRAWN_HI"]] = s32(drawn), s32(drawn >> 32)
    return w


def drive_emu(cursor, table, N, rank, world, shuffle, hp, vp, calls, mut=None):
    """`calls` consecutive vptr_clip_draw launches from `cursor` (a list of 16 int32 values)
    -> (sel int32 [calls, N, 4], cursors int32 [calls, 16]: the record after each call)"""
    n = int(table.shape[0])
    bpe = n // (N * world)
    assert bpe >= 1
    u = [int(v) & M32 for v in cursor]
    seed = u[CUR["SEED_LO"]] | (u[CUR["SEED_HI"]] << 32)
    epoch0, batch0 = u[CUR["EPOCH"]], u[CUR["BATCH"]] % bpe
    drawn0 = u[CUR["DRAWN_LO"]] | (u[CUR["DRAWN_HI"]] << 32)
    period = bpe + 1 if mut == "late_wrap" else bpe          # the cursor's own walk
    k = torch.arange(calls + 1, dtype=torch.int64)
    epochs, batches = epoch0 + (batch0 + k) // period, (batch0 + k) % period
    e, b = epochs[:calls, None], (batches[:calls] % bpe)[:, None]
    j = torch.arange(N, dtype=torch.int64)[None, :]
    i = (b * world + (0 if mut == "rank_stride" else rank)) * N + j
    e = e.expand_as(i)
    clip = perm_emu(i, n, seed, e, mut) if shuffle else i
    fl = flips_emu(i if mut == "flip_by_position" else clip, seed, e, hp, vp)
    rows = table.long()[clip.clamp(max=n - 1)]               # "one_walk" may leave the clip list: the row is wrong either way
    sel = torch.stack([rows[..., 0], rows[..., 1], fl, clip], dim=-1).to(torch.int32)
    cur = torch.tensor([[s32(v) for v in cursor]], dtype=torch.int64).repeat(calls, 1)
    cur[:, CUR["EPOCH"]] = epochs[1:] & M32
    cur[:, CUR["BATCH"]] = batches[1:]
    cur[:, CUR["BPE"]] = bpe
    d = drawn0 + k[1:]
    cur[:, CUR["DRAWN_LO"]], cur[:, CUR["DRAWN_HI"]] = d & M32, (d >> 32) & M32
    cur = torch.where(cur >= (1 << 31), cur - (1 << 32), cur)
    return sel, cur.to(torch.int32)


def draw_sweep():
    """the sweep of the issue: n_clips x N x (rank, world) x shuffle, the combinations with at least one batch per epoch"""
    out = []
    for n in (1, 5, 17, 257, 4097):
        for N in (1, 3, 16, 300):
            for rank, world in ((0, 1), (1, 2), (2, 3)):
                if n // (N * world) < 1:
                    continue
                for shuffle in (1, 0):
                    out.append(dict(n=n, N=N, rank=rank, world=world, shuffle=shuffle))
    return out


def draw_id(c):
    return "n%d-N%d-r%dw%d-%s" % (c["n"], c["N"], c["rank"], c["world"], "shuf" if c["shuffle"] else "seq")


def draw_calls(c):
    """two epochs and one call more"""
    return 2 * (c["n"] // (c["N"] * c["world"])) + 1


SWEEP_FLIPS = (0.5, 0.25)


# ---- the gather ---------------------------------------------------------------------------------------------------------------------
def gather_index(sel, Tp, Tf, n_frames, mut=None):
    """int64 [N, Tp + Tf]: the store frame of every output frame"""
    sel = torch.as_tensor(sel).long()
    t = torch.arange(Tp + Tf, dtype=torch.int64)[None, :]
    past, fut = sel[:, SEL["PAST"], None] + t, sel[:, SEL["FUTURE"], None] + (t - Tp)
    f = past if mut == "future_from_past" else torch.where(t < Tp, past, fut)
    return f if mut == "no_clamp" else f.clamp(0, n_frames - 1)


def gather_emu(store, sel, Tp, Tf, mut=None):
    """store: uint8 numpy [F, H, W, C] -> (uint8 numpy [N, T, H, W, C], flips list)"""
    f = gather_index(sel, Tp, Tf, store.shape[0], mut).numpy()
    if mut == "no_clamp" and f.min() < 0:
        raise IndexError("frame index %d" % f.min())       # numpy would wrap a negative index around
    return store[f], (torch.as_tensor(sel)[:, SEL["FLIPS"]] & 3).tolist()


# name -> (Hin, Win, C, crop box or None, (Hout, Wout), F, Tp, Tf, sel rows [(past, future, flips)])
GATHER_CASES = {
    # KTH 64 with the centre crop; all four flip combinations, independent starts, the same clip twice, overlapping clips, a clip that
    # ends on the store's last frame
    "kth64": (120, 160, 1, (0, 20, 120, 120), (64, 64), 12, 2, 3, [(0, 2, 0), (7, 9, 1), (1, 3, 2), (7, 9, 3), (5, 0, 1), (6, 9, 0)]),
    "bair": (64, 64, 3, None, (64, 64), 9, 2, 2, [(0, 2, 3), (5, 7, 0), (4, 1, 2), (5, 7, 1)]),
    "odd": (37, 53, 3, None, (19, 30), 10, 3, 2, [(0, 3, 1), (5, 8, 2), (2, 2, 0), (1, 4, 3), (5, 8, 2)]),
    "upscale": (24, 20, 1, None, (40, 36), 8, 1, 3, [(0, 1, 0), (4, 5, 3), (7, 0, 1)]),
    "Tp0": (37, 53, 3, None, (19, 30), 10, 0, 4, [(9, 6, 1), (0, 0, 2), (3, 1, 0)]),
    "TpT": (37, 53, 3, None, (19, 30), 10, 4, 0, [(6, 9, 1), (0, 0, 2), (3, 1, 3)]),
}
# CPU only: frame indices outside the store are clamped (never handed to the GPU)
CLAMP_CASE = (24, 20, 1, None, (40, 36), 8, 2, 2, [(7, 30, 0), (-3, 6, 1), (100, -100, 2)])


def consts(C):
    return KTH if C == 1 else BAIR


def gather_store(name):
    g = CLAMP_CASE if name == "clamp" else GATHER_CASES[name]
    Hin, Win, C, _, _, F = g[:6]
    return make_raw((1, F, Hin, Win, C), "random", 7100 + sorted(list(GATHER_CASES) + ["clamp"]).index(name))[0]


def gather_sel(name):
    g = CLAMP_CASE if name == "clamp" else GATHER_CASES[name]
    return torch.tensor([[p, f, fl, 1000 + k] for k, (p, f, fl) in enumerate(g[8])], dtype=torch.int32)


def gather_ref(name, mut=None):
    """fp32 [N, T, C, Hout, Wout] of a gather case through the emulation and ingest_ref.ref_ingest"""
    g = CLAMP_CASE if name == "clamp" else GATHER_CASES[name]
    _, _, C, crop, out_hw, _, Tp, Tf = g[:8]
    raw, flips = gather_emu(gather_store(name), gather_sel(name), Tp, Tf, mut)
    return ref_ingest(raw, crop, out_hw, *consts(C), flips=flips)


# mutation -> what must change under it.  ("draw", case dict, calls) / ("gather", case name) / ("perm", n)
MUTATION_CASES = {
    "rank_stride": [("draw", dict(n=17, N=3, rank=1, world=2, shuffle=1), 3), ("draw", dict(n=257, N=16, rank=2, world=3, shuffle=0), 2)],
    "future_from_past": [("gather", "kth64"), ("gather", "bair"), ("gather", "upscale")],
    "flip_by_position": [("draw", dict(n=257, N=16, rank=0, world=1, shuffle=1), 2), ("draw", dict(n=17, N=3, rank=1, world=2, shuffle=1), 5)],
    "late_wrap": [("draw", dict(n=17, N=3, rank=0, world=1, shuffle=1), 6), ("draw", dict(n=5, N=1, rank=1, world=2, shuffle=0), 3)],
    "no_clamp": [("gather", "clamp")],
    "one_walk": [("perm", 17), ("perm", 257), ("perm", 4097), ("perm", 65537)],
    "no_epoch_key": [("draw", dict(n=17, N=3, rank=0, world=1, shuffle=1), 11), ("draw", dict(n=4097, N=300, rank=0, world=1, shuffle=1), 27)],
}
