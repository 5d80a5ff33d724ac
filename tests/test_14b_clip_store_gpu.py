"""The HBM-resident clip store on the device: vptr_clip_draw and vptr_clip_ingest_gather through the C ABI against the integer emulation of
clip_store_cases.py (proven consistent by test_clip_store_cpu.py) and against the dense vptr_clip_ingest on the gathered batch, every
reject, one graph capture across an epoch wrap, and the host layer (DeviceClipStore, StoreLoader, run_epoch into a captured trainer).

Every comparison is torch.equal: the draw is integer arithmetic, the gather is the dense kernel's body on other addresses.  fp32 outputs
are NaN before each call and sit between guard floats; `sel` sits between rows of 0xA5A5A5A5 and the cursor record in front of 16 such
words.  No `sel` with a frame index outside the store is handed to the GPU: the clamp is covered by the CPU emulation."""
import functools

import numpy as np
import pytest
import torch

import clip_store_cases as K
import validation_cases as V
from ingest_ref import make_raw, ref_ingest
from test_02_model_gpu import TOL
from vptr_amd.data import ClipIngest, DeviceClipStore, IngestPlan, StoreLoader      # the module under test

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(autouse=True)
def _drop_slabs():
    yield
    from vptr_amd import ops
    ops.unregister_flat_slabs()


# ---- the draw through the C ABI ---------------------------------------------------------------------------------------------------
def abi_drive(dev, c, cursor, calls, hp=K.SWEEP_FLIPS[0], vp=K.SWEEP_FLIPS[1], table=None):
    """`calls` launches from `cursor` (16 int32 values), no sync in between; every call writes its own guarded slice of a history
    buffer and the cursor record (+ 16 guard words) is copied out after every call -> (sel [calls, N, 4], cursors [calls, 16]) on the host"""
    from vptr_amd._lib import lib, ptr, stream
    N = c["N"]
    table = (K.clip_table_for(c["n"]) if table is None else table).to(dev)
    hist = torch.full((calls, N + 2, 4), K.GUARD, dtype=torch.int32, device=dev)
    cur = torch.full((32,), K.GUARD, dtype=torch.int32, device=dev)
    cur[:16] = torch.tensor(cursor, dtype=torch.int32)
    cur_hist = torch.zeros((calls, 32), dtype=torch.int32, device=dev)
    assert cur.data_ptr() % 64 == 0
    for k in range(calls):
        rc = lib.vptr_clip_draw(ptr(cur), ptr(table), ptr(hist[k, 1:]), c["n"], N, c["rank"], c["world"], c["shuffle"], hp, vp, stream())
        assert rc == 0, lib.vptr_last_error().decode()
        cur_hist[k].copy_(cur)
    torch.cuda.synchronize()
    hist, cur_hist = hist.cpu(), cur_hist.cpu()
    assert bool((hist[:, 0] == K.GUARD).all()) and bool((hist[:, -1] == K.GUARD).all()), "guard rows around sel changed"
    assert bool((cur_hist[:, 16:] == K.GUARD).all()), "guard words behind the cursor changed"
    return hist[:, 1:-1].contiguous(), cur_hist[:, :16].contiguous()


@pytest.mark.parametrize("c", K.draw_sweep(), ids=K.draw_id)
def test_draw_sweep_two_epochs_and_one_call(dev, c):
    calls = K.draw_calls(c)
    cursor = K.cursor0(K.SEED0)
    want_sel, want_cur = K.drive_emu(cursor, K.clip_table_for(c["n"]), c["N"], c["rank"], c["world"], c["shuffle"], *K.SWEEP_FLIPS, calls)
    sel, cur = abi_drive(dev, c, cursor, calls)
    assert torch.equal(cur, want_cur), "cursor: first difference at call %d" % int((cur != want_cur).any(dim=1).nonzero()[0])
    assert torch.equal(sel, want_sel), "sel: first difference at call %d" % int((sel != want_sel).flatten(1).any(dim=1).nonzero()[0])
    assert int(cur[-1, K.CUR["EPOCH"]]) >= 2                                  # across both wraps


@pytest.mark.parametrize("c", [dict(n=257, N=16, rank=1, world=2, shuffle=1), dict(n=17, N=3, rank=0, world=1, shuffle=1)], ids=K.draw_id)
def test_draw_seed_words_start_positions_and_repeats(dev, c):
    table = K.clip_table_for(c["n"])
    got = {}
    for tag, seed in K.SEEDS.items():
        # a start in the middle of a late epoch, the drawn count about to carry into its high word
        cursor = K.cursor0(seed, epoch=123456, batch=2, drawn=(1 << 32) - 2)
        want = K.drive_emu(cursor, table, c["N"], c["rank"], c["world"], 1, 0.5, 0.5, 5)
        got[tag] = abi_drive(dev, c, cursor, 5, 0.5, 0.5)
        assert torch.equal(got[tag][0], want[0]) and torch.equal(got[tag][1], want[1]), tag
        again = abi_drive(dev, c, cursor, 5, 0.5, 0.5)                        # twice from the same cursor: bit-identical
        assert torch.equal(again[0], got[tag][0]) and torch.equal(again[1], got[tag][1])
    assert all(not torch.equal(got[a][0], got[b][0]) for a in got for b in got if a < b)
    # a batch word past the epoch is reduced modulo batches_per_epoch
    bpe = c["n"] // (c["N"] * c["world"])
    a = abi_drive(dev, c, K.cursor0(K.SEED0, batch=bpe + 1), 1)
    b = abi_drive(dev, c, K.cursor0(K.SEED0, batch=1), 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("hp,vp,bits", [(0.0, 0.0, 0), (1.0, 0.0, 1), (0.0, 1.0, 2), (1.0, 1.0, 3)])
def test_draw_flip_probabilities_0_and_1_are_exact(dev, hp, vp, bits):
    c = dict(n=4097, N=300, rank=0, world=1, shuffle=1)
    sel, _ = abi_drive(dev, c, K.cursor0(K.SEEDS["both"]), 13, hp, vp)
    assert bool((sel[..., K.SEL["FLIPS"]] == bits).all())
    assert sel[..., K.SEL["CLIP"]].unique().numel() == 13 * 300


# ---- the gather through the C ABI -------------------------------------------------------------------------------------------------
def _plan_args(plan):
    from vptr_amd._lib import ptr
    top, left, Hc, Wc = plan.crop
    Hout, Wout = plan.out_hw
    hp, vp = Wout != Wc, Hout != Hc
    tabs = (ptr(plan.kx) if hp else None, ptr(plan.bx) if hp else None, ptr(plan.ky) if vp else None, ptr(plan.by) if vp else None, ptr(plan.lut))
    dims = (plan.in_hw[0], plan.in_hw[1], plan.channels, top, left, Hc, Wc, Hout, Wout, plan.ksx if hp else 0, plan.ksy if vp else 0)
    return tabs, dims


def _guarded_outs(dev, N, Tp, Tf, C, Hout, Wout, pad=64):
    per = C * Hout * Wout
    n0, n1 = N * Tp * per, N * Tf * per
    guard = torch.arange(n0 + n1 + 3 * pad, device=dev, dtype=torch.float32) * 0.37 + 1.0
    o0 = guard[pad:pad + n0].view(N, Tp, C, Hout, Wout)
    o1 = guard[2 * pad + n0:2 * pad + n0 + n1].view(N, Tf, C, Hout, Wout)
    o0.fill_(NAN)
    o1.fill_(NAN)
    spans = ((0, pad), (pad + n0, 2 * pad + n0), (2 * pad + n0 + n1, 3 * pad + n0 + n1))
    return guard, guard.clone(), o0, o1, spans


def abi_gather(store_d, sel, plan, Tp, Tf):
    """one direct C-ABI call: sel between guard rows, the outputs NaN-filled views into a guard buffer -> (out0, out1)"""
    from vptr_amd._lib import check, lib, ptr, stream
    dev = store_d.device
    N = int(sel.shape[0])
    selbuf = torch.full((N + 2, 4), K.GUARD, dtype=torch.int32, device=dev)
    selbuf[1:-1] = sel.to(dev)
    before_sel = selbuf.clone()
    guard, before, o0, o1, spans = _guarded_outs(dev, N, Tp, Tf, plan.channels, *plan.out_hw)
    tabs, dims = _plan_args(plan)
    check(lib.vptr_clip_ingest_gather(ptr(store_d), int(store_d.shape[0]), ptr(selbuf[1:]), *tabs, ptr(o0) if Tp else None, ptr(o1) if Tf else None,
                                      N, Tp + Tf, Tp, *dims, stream()), "vptr_clip_ingest_gather")
    gi32, bi32 = guard.view(torch.int32), before.view(torch.int32)
    for lo, hi in spans:
        assert torch.equal(gi32[lo:hi], bi32[lo:hi]), "guard floats %d .. %d changed" % (lo, hi)
    assert torch.equal(selbuf, before_sel)
    return o0, o1


def abi_dense(raw_d, flips_d, plan, Tp, Tf):
    """vptr_clip_ingest on a dense batch [N, T, H, W, C] into fresh NaN tensors"""
    from vptr_amd._lib import check, lib, ptr, stream
    N = int(raw_d.shape[0])
    o0 = torch.full((N, Tp, plan.channels) + tuple(plan.out_hw), NAN, device=raw_d.device)
    o1 = torch.full((N, Tf, plan.channels) + tuple(plan.out_hw), NAN, device=raw_d.device)
    tabs, dims = _plan_args(plan)
    check(lib.vptr_clip_ingest(ptr(raw_d), *tabs, ptr(flips_d), ptr(o0) if Tp else None, ptr(o1) if Tf else None, N, Tp + Tf, Tp, *dims,
                               stream()), "vptr_clip_ingest")
    return o0, o1


def torch_gather(store_d, sel, Tp, Tf):
    """the batch gathered with torch indexing: uint8 [N, T, H, W, C] and the flips"""
    idx = K.gather_index(sel.cpu(), Tp, Tf, int(store_d.shape[0]), mut="no_clamp").to(store_d.device)
    assert int(idx.min()) >= 0 and int(idx.max()) < store_d.shape[0]
    return store_d[idx].contiguous(), sel[:, K.SEL["FLIPS"]].to(device=store_d.device, dtype=torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def gather_plan(name):
    Hin, Win, C, crop, out_hw = K.GATHER_CASES[name][:5]
    mean, std = K.consts(C)
    return IngestPlan((Hin, Win), C, out_hw, crop=crop, mean=mean, std=std, device="cuda:0")


@pytest.mark.parametrize("name", sorted(K.GATHER_CASES))
def test_gather_equals_dense_ingest_of_the_gathered_batch(dev, name):
    Tp, Tf = K.GATHER_CASES[name][6:8]
    plan, sel = gather_plan(name), K.gather_sel(name)
    store_d = torch.from_numpy(K.gather_store(name)).to(dev)
    o0, o1 = abi_gather(store_d, sel, plan, Tp, Tf)
    raw_d, flips_d = torch_gather(store_d, sel, Tp, Tf)
    d0, d1 = abi_dense(raw_d, flips_d, plan, Tp, Tf)
    assert torch.equal(o0.view(torch.int32), d0.view(torch.int32)) and torch.equal(o1.view(torch.int32), d1.view(torch.int32))
    ref = K.gather_ref(name)
    assert torch.equal(o0.cpu(), ref[:, :Tp]) and torch.equal(o1.cpu(), ref[:, Tp:])
    assert not bool(torch.isnan(o0).any()) and not bool(torch.isnan(o1).any())
    # the op, into pre-filled tensors of the caller
    import vptr_amd.ops as ops
    mine = (torch.full_like(d0, NAN), torch.full_like(d1, NAN))
    back = ops.ingest_gather(store_d, sel.to(dev), plan, (Tp, Tf), out=mine)
    assert back[0] is mine[0] and back[1] is mine[1] and torch.equal(mine[0], d0) and torch.equal(mine[1], d1)
    fresh = ops.ingest_gather(store_d, sel.to(dev), plan, (Tp, Tf))
    assert torch.equal(fresh[0], d0) and torch.equal(fresh[1], d1) and fresh[0].is_contiguous() and fresh[1].is_contiguous()


def test_gather_from_a_store_past_4_gib(dev):
    """256 x 256 x 3 frames, 21 900 of them: 4.3e9 bytes; frames 21 846 .. 21 899 start beyond byte 2^32.  Only the selected frames are
    written, the rest of the allocation is whatever it held."""
    H = W = 256
    F, per = 21900, 256 * 256 * 3
    assert F * per > 1 << 32 and 21846 * per > 1 << 32 > 21845 * per
    store_d = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    sel = torch.tensor([[21899, 21846, 1, 0], [0, 21850, 2, 1], [21847, 10922, 3, 2]], dtype=torch.int32)
    picked = sorted({int(v) for v in sel[:, :2].reshape(-1)})
    data = make_raw((1, len(picked), H, W, 3), "random", 7300)[0]
    for k, f in enumerate(picked):
        store_d[f].copy_(torch.from_numpy(data[k]))
    plan = IngestPlan((H, W), 3, (64, 64), mean=K.BAIR[0], std=K.BAIR[1], device=dev)
    o0, o1 = abi_gather(store_d, sel, plan, 1, 1)
    raw_d, flips_d = torch_gather(store_d, sel, 1, 1)
    d0, d1 = abi_dense(raw_d, flips_d, plan, 1, 1)
    assert torch.equal(o0, d0) and torch.equal(o1, d1)
    host = np.stack([np.stack([data[picked.index(int(p))], data[picked.index(int(f))]]) for p, f in sel[:, :2].tolist()])
    ref = ref_ingest(host, None, (64, 64), *K.BAIR, flips=sel[:, 2].tolist())
    assert torch.equal(o0.cpu(), ref[:, :1]) and torch.equal(o1.cpu(), ref[:, 1:])
    del store_d
    torch.cuda.empty_cache()


# ---- rejects --------------------------------------------------------------------------------------------------------------------------
def test_c_abi_rejects_write_nothing(dev):
    from vptr_amd._lib import lib, ptr, stream
    cur = torch.full((32,), K.GUARD, dtype=torch.int32, device=dev)
    cur[:16] = torch.tensor(K.cursor0(K.SEED0, epoch=3, batch=1), dtype=torch.int32)
    table = K.clip_table_for(17).to(dev)
    selbuf = torch.full((6, 4), K.GUARD, dtype=torch.int32, device=dev)
    store = torch.full((9, 20, 40, 1), 7, dtype=torch.uint8, device=dev)
    tab = torch.zeros(257 * 19, dtype=torch.int32, device=dev)
    lut = torch.zeros(3 * 256, device=dev)
    out = torch.full((3 * 3 * 8 * 257,), 7.25, device=dev)
    before = [t.clone() for t in (cur, selbuf, out, table, store)]
    P = lambda t, off=0: None if t is None else ptr(t).value + off      # noqa: E731

    good = dict(cursor=P(cur), table=P(table), sel=P(selbuf, 16), n=17, N=4, rank=0, world=1, shuffle=1, hp=0.5, vp=0.5)
    draws = [(dict(cursor=None), "null"), (dict(table=None), "null"), (dict(sel=None), "null"), (dict(cursor=P(cur, 4)), "aligned"),
             (dict(sel=P(selbuf, 20)), "aligned"), (dict(table=P(table, 4)), "aligned"), (dict(n=0), "n_clips 0"), (dict(N=0), "N 0"), (dict(world=0), "world 0"), (dict(rank=-1), "rank -1"),
             (dict(rank=1), "rank 1"), (dict(rank=2, world=2), "rank 2"), (dict(N=18), "batches_per_epoch"), (dict(N=3, world=6, rank=5), "batches_per_epoch"),
             (dict(hp=-0.01), "[0, 1]"), (dict(vp=1.01), "[0, 1]"), (dict(vp=float("nan")), "[0, 1]")]
    for change, word in draws:
        a = dict(good, **change)
        rc = lib.vptr_clip_draw(a["cursor"], a["table"], a["sel"], a["n"], a["N"], a["rank"], a["world"], a["shuffle"], a["hp"], a["vp"], stream())
        msg = lib.vptr_last_error().decode()
        assert rc != 0 and msg.startswith("clip_draw:") and word in msg, (change, rc, msg)

    g = dict(store=P(store), n_frames=9, sel=P(selbuf, 16), kx=P(tab), bx=P(tab), ky=P(tab), by=P(tab), lut=P(lut), out0=P(out), out1=P(out), N=1,
             T=3, Tp=2, Hin=20, Win=40, C=1, top=2, left=4, Hc=16, Wc=32, Hout=8, Wout=16, ksx=5, ksy=5)
    order = ("store", "n_frames", "sel", "kx", "bx", "ky", "by", "lut", "out0", "out1", "N", "T", "Tp", "Hin", "Win", "C", "top", "left", "Hc",
             "Wc", "Hout", "Wout", "ksx", "ksy")
    gathers = [(dict(store=None), "null"), (dict(sel=None), "null"), (dict(lut=None), "null"), (dict(n_frames=0), "n_frames 0"), (dict(C=2), "C 2"),
               (dict(N=0), "N 0"), (dict(T=0), "T 0"), (dict(Hin=0), "Hin 0"), (dict(Wout=257), "256"), (dict(Hout=0), "256"), (dict(left=30), "crop box"),
               (dict(top=-1), "crop box"), (dict(Hc=0), "crop box"), (dict(ksx=19), "8x"), (dict(ksy=19), "8x"), (dict(ksx=0), "8x"), (dict(Tp=4), "Tp"),
               (dict(Tp=-1), "Tp"), (dict(out1=None), "out1"), (dict(out0=None), "null output"), (dict(kx=None), "horizontal"), (dict(bx=None), "horizontal"),
               (dict(ky=None), "vertical"), (dict(by=None), "vertical"),
               (dict(N=1 << 20, T=1 << 10, Tp=2, Hin=64, Win=64, left=0, top=0, Hc=64, Wc=64, Hout=8, Wout=16), "too large"),
               (dict(N=1 << 20, T=1 << 12, Hin=1, Win=1, top=0, left=0, Hc=1, Wc=1, Hout=1, Wout=1), "workgroups of one launch")]
    for change, word in gathers:
        a = dict(g, **change)
        rc = lib.vptr_clip_ingest_gather(*[a[k] for k in order], stream())
        msg = lib.vptr_last_error().decode()
        assert rc != 0 and msg.startswith("clip_ingest_gather:") and word in msg, (change, rc, msg)
    torch.cuda.synchronize()
    for t, b in zip((cur, selbuf, out, table, store), before):
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_op_guards(dev):
    import vptr_amd.ops as ops
    plan = gather_plan("odd")
    store = torch.zeros((10, 37, 53, 3), dtype=torch.uint8, device=dev)
    sel = torch.zeros((2, 4), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="for this plan"):
        ops.ingest_gather(store[..., :1].contiguous(), sel, plan, (1, 1))
    with pytest.raises(RuntimeError, match="for this plan"):
        ops.ingest_gather(store.float(), sel, plan, (1, 1))
    with pytest.raises(RuntimeError, match="sel must be"):
        ops.ingest_gather(store, sel.long(), plan, (1, 1))
    with pytest.raises(RuntimeError, match="sel must be"):
        ops.ingest_gather(store, sel[:, :3].contiguous(), plan, (1, 1))
    with pytest.raises(RuntimeError, match="split"):
        ops.ingest_gather(store, sel, plan, (0, 0))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.ingest_gather(store, sel, plan, (1, 1), out=(torch.zeros((2, 1, 3, 19, 30), device=dev), torch.zeros((2, 2, 3, 19, 30), device=dev)))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.ingest_gather(store, sel.cpu(), plan, (1, 1))
    cur = torch.zeros(16, dtype=torch.int32, device=dev)
    table = torch.zeros((5, 2), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="cursor"):
        ops.clip_draw(cur[:8], table, sel)
    with pytest.raises(RuntimeError, match="clip_table"):
        ops.clip_draw(cur, table.long(), sel)
    with pytest.raises(RuntimeError, match="batches_per_epoch"):
        ops.clip_draw(cur, table, sel, world=3, rank=0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.clip_draw(cur.cpu(), table, sel)
    assert ops.clip_draw(cur, table, sel) is sel and cur.tolist()[K.CUR["BATCH"]] == 1


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_across_an_epoch_wrap(dev):
    """draw + gather captured once (n_clips 17, N 4: 4 batches per epoch) and replayed 9 times from a cursor at batch 2 of epoch 5: every
    replay's sel and outputs equal the eager sequence from the same cursor, and sel equals the emulation"""
    import vptr_amd.ops as ops
    Tp, Tf, n, N, replays = 2, 1, 17, 4, 9
    plan = gather_plan("odd")
    F = 2 * n + 3
    store_d = torch.from_numpy(make_raw((1, F, 37, 53, 3), "random", 7400)[0]).to(dev)
    c = torch.arange(n)
    table = torch.stack([2 * c, (2 * c + 7) % (F - Tf + 1)], dim=1).to(torch.int32)
    table_d = table.to(dev)
    start = torch.tensor(K.cursor0(K.SEEDS["high"], epoch=5, batch=2), dtype=torch.int32, device=dev)
    cur = start.clone()
    sel = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    outs = (torch.full((N, Tp, 3, 19, 30), NAN, device=dev), torch.full((N, Tf, 3, 19, 30), NAN, device=dev))

    def pair():
        ops.clip_draw(cur, table_d, sel, shuffle=True, hflip_p=0.5, vflip_p=0.5)
        ops.ingest_gather(store_d, sel, plan, (Tp, Tf), out=outs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair()                                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pair()
    runs = {}
    for mode in ("graph", "eager"):
        cur.copy_(start)
        seq = []
        for _ in range(replays):
            for o in outs:
                o.fill_(NAN)
            g.replay() if mode == "graph" else pair()
            torch.cuda.synchronize()
            seq.append((sel.cpu(), cur.cpu(), outs[0].clone(), outs[1].clone()))
        runs[mode] = seq
    g.reset()
    want_sel, want_cur = K.drive_emu(start.tolist(), table, N, 0, 1, 1, 0.5, 0.5, replays)
    assert want_cur[:, K.CUR["EPOCH"]].tolist() == [5, 6, 6, 6, 6, 7, 7, 7, 7]
    for k, (a, b) in enumerate(zip(runs["graph"], runs["eager"])):
        assert torch.equal(a[0], want_sel[k]) and torch.equal(a[1], want_cur[k]), k
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k
        assert not bool(torch.isnan(a[2]).any()) and not bool(torch.isnan(a[3]).any())
    raw_d, flips_d = torch_gather(store_d, runs["graph"][-1][0], Tp, Tf)
    d0, d1 = abi_dense(raw_d, flips_d, plan, Tp, Tf)
    assert torch.equal(runs["graph"][-1][2], d0) and torch.equal(runs["graph"][-1][3], d1)


# ---- the host layer -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kth_store():
    """55 frames of 120 x 160 grey in 11 clips of 2 + 3 frames, from videos of 23, 21 and 16 frames"""
    videos = [make_raw((1, n, 120, 160, 1), "random", 7500 + k)[0] for k, n in enumerate((23, 21, 16))]
    store = DeviceClipStore.from_videos(videos, 2, 3, device="cuda:0")
    assert store.n_clips == 11 and store.n_frames == 55 and store.frames.is_cuda
    return store, np.concatenate([videos[0][1:21], videos[1][0:20], videos[2][0:15]])


def _host_batch(frames, sel, Tp, Tf):
    idx = K.gather_index(sel, Tp, Tf, frames.shape[0]).numpy()
    return frames[idx]


def test_store_loader_epoch_equals_clip_ingest_on_host_batches(dev):
    store, frames = kth_store()
    assert torch.equal(store.frames.cpu(), torch.from_numpy(frames))
    plan = IngestPlan.kth(64, device=dev)
    loader = StoreLoader(store, plan, 2, 2, 3, hflip_p=0.5, vflip_p=0.5, seed=K.SEEDS["low"])
    ing = ClipIngest(plan, 2, 3)
    assert len(loader) == 5
    want_sel, _ = K.drive_emu(K.cursor0(K.SEEDS["low"]), store.clip_table.cpu(), 2, 0, 1, 1, 0.5, 0.5, 10)
    seen, flips = [], set()
    for epoch in range(2):
        count = 0
        for past, future in loader:
            sel = loader.last_selection().cpu()
            assert torch.equal(sel, want_sel[5 * epoch + count])
            ref_p, ref_f = ing(_host_batch(frames, sel, 2, 3), flips=sel[:, K.SEL["FLIPS"]].numpy())
            assert tuple(past.shape) == (2, 2, 1, 64, 64) and tuple(future.shape) == (2, 3, 1, 64, 64)
            assert torch.equal(past, ref_p) and torch.equal(future, ref_f)
            seen.extend(sel[:, K.SEL["CLIP"]].tolist())
            flips.update(sel[:, K.SEL["FLIPS"]].tolist())
            count += 1
        assert count == 5 and len(set(seen[10 * epoch:])) == 10
    assert seen[:10] != seen[10:] and len(flips) > 1
    assert loader.state_dict() == dict(seed=K.SEEDS["low"], epoch=2, batch=0, drawn=10, batches_per_epoch=5)


def test_store_loader_seek_and_resume(dev):
    store, _ = kth_store()
    plan = IngestPlan.kth(64, device=dev)
    mk = lambda **kw: StoreLoader(store, plan, 2, 2, 3, hflip_p=0.5, vflip_p=0.5, **kw)      # noqa: E731
    full = mk(seed=77)
    whole = []
    for _ in range(8):
        p, f = full.draw()
        whole.append((p.clone(), f.clone(), full.last_selection().clone()))
    first = mk(seed=77)
    for _ in range(3):
        first.draw()
    state = first.state_dict()
    assert state == dict(seed=77, epoch=0, batch=3, drawn=3, batches_per_epoch=5)
    resumed = mk(seed=5)
    resumed.load_state_dict(state)
    rest = list(resumed)                                                      # the rest of epoch 0: batches 3 and 4
    assert len(rest) == 2
    for k, (p, f) in enumerate(rest[-1:]):                                    # tensors of earlier batches are fresh ones: all stay valid
        assert torch.equal(p, whole[4][0]) and torch.equal(f, whole[4][1])
    assert torch.equal(rest[0][0], whole[3][0]) and torch.equal(resumed.last_selection(), whole[4][2])
    for k in range(5, 8):                                                     # and on into epoch 1
        p, f = resumed.draw()
        assert torch.equal(p, whole[k][0]) and torch.equal(f, whole[k][1]) and torch.equal(resumed.last_selection(), whole[k][2])
    assert resumed.state_dict() == dict(seed=77, epoch=1, batch=3, drawn=8, batches_per_epoch=5)
    resumed.seek(1, 1)
    p, f = resumed.draw()
    assert torch.equal(p, whole[6][0]) and torch.equal(f, whole[6][1])


def test_store_loader_sequential_pass_with_tail_and_ranks(dev):
    store, frames = kth_store()
    plan = IngestPlan.kth(64, device=dev)
    ing = ClipIngest(plan, 2, 3)
    loader = StoreLoader(store, plan, 4, 2, 3, shuffle=False, drop_last=False)
    assert len(loader) == 3
    got = [(p, f, loader.last_selection().cpu()) for p, f in loader]
    assert [int(p.shape[0]) for p, _, _ in got] == [4, 4, 3]
    assert torch.cat([s[:, K.SEL["CLIP"]] for _, _, s in got]).tolist() == list(range(11))
    table = store.clip_table.cpu()
    for p, f, sel in got:
        assert torch.equal(sel[:, :2], table[sel[:, 3].long()]) and bool((sel[:, 2] == 0).all())
        ref_p, ref_f = ing(_host_batch(frames, sel, 2, 3))
        assert torch.equal(p, ref_p) and torch.equal(f, ref_f)
    # two ranks of a world of 2 take disjoint clips of the same epoch order
    a = StoreLoader(store, plan, 2, 2, 3, seed=9, rank=0, world=2)
    b = StoreLoader(store, plan, 2, 2, 3, seed=9, rank=1, world=2)
    clips = []
    for la, lb in zip(a, b):
        clips.append(torch.stack([a.last_selection()[:, 3], b.last_selection()[:, 3]]).cpu())
    order = torch.cat([c.reshape(-1) for c in clips])
    assert len(clips) == 2 and torch.equal(order.long(), K.perm_emu(torch.arange(8), 11, 9, 0))


def test_run_epoch_into_a_captured_trainer(dev):
    """StoreLoader(out=trainer.static_inputs()) under run_epoch: the static buffers hold the loader's batch, and the epoch's meters equal
    those of the same batches handed over as tensors.  Bitwise in deterministic mode, otherwise at test_16's loss-term bar
    (TOL * |ref| + 1e-6 with the TOL of test_02_model_gpu.py)."""
    import vptr_amd.model as pkg
    from vptr_amd import ops
    from vptr_amd.meters import DeviceLossMeters
    from vptr_amd.train import run_epoch
    c = V.case("nar")
    HW, N, Tp, Tf = c["meta"]["HW"], c["meta"]["N"], c["cfg"]["Tp"], c["cfg"]["Tf"]
    L = Tp + Tf
    videos = [make_raw((1, n, HW, HW, 1), "random", 7600 + k)[0] for k, n in enumerate((3 * L + 1, 2 * L, 2 * L + 3))]
    store = DeviceClipStore.from_videos(videos, Tp, Tf, device=dev)
    assert store.n_clips == 7 and 7 // N >= 2
    plan = IngestPlan((HW, HW), 1, (HW, HW), mean=V.NORM[0], std=V.NORM[1], device=dev)
    names = ["T_total", "T_MSE", "T_GDL", "T_bpc"]
    ops.unregister_flat_slabs()
    ops.manual_seed(dev, 5)
    tr = V.trainer(pkg, c, dev)
    plain = StoreLoader(store, plan, N, Tp, Tf, hflip_p=0.5, seed=31)
    batches = [(p.clone(), f.clone()) for p, f in plain]                      # epoch 0 as tensors
    assert len(batches) == 7 // N
    tr.capture(*batches[0], warmup=1)
    snap = tr._snapshot()
    static = tr.static_inputs()
    loader = StoreLoader(store, plan, N, Tp, Tf, hflip_p=0.5, seed=31, out=static)
    m_store = run_epoch(tr, loader, True, DeviceLossMeters(names, dev))
    assert torch.equal(static[0], batches[-1][0]) and torch.equal(static[1], batches[-1][1])
    got = m_store.compute()
    tr._restore(snap)
    want = run_epoch(tr, batches, True, DeviceLossMeters(names, dev)).compute()
    for k in names:
        assert got[k]["count"] == want[k]["count"] == float(len(batches)) and got[k]["nonfinite"] == 0
        for field in ("avg", "last"):
            a, b = got[k][field], want[k][field]
            print("run_epoch %-8s %-4s store % .9e tensors % .9e |diff| %.3e" % (k, field, a, b, abs(a - b)))
            if ops.config.deterministic:
                assert a == b, (k, field, a, b)
            else:
                assert abs(a - b) <= TOL * abs(b) + 1e-6, (k, field, a, b)
