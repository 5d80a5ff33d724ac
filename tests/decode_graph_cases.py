"""Cases, references and an fp32 CPU emulation for the device-held decoding position (include/vptr_hip_decode.h), shared by
tests/test_12b_decode_graph_gpu.py (the kernels through the C ABI) and tests/test_decode_graph_cpu.py (the emulation, and named
mutations of it that the same checks must catch)."""
import torch

from oracle import fill

WORDS, POS, TCAP, OVERFLOW, STEPS = 16, 0, 1, 2, 3
MAXT = 64
GUARD = 3          # NaN guard rows on either side of every buffer
TOLA = 5e-5        # the bar tests/test_12_far_cache_gpu.py holds vptr_tattn_step to against torch fp64

# (C, nh, p16): head width 12 (two floats per lane), 5 (one), 132 and 65 (a second trip of the chunk loop at either width), 66 (BAIR)
GEOMS = [(48, 4, 0), (15, 3, 0), (264, 2, 0), (130, 2, 0), (528, 8, 0), (528, 8, 1)]
ROWS = [1, 17, 64]                                    # one row, the grid's 8-row tail, a full multiple
POSITIONS = [(5, 0), (5, 1), (5, 4)]                  # (Tcap, POS)
STEP_CASES = [(rows, Tcap, pos, C, nh, p16) for (C, nh, p16) in GEOMS for rows in ROWS for (Tcap, pos) in POSITIONS]
STEP_CASES.append((17, MAXT, MAXT - 1, 48, 4, 0))     # the last of the 64 keys
FP64_CASE = (17, 5, 4, 528, 8, 0)


def step_inputs(rows, Tcap, pos, C):
    """q, knew, vnew [rows, C]; kc, vc [Tcap, rows, C] with slots >= pos NaN (never to be read); CPU fp32"""
    q, kn, vn = fill.rand_normal((rows, C), 800, 0.5), fill.rand_normal((rows, C), 801, 0.5), fill.rand_normal((rows, C), 802)
    kc, vc = fill.rand_normal((Tcap, rows, C), 803, 0.5), fill.rand_normal((Tcap, rows, C), 804)
    kc[pos:] = float("nan")
    vc[pos:] = float("nan")
    return q, kn, vn, kc, vc


def guarded(t, device="cpu"):
    """(whole, view): `t` inside GUARD NaN rows (of t's row size) on either side; the view is what the kernel gets"""
    row = t[0].numel() if t.dim() > 1 else 1
    n = t.numel()
    whole = torch.full((n + 2 * GUARD * row,), float("nan"), dtype=t.dtype)
    whole[GUARD * row:GUARD * row + n] = t.reshape(-1)
    whole = whole.to(device)
    return whole, whole[GUARD * row:GUARD * row + n].view(t.shape)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guards_hold(whole, view):
    """the guard rows around `view` are still NaN bit for bit (the canonical NaN `guarded` wrote)"""
    n = view.numel()
    g = (whole.numel() - n) // 2
    nan = bits(torch.full((g,), float("nan")))
    w = bits(whole)
    return torch.equal(w[:g], nan) and torch.equal(w[g + n:], nan)


def step_ref64(q, kc, vc, Tk, nh):
    """tests/test_12_far_cache_gpu.py::step_ref"""
    rows, C = q.shape
    hd = C // nh
    qh = q.double().reshape(rows, nh, hd)
    kh = kc[:Tk].double().reshape(Tk, rows, nh, hd)
    vh = vc[:Tk].double().reshape(Tk, rows, nh, hd)
    p = torch.einsum("rhd,jrhd->rhj", qh, kh).softmax(dim=-1)
    return torch.einsum("rhj,jrhd->rhd", p, vh).reshape(rows, C)


def record(pos, tcap, overflow=0, steps=0):
    r = torch.zeros(WORDS, dtype=torch.int32)
    r[POS], r[TCAP], r[OVERFLOW], r[STEPS] = pos, tcap, overflow, steps
    return r


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
MUTATIONS = ("slot_plus_one", "pos_keys", "stale_slot", "advance_unbounded", "tpos_minus_one")


def emu_begin(rec, tpos, cur, mut=None):
    t, Tmax = int(rec[POS]), tpos.shape[0]
    if t < 0 or t >= min(int(rec[TCAP]), Tmax):
        return
    cur.copy_(tpos[t - 1 if mut == "tpos_minus_one" else t])


def emu_advance(rec, mut=None):
    t = int(rec[POS])
    if (0 <= t < int(rec[TCAP])) or mut == "advance_unbounded":
        rec[POS] += 1
        rec[STEPS] += 1
    else:
        rec[OVERFLOW] += 1


def emu_step_pos(q, kn, vn, kc, vc, o, rec, nh, mut=None):
    """fp32; writes slot POS of kc / vc and o in place, as vptr_tattn_step_pos does"""
    t, Tcap = int(rec[POS]), kc.shape[0]
    if t < 0 or t >= Tcap or t >= MAXT:
        return
    rows, C = q.shape
    hd = C // nh
    old_k, old_v = kc[t].clone(), vc[t].clone()
    slot = t + 1 if mut == "slot_plus_one" else t
    if slot < Tcap:
        kc[slot], vc[slot] = kn, vn
    Tk = t if mut == "pos_keys" else t + 1
    keys = torch.cat([kc[:t], (old_k if mut == "stale_slot" else kn)[None]])[:Tk]
    vals = torch.cat([vc[:t], (old_v if mut == "stale_slot" else vn)[None]])[:Tk]
    qh = q.reshape(rows, nh, hd)
    p = torch.einsum("rhd,jrhd->rhj", qh, keys.reshape(Tk, rows, nh, hd)).softmax(dim=-1)
    o.copy_(torch.einsum("rhj,jrhd->rhd", p, vals.reshape(Tk, rows, nh, hd)).reshape(rows, C))


# ------------------------------------------------------------------------------------------------ the checks both files run
def check_step_case(run, case, device="cpu", reference=None, decode=None):
    """run(q, kn, vn, kc, vc, o, rec, rows, Tcap, C, nh, p16) performs one vptr_tattn_step_pos on guarded, NaN-filled buffers.
    reference(q, kc_filled, vc_filled, Tk, ...) -> o to compare with bit for bit (the GPU file: vptr_tattn_step); None: torch fp64 at TOLA.
    Returns a list of failed property names (empty: the case holds)."""
    rows, Tcap, pos, C, nh, p16 = case
    q, kn, vn, kc, vc = step_inputs(rows, Tcap, pos, C)
    kfill, vfill = kc.clone(), vc.clone()
    kfill[pos], vfill[pos] = kn, vn
    (wq, dq), (wkn, dkn), (wvn, dvn) = guarded(q, device), guarded(kn, device), guarded(vn, device)
    (wkc, dkc), (wvc, dvc) = guarded(kc, device), guarded(vc, device)
    wo, do = guarded(torch.full((rows, C), float("nan")), device)
    rec = record(pos, Tcap).to(device)
    run(dq, dkn, dvn, dkc, dvc, do, rec, rows, Tcap, C, nh, p16)
    bad = []
    if reference is not None:
        if not same_bits(do, reference(q, kfill, vfill, pos + 1, rows, Tcap, C, nh, p16)):
            bad.append("o differs from vptr_tattn_step")
    else:
        got = do.detach().cpu()
        ref = step_ref64(q, kfill, vfill, pos + 1, nh)
        err = float((got.double() - ref).norm() / ref.norm()) if bool(torch.isfinite(got).all()) else float("inf")
        if not err < TOLA:
            bad.append("o vs fp64: %.3e" % err)
    if not (same_bits(dkc[pos], kn) and same_bits(dvc[pos], vn)):
        bad.append("slot POS is not knew / vnew")
    if not (same_bits(dkc[:pos], kc[:pos]) and same_bits(dvc[:pos], vc[:pos])):
        bad.append("a slot below POS changed")
    if not (same_bits(dkc[pos + 1:], kc[pos + 1:]) and same_bits(dvc[pos + 1:], vc[pos + 1:])):
        bad.append("a slot above POS is no longer NaN")
    for name, w, d in (("q", wq, dq), ("knew", wkn, dkn), ("vnew", wvn, dvn), ("kcache", wkc, dkc), ("vcache", wvc, dvc), ("o", wo, do)):
        if not guards_hold(w, d):
            bad.append("guard of %s" % name)
    if not (same_bits(dq, q) and same_bits(dkn, kn) and same_bits(dvn, vn)):
        bad.append("an input changed")
    if not torch.equal(rec.cpu(), record(pos, Tcap)):
        bad.append("the record changed")
    return bad


def check_full_case(run, rows, Tcap, C, nh, device="cpu"):
    """POS == Tcap: caches, o and guards untouched.  -> failed property names"""
    q, kn, vn, kc, vc = step_inputs(rows, Tcap, Tcap, C)
    (wq, dq), (wkn, dkn), (wvn, dvn) = guarded(q, device), guarded(kn, device), guarded(vn, device)
    (wkc, dkc), (wvc, dvc) = guarded(kc, device), guarded(vc, device)
    wo, do = guarded(torch.full((rows, C), float("nan")), device)
    rec = record(Tcap, Tcap).to(device)
    run(dq, dkn, dvn, dkc, dvc, do, rec, rows, Tcap, C, nh, 0)
    bad = []
    if not (same_bits(dkc, kc) and same_bits(dvc, vc)):
        bad.append("a cache changed")
    if not same_bits(do, torch.full((rows, C), float("nan"))):
        bad.append("o was written")
    for name, w, d in (("kcache", wkc, dkc), ("vcache", wvc, dvc), ("o", wo, do)):
        if not guards_hold(w, d):
            bad.append("guard of %s" % name)
    return bad


def check_begin(run, C, Tmax, device="cpu"):
    """run(rec, tpos, cur, Tmax, C): tpos_cur == tpos[POS] at POS 0, 1, Tmax - 1; nothing at POS = Tmax (TCAP above it) and at
    POS = TCAP < Tmax; guards.  -> failed property names"""
    tpos = fill.rand_normal((Tmax, C), 810)
    bad = []
    for pos, tcap in ((0, Tmax), (1, Tmax), (Tmax - 1, Tmax), (Tmax, Tmax + 2), (2, 2)):
        wt, dt = guarded(tpos, device)
        wc, dc = guarded(torch.full((C,), float("nan")), device)
        rec = record(pos, tcap).to(device)
        run(rec, dt, dc, Tmax, C)
        want = tpos[pos] if pos < min(tcap, Tmax) else torch.full((C,), float("nan"))
        if not same_bits(dc, want):
            bad.append("tpos_cur at POS %d, TCAP %d" % (pos, tcap))
        if not (guards_hold(wc, dc) and guards_hold(wt, dt) and same_bits(dt, tpos)):
            bad.append("guards at POS %d" % pos)
        if not torch.equal(rec.cpu(), record(pos, tcap)):
            bad.append("the record changed at POS %d" % pos)
    return bad


def check_advance(run, Tcap, device="cpu"):
    """run(rec): Tcap + 2 calls from POS = 0, the four words after each (the reserved words stay as they were).  -> failures"""
    base = torch.arange(100, 100 + WORDS, dtype=torch.int32)
    rec = base.clone()
    rec[POS], rec[TCAP], rec[OVERFLOW], rec[STEPS] = 0, Tcap, 0, 0
    rec = rec.to(device)
    bad = []
    for i in range(1, Tcap + 3):
        run(rec)
        want = base.clone()
        want[POS], want[TCAP], want[OVERFLOW], want[STEPS] = min(i, Tcap), Tcap, max(0, i - Tcap), min(i, Tcap)
        if not torch.equal(rec.cpu(), want):
            bad.append("after call %d: %s" % (i, rec.cpu().tolist()[:4]))
    return bad
