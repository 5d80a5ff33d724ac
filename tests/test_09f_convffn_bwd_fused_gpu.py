"""Op-level fp64 parity of the conv-FFN backward between norm2 and the depthwise 3x3 in its two-launch form (include/vptr_hip_convffn.h):
`vptr_norm_act_bwd_sums` (norm2's affine gradients and frame sums, no dx pass) followed by `vptr_dwconv3x3_norm_bwd` (norm2's dx arithmetic in
the load path of the depthwise data / weight / bias gradients) -- through the C ABI --, their documented rejections, and one integration test
of the combined autograd node through `MlpDWBN`.

Reference, fp64 all the way: helpers.norm_act_ln_bwd_ref on (y2, w2, b2, dy, regenerated dropout mask) gives the gradient g2 w.r.t. the
depthwise output and norm2's affine gradients; fp64 F.conv2d(groups = F, padding = 1) autograd with g2 as the upstream gradient gives da, dw9
and db.  The x operand of that step is the fp16-ROUNDED activation the kernel reads (as in test_dwconv3x3_bwd_weight_classes), so the rounding
of the side copy is no part of the error.  da is NaN-filled before every call, dw9 / db start from non-zero values the reference includes.

Bars: rel-L2 < 5e-5 against fp64 for da, dw9, db (fp32 vector kernels' gradients), and on the same inputs the fused error
is at most twice that of the three-call path (`vptr_norm_act_bwd` + `vptr_dwconv3x3_bwd_xh`): the summation orders differ, the arithmetic does
not.  Measured values: profiles/convffn_bwd_fused_margins.md.
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import KINK_CAP, norm_act_ln_bwd_ref, rel
from oracle import fill

pytestmark = pytest.mark.gpu

TOLG = 5e-5
NAN = float("nan")
SITE = 21

# id -> (frames, H, W, F)
#   1x8x8x64:    one channel slab, one frame
#   5x8x8x192:   three slabs; five frames: no group size divides them (groups of 2: 2 + 2 + 1)
#   70x4x4x128:  >= 64 frames -> step 1 runs its chunked (atomic: four chunks) and deferred (partials: 14 chunks of 5) classes, the launcher's own
#                group size is 8: a tail group of 6 (groups of 4: a tail of 2); W / 2 = 2; 16 pixels: one live pixel slot of four per thread
#   9x4x8x64:    H != W: halo indexing of a non-square map; 32 pixels: two live pixel slots
CASES = {"1x8x8x64": (1, 8, 8, 64), "5x8x8x192": (5, 8, 8, 192), "70x4x4x128": (70, 4, 4, 128), "9x4x8x64": (9, 4, 8, 64)}
# (case, form of step 1, frames per workgroup: 0 = the launcher's choice)
VARIANTS = [("1x8x8x64", "atomic", 0), ("5x8x8x192", "atomic", 0), ("5x8x8x192", "atomic", 2), ("70x4x4x128", "atomic", 0),
            ("70x4x4x128", "atomic", 4), ("70x4x4x128", "partials", 0), ("9x4x8x64", "atomic", 0), ("9x4x8x64", "atomic", 4)]
ACTS = {"none": 0, "gelu": 1}


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def abi():
    from vptr_amd import _lib
    return _lib


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def cdiv(a, b):
    return (a + b - 1) // b


@contextlib.contextmanager
def deterministic(ops, on):
    prev = ops.config.deterministic
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(prev)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    frames, H, W, Fc = CASES[case]
    rows, HW = frames * H * W, H * W
    seed = 5000 + 20 * sorted(CASES).index(case)
    return dict(y2=rn((rows, Fc), seed, 2.0) + 0.3, dy=rn((rows, Fc), seed + 1), w2=rn((HW, Fc), seed + 2).abs() + 0.5, b2=rn((HW, Fc), seed + 3, 0.3),
                ah=rn((rows, Fc), seed + 4).half(), w=rn((Fc, 1, 3, 3), seed + 5, 0.3), dw90=rn((9, Fc), seed + 6, 0.5), db0=rn((Fc,), seed + 7, 0.5),
                dw20=rn((HW, Fc), seed + 8, 0.5), db20=rn((HW, Fc), seed + 9, 0.5))


def _mask(ops, abi, dev, n, p):
    """the dropout mask of (seed scope, SITE) regenerated through vptr_dropout (element index = row * F + col): (seed tensor, 0 / 1 mask)"""
    ops.manual_seed(dev, 97531)
    seed = ops.new_seed_scope(dev)
    ones, md = torch.ones(n, device=dev), torch.empty(n, device=dev)
    abi.check(abi.lib.vptr_dropout(abi.ptr(ones), abi.ptr(md), n, p, abi.ptr(seed), SITE, abi.stream()), "vptr_dropout")
    mask = (md != 0).float().cpu()
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    return seed, mask


@functools.lru_cache(maxsize=None)
def _reference(ops, abi, dev, case, act, p):
    """(seed tensor or None, fp64 reference) of one (case, activation, dropout) -- shared by the variants of the case"""
    frames, H, W, Fc = CASES[case]
    rows, HW = frames * H * W, H * W
    t = _inputs(case)
    seed, mask = (None, None)
    if p > 0:
        seed, mask = _mask(ops, abi, dev, rows * Fc, p)
        mask = mask.reshape(rows, Fc)
    ref = norm_act_ln_bwd_ref(t["y2"], t["w2"], t["b2"], t["dy"], frames, HW, act, mask, 1.0 - p)
    assert ref["kink_share"] <= KINK_CAP

    def nchw(x):
        return x.double().reshape(frames, H, W, Fc).permute(0, 3, 1, 2)
    ar, wr = nchw(t["ah"]).clone().requires_grad_(True), t["w"].double().requires_grad_(True)
    br = torch.zeros(Fc, dtype=torch.float64, requires_grad=True)
    F.conv2d(ar, wr, br, padding=1, groups=Fc).backward(nchw(ref["dx"]))
    out = dict(da=ar.grad.permute(0, 2, 3, 1).reshape(rows, Fc), dw9=t["dw90"].double() + wr.grad.reshape(Fc, 9).t(), db=t["db0"].double() + br.grad,
               dw2=ref["dw"], db2=ref["db"], mean=ref["mean"].float(), rstd=ref["rstd"].float(), g2=ref["dx"])
    return seed, out


@functools.lru_cache(maxsize=None)
def _run(ops, abi, dev, case, form, fpg, act, p):
    """both routes on one (variant, activation, dropout): rel-L2 of the fused and of the three-call outputs against fp64, of the two routes
    against each other ("gap"), and of step 1's affine gradients"""
    lib, ptr, check, stream = abi.lib, abi.ptr, abi.check, abi.stream
    frames, H, W, Fc = CASES[case]
    rows, HW, E = frames * H * W, H * W, H * W * Fc
    t = _inputs(case)
    seed, ref = _reference(ops, abi, dev, case, act, p)
    d = {k: t[k].to(dev) for k in ("y2", "dy", "w2", "b2", "ah")}
    w9 = t["w"].reshape(Fc, 9).t().contiguous().to(dev)
    mean, rstd = ref["mean"].to(dev), ref["rstd"].to(dev)
    nscratch = max(2 * Fc, 2 * frames * (1 + 4 * cdiv(E // 4, 256)))
    res = {}
    with deterministic(ops, False):
        # ---- fused route: step 1 (sums), step 2 (the kernel)
        scratch = torch.full((nscratch,), NAN, device=dev)
        dw2, db2 = t["dw20"].clone().to(dev), t["db20"].clone().to(dev)
        nparts = lib.vptr_norm_act_bwd_partials(rows, Fc, HW, 0)
        part = None
        if form == "partials":
            assert nparts == cdiv(frames, cdiv(frames, 16)) and nparts > 0
            part = torch.full((nparts, 2, E), NAN, device=dev)
        check(lib.vptr_norm_act_bwd_sums(ptr(d["dy"]), ptr(d["y2"]), ptr(mean), ptr(rstd), ptr(d["w2"]), ptr(d["b2"]), ptr(dw2), ptr(db2), ptr(scratch),
                                         rows, Fc, HW, act, p, ptr(seed), SITE, ptr(part), stream()), "vptr_norm_act_bwd_sums")
        da = torch.full((rows, Fc), NAN, device=dev)
        dw9, db = t["dw90"].clone().to(dev), t["db0"].clone().to(dev)
        check(lib.vptr_dwconv3x3_norm_bwd(ptr(d["dy"]), ptr(d["y2"]), ptr(mean), ptr(rstd), ptr(d["w2"]), ptr(d["b2"]), ptr(scratch), act, p, ptr(seed), SITE,
                                          ptr(d["ah"]), ptr(w9), ptr(da), ptr(dw9), ptr(db), frames, H, W, Fc, fpg, stream()), "vptr_dwconv3x3_norm_bwd")
        # ---- three-call route on the same inputs
        scratch3 = torch.full((nscratch,), NAN, device=dev)
        g2 = torch.full((rows, Fc), NAN, device=dev)
        dw23, db23 = t["dw20"].clone().to(dev), t["db20"].clone().to(dev)
        check(lib.vptr_norm_act_bwd(ptr(d["dy"]), ptr(d["y2"]), ptr(mean), ptr(rstd), ptr(d["w2"]), ptr(d["b2"]), ptr(g2), ptr(dw23), ptr(db23), ptr(scratch3),
                                    rows, Fc, HW, 0, act, 0, p, ptr(seed), SITE, None, 1, 1, 0, stream()), "vptr_norm_act_bwd")
        da3 = torch.full((rows, Fc), NAN, device=dev)
        dw93, db3 = t["dw90"].clone().to(dev), t["db0"].clone().to(dev)
        check(lib.vptr_dwconv3x3_bwd_xh(ptr(g2), ptr(d["ah"]), ptr(w9), ptr(da3), ptr(dw93), ptr(db3), frames, H, W, Fc, stream()), "vptr_dwconv3x3_bwd_xh")
    torch.cuda.synchronize()
    for k, a, b in (("da", da, da3), ("dw9", dw9, dw93), ("db", db, db3)):
        res["fused_" + k] = rel(a, ref[k])
        res["three_" + k] = rel(b, ref[k])
        res["gap_" + k] = rel(a, b)
    res["three_g2"] = rel(g2, ref["g2"])
    # step 1: the frame sums the kernel read and the affine gradients, in either destination
    res["sums_finite"] = bool(torch.isfinite(scratch[:2 * frames]).all())
    res["sums_vs_three"] = rel(scratch[:2 * frames], scratch3[:2 * frames].double())
    if form == "partials":
        sums = part.double().sum(0).cpu()
        res["dw2"], res["db2"] = rel(sums[0].reshape(HW, Fc), ref["dw2"]), rel(sums[1].reshape(HW, Fc), ref["db2"])
        res["untouched"] = bool(torch.equal(dw2.cpu(), t["dw20"]) and torch.equal(db2.cpu(), t["db20"]))
    else:
        res["dw2"], res["db2"] = rel(dw2, t["dw20"].double() + ref["dw2"]), rel(db2, t["db20"].double() + ref["db2"])
        res["untouched"] = True
    return res


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("case,form,fpg", VARIANTS, ids=["%s-%s-g%d" % v for v in VARIANTS])
def test_fused_bwd_vs_fp64(ops, dev, abi, case, form, fpg, act, p):
    """da, dw9, db of the two-launch route vs fp64 (< 5e-5) and vs the three-call route's own error (at most twice it); step 1's affine gradients
    (atomics onto non-zero start values, or the partial rows summed with dw / db left alone) vs fp64; its frame sums are those of vptr_norm_act_bwd"""
    r = _run(ops, abi, dev, case, form, fpg, ACTS[act], p)
    print({k: ("%.3e" % v if isinstance(v, float) else v) for k, v in r.items()})
    assert r["sums_finite"] and r["untouched"]
    assert r["sums_vs_three"] < 1e-6          # same kernels, same geometry (the atomic form's chunks retire in any order: not bit-equal)
    assert r["dw2"] < TOLG and r["db2"] < TOLG
    assert r["three_g2"] < TOLG
    for k in ("da", "dw9", "db"):
        assert r["fused_" + k] < TOLG, k
        assert r["three_" + k] < TOLG, k
        assert r["fused_" + k] <= 2.0 * r["three_" + k], (k, r["fused_" + k], r["three_" + k])


REJECTS = {"odd_W": (4, 4, 5, 64, False), "F_48": (4, 8, 8, 48, False), "map_128_pixels": (2, 16, 8, 64, False), "deterministic": (4, 8, 8, 64, True)}


@pytest.mark.parametrize("why", sorted(REJECTS))
def test_fused_bwd_rejects(ops, dev, abi, why):
    """odd W, F % 64 != 0, a map beyond the 64-pixel bound, the deterministic mode: < 0 with a message, nothing launched -- da keeps its NaN fill,
    dw9 / db their start values"""
    lib, ptr, stream = abi.lib, abi.ptr, abi.stream
    frames, H, W, Fc, det = REJECTS[why]
    rows, HW = frames * H * W, H * W
    dy, y2, w2, b2 = rn((rows, Fc), 1).to(dev), rn((rows, Fc), 2).to(dev), rn((HW, Fc), 3).to(dev), rn((HW, Fc), 4).to(dev)
    ah, w9 = rn((rows, Fc), 5).half().to(dev), rn((9, Fc), 6).to(dev)
    mean, rstd, fsum = torch.zeros(frames, device=dev), torch.ones(frames, device=dev), torch.zeros(2 * frames, device=dev)
    dw90, db0 = rn((9, Fc), 7), rn((Fc,), 8)
    da, dw9, db = torch.full((rows, Fc), NAN, device=dev), dw90.clone().to(dev), db0.clone().to(dev)
    with deterministic(ops, det):
        rc = lib.vptr_dwconv3x3_norm_bwd(ptr(dy), ptr(y2), ptr(mean), ptr(rstd), ptr(w2), ptr(b2), ptr(fsum), 1, 0.0, None, 0, ptr(ah), ptr(w9), ptr(da),
                                         ptr(dw9), ptr(db), frames, H, W, Fc, 0, stream())
        msg = lib.vptr_last_error().decode()
    assert rc < 0 and "dwconv3x3_norm_bwd" in msg
    torch.cuda.synchronize()
    assert bool(torch.isnan(da).all()) and torch.equal(dw9.cpu(), dw90) and torch.equal(db.cpu(), db0)


def _mlp(dev):
    from vptr_amd.model import vidhrformer as V
    N, T, H, W, C, hidden = 2, 3, 8, 8, 64, 256
    m = V.MlpDWBN(H, W, C, hidden_features=hidden, out_features=C, drop=0.1, AR_model=True)
    fill.apply_fill(m, 11)
    rows = N * T * H * W
    return m.to(dev).train(), V.Geom(N, T, H, W), rows, C, hidden


def test_mlp_dwbn_routes_agree(ops, dev, abi):
    """MlpDWBN (LayerNorm variant), 6 frames of 8 x 8, C = 64, hidden 256, dropout 0.1: input gradient and every parameter gradient with
    config.fused_convffn_bwd on and off at the same seed.  Bar: the largest rel-L2 between the two routes over the op cases above (all variants,
    activations and dropout settings).  The forward pass is not bit-reproducible from run to run (its frame statistics meet in atomics: two
    forwards at one seed differ by ~1e-8, their fc1 gradients by more than the bar whatever the route), so both backward passes run on ONE forward:
    the combined node reads the attribute again at backward time.  Its fused launch must have run exactly once with the attribute on and not
    at all with it off."""
    from vptr_amd.ops import convffn
    bar = max(_run(ops, abi, dev, case, form, fpg, act, p)["gap_" + k]
              for case, form, fpg in VARIANTS for act in ACTS.values() for p in (0.0, 0.1) for k in ("da", "dw9", "db"))
    m, g, rows, C, hidden = _mlp(dev)
    cot = rn((rows, C), 33).to(dev)
    assert ops.norm_dwconv_ok(rows, g.H * g.W, hidden, g.H, g.W) and ops.norm_dwconv_bwd_ok(g.H * g.W, hidden, g.H, g.W)
    grads = {}
    prev = ops.config.fused_convffn_bwd
    try:
        ops.config.fused_convffn_bwd = True
        ops.manual_seed(dev, 2468)
        ops.new_seed_scope(dev)
        u, res = rn((rows, C), 31).to(dev).requires_grad_(True), rn((rows, C), 32).to(dev).requires_grad_(True)
        loss = (m.forward_tokens(u, res, g, 5) * cot).sum()
        for on in (True, False):
            ops.config.fused_convffn_bwd = on
            m.zero_grad(set_to_none=True)
            u.grad = res.grad = None
            before = convffn.fused_bwd_calls
            loss.backward(retain_graph=on)
            torch.cuda.synchronize()
            assert convffn.fused_bwd_calls - before == (1 if on else 0)
            grads[on] = dict({k: v.grad.detach().clone() for k, v in m.named_parameters()}, u=u.grad.clone(), res=res.grad.clone())
    finally:
        ops.config.fused_convffn_bwd = prev
        ops.discard_wgrads()
    worst = {k: rel(grads[True][k], grads[False][k]) for k in grads[True]}
    print("bar %.3e" % bar, {k: "%.3e" % v for k, v in worst.items()})
    assert set(worst) >= {"u", "fc1.weight", "norm1.weight", "dw3x3.weight", "dw3x3.bias", "norm2.weight", "norm2.bias", "fc2.weight", "norm3.weight"}
    assert all(float(v.abs().max()) > 0 for v in grads[True].values())
    for k, v in worst.items():
        assert v <= bar, (k, v, bar)


def test_mlp_dwbn_attribute_off_keeps_two_nodes(ops, dev):
    """with the attribute off at FORWARD time MlpDWBN builds the two nodes of before (no combined node in the graph, no fused launch)"""
    from vptr_amd.ops import convffn
    m, g, rows, C, hidden = _mlp(dev)
    u, res = rn((rows, C), 31).to(dev).requires_grad_(True), rn((rows, C), 32).to(dev)
    seen = {}
    for on in (True, False):
        calls = []
        orig = ops.norm_dwconv3x3_norm
        prev = ops.config.fused_convffn_bwd
        ops.config.fused_convffn_bwd = on
        ops.norm_dwconv3x3_norm = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            before = convffn.fused_bwd_calls
            m.forward_tokens(u, res, g, 5).sum().backward()
            torch.cuda.synchronize()
            seen[on] = (len(calls), convffn.fused_bwd_calls - before)
        finally:
            ops.norm_dwconv3x3_norm = orig
            ops.config.fused_convffn_bwd = prev
            ops.discard_wgrads()
    assert seen == {True: (1, 1), False: (0, 0)}
