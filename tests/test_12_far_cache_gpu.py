"""KV-cached autoregressive decoding of VPTRFormerFAR: the vptr_tattn_step kernel through the C ABI against torch fp64, the
projection + step op, `forward_cached` against the oracle's single full causal pass (the cached path must reproduce it: every
sub-layer but the causal temporal attention is frame-local in eval mode, tests/test_far_cache_cpu.py), the cached rollouts and
the guards."""
import pytest
import torch
import torch.nn.functional as F

from helpers import build_transformer, jload, load, rel
from oracle import fill
from oracle import vptr_oracle as O

pytestmark = pytest.mark.gpu

TOLA = 5e-5   # attention cores (tests/test_00_ops_gpu.py::test_temporal_attention)
TOL3 = 3e-5   # split-bf16 GEMM (tests/test_00_ops_gpu.py)
TOL = 1e-3    # the project's model bar (tests/test_02_model_gpu.py)


@pytest.fixture(scope="module")
def ops():
    import vptr_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def pkg():
    import vptr_amd.model as pkg
    return pkg


def rn(shape, seed, scale=1.0):
    return fill.rand_normal(shape, seed, scale)


def step_ref(q, kc, vc, Tk, nh):
    """fp64: o[r, h] = softmax_j(q[r,h] . k[j,r,h]) v[j,r,h], j < Tk; q [rows, C], kc / vc [Tcap, rows, C] time-major"""
    rows, C = q.shape
    hd = C // nh
    qh = q.double().reshape(rows, nh, hd)
    kh = kc[:Tk].double().reshape(Tk, rows, nh, hd)
    vh = vc[:Tk].double().reshape(Tk, rows, nh, hd)
    p = torch.einsum("rhd,jrhd->rhj", qh, kh).softmax(dim=-1)
    return torch.einsum("rhj,jrhd->rhd", p, vh).reshape(rows, C)


# ------------------------------------------------------------------------------------------------------ 1. the kernel
STEP_CASES = [(5, 1, 3, 12, 2),      # one key: softmax of one element; spare capacity
              (67, 17, 20, 48, 8),   # rows no multiple of 8 or 64, more than 16 keys, head width 6
              (3, 64, 64, 132, 2),   # the limit of 64 keys, head width 66
              (64, 29, 30, 528, 8),  # the BAIR model's head geometry at one sample
              (9, 6, 6, 80, 5)]      # head width 16, odd head count


def _step_inputs(rows, Tk, Tcap, C, dev):
    q = rn((rows, C), 700, 0.5)
    kc, vc = rn((Tcap, rows, C), 701, 0.5), rn((Tcap, rows, C), 702)
    kc[Tk:] = float("nan")           # the kernel must not read a slot past Tk
    vc[Tk:] = float("nan")
    return q, kc, vc


@pytest.mark.parametrize("rows,Tk,Tcap,C,nh", STEP_CASES)
def test_tattn_step_kernel(ops, dev, rows, Tk, Tcap, C, nh):
    from vptr_amd._lib import check, lib, ptr, stream
    q, kc, vc = _step_inputs(rows, Tk, Tcap, C, dev)
    ref = step_ref(q, kc, vc, Tk, nh)
    qd, kd, vd = q.to(dev), kc.to(dev), vc.to(dev)
    o = torch.full((rows, C), float("nan"), device=dev)
    check(lib.vptr_tattn_step(ptr(qd), ptr(kd), ptr(vd), ptr(o), rows, Tk, Tcap, C, nh, 0, stream()), "vptr_tattn_step")
    assert bool(torch.isfinite(o).all())
    err = rel(o, ref)
    print("tattn_step rows %d Tk %d C %d nh %d: rel %.3e" % (rows, Tk, C, nh, err))
    assert err < TOLA


@pytest.mark.parametrize("rows,Tk,Tcap,C,nh", [c for c in STEP_CASES if c[3] in (48, 528)])
def test_tattn_step_kernel_p16_output(ops, dev, rows, Tk, Tcap, C, nh):
    from vptr_amd._lib import check, lib, ptr, stream
    q, kc, vc = _step_inputs(rows, Tk, Tcap, C, dev)
    ref = step_ref(q, kc, vc, Tk, nh)
    qd, kd, vd = q.to(dev), kc.to(dev), vc.to(dev)
    o = torch.zeros((rows, C), device=dev)
    check(lib.vptr_tattn_step(ptr(qd), ptr(kd), ptr(vd), ptr(o), rows, Tk, Tcap, C, nh, 1, stream()), "vptr_tattn_step")
    got = ops.p16_decode(o)
    assert bool(torch.isfinite(got).all())
    err = rel(got, ref)
    print("tattn_step p16 rows %d Tk %d C %d: rel %.3e" % (rows, Tk, C, err))
    assert err < TOLA


# ------------------------------------------------------------------------------------------------------ 2. rejections
@pytest.mark.parametrize("Tk,Tcap,C,nh,p16", [(65, 66, 12, 2, 0),   # Tk above the kernel's 64 keys
                                              (4, 3, 12, 2, 0),     # Tk above the capacity
                                              (2, 3, 12, 5, 0),     # C % nh != 0
                                              (2, 3, 12, 2, 1),     # P16 output with C % 16 != 0
                                              (0, 3, 12, 2, 0)])    # no key at all
def test_tattn_step_rejects(dev, Tk, Tcap, C, nh, p16):
    from vptr_amd._lib import lib, ptr, stream
    rows = 2
    q = torch.zeros((rows, C), device=dev)
    kc = torch.zeros((max(Tk, Tcap), rows, C), device=dev)
    vc = torch.zeros_like(kc)
    o = torch.full((rows, C), 7.25, device=dev)
    rc = lib.vptr_tattn_step(ptr(q), ptr(kc), ptr(vc), ptr(o), rows, Tk, Tcap, C, nh, p16, stream())
    assert rc != 0
    msg = lib.vptr_last_error().decode()
    assert "tattn_step" in msg, msg
    torch.cuda.synchronize()
    assert bool((o == 7.25).all())      # nothing was launched


# ------------------------------------------------------------------------------------------------------ 3. the op
@pytest.mark.parametrize("rows,C,p16", [(67, 48, False), (64, 528, True)])
@pytest.mark.parametrize("t", [0, 4])
def test_proj_temporal_attention_step(ops, dev, rows, C, p16, t):
    """Against fp64 F.linear + attention.  Bounds: the slot written by the batched GEMM is a split-bf16 GEMM output, TOL3.  The heads:
    the step kernel on exact inputs is within TOLA; q, k_t and v_t each carry a relative error <= TOL3, and with scores of order one
    (inputs scaled accordingly) the softmax and the convex combination of value rows pass each of them on with a factor <= 1, so
    TOLA + 3 * TOL3 to first order."""
    nh, Tcap = 8, 6
    xq, xv = rn((rows, C), 710), rn((rows, C), 711)
    w, b = rn((3 * C, C), 712, C ** -0.5), rn((3 * C,), 713, 0.1)
    kc, vc = rn((Tcap, rows, C), 714, 0.5), rn((Tcap, rows, C), 715)
    Ws, bs = [w[:C], w[C:2 * C], w[2 * C:]], [b[:C], b[C:2 * C], b[2 * C:]]
    qr = F.linear(xq.double(), Ws[0].double(), bs[0].double()) * float(C // nh) ** -0.5
    kr = F.linear(xq.double(), Ws[1].double(), bs[1].double())
    vr = F.linear(xv.double(), Ws[2].double(), bs[2].double())
    kref, vref = kc.double().clone(), vc.double().clone()
    kref[t], vref[t] = kr, vr
    ref = step_ref(qr, kref, vref, t + 1, nh)
    wd, bd = w.to(dev), b.to(dev)
    kd, vd = kc.to(dev), vc.to(dev)
    xqd, xvd = xq.to(dev), xv.to(dev)
    if p16:
        xqd, xvd = ops.to_p16(xqd), ops.to_p16(xvd)
    with torch.no_grad():
        o = ops.proj_temporal_attention_step(xqd, xvd, wd[:C], bd[:C], wd[C:2 * C], bd[C:2 * C], wd[2 * C:], bd[2 * C:], kd, vd, t, nh,
                                             x_p16=p16, o_p16=p16)
    got = ops.p16_decode(o) if p16 else o
    ek, ev, eo = rel(kd[t], kr), rel(vd[t], vr), rel(got, ref)
    print("proj step rows %d C %d t %d: k %.3e v %.3e o %.3e" % (rows, C, t, ek, ev, eo))
    assert ek < TOL3 and ev < TOL3
    assert eo < TOLA + 3 * TOL3
    others = [j for j in range(Tcap) if j != t]
    assert torch.equal(kd[others].cpu().view(torch.int32), kc[others].view(torch.int32))     # bit-unchanged
    assert torch.equal(vd[others].cpu().view(torch.int32), vc[others].view(torch.int32))


def test_proj_temporal_attention_step_is_no_grad_only(ops, dev):
    C, rows = 48, 8
    x = torch.zeros((rows, C), device=dev, requires_grad=True)
    w, b = torch.zeros((3 * C, C), device=dev), torch.zeros((3 * C,), device=dev)
    kc = torch.zeros((2, rows, C), device=dev)
    with pytest.raises(RuntimeError):
        ops.proj_temporal_attention_step(x, x, w[:C], b[:C], w[C:2 * C], b[C:2 * C], w[2 * C:], b[2 * C:], kc, kc.clone(), 0, 8)


# ------------------------------------------------------------------------------------------------------ 4. the model
CFG6 = dict(Tp=3, Tf=3, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=2, rpe=True)
CFG20 = dict(Tp=2, Tf=18, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=1, rpe=True)   # 20 frames: more than 16 keys


@pytest.fixture(scope="module")
def far_cases(pkg):
    """model, parameters, features and the oracle's single full pass per config -- computed once, read-only"""
    out = {}
    for name, cfg, N, seed in (("six", CFG6, 2, 730), ("twenty", CFG20, 1, 740)):
        m = build_transformer(pkg, cfg, True)
        fill.apply_fill(m, seed)
        P = {k: v.detach().clone() for k, v in m.state_dict().items()}
        T = cfg["Tp"] + cfg["Tf"]
        feat = fill.rand_normal((N, T, cfg["C"], cfg["H"], cfg["W"]), seed + 1).abs()       # encoder features are post-ReLU
        out[name] = (m.to("cuda:0").eval(), P, feat, O.far_forward(P, feat, cfg), cfg)
    return out


@pytest.mark.parametrize("name,prefill", [("six", 0), ("six", 3), ("twenty", 0), ("twenty", 3)])
def test_forward_cached_matches_full_pass(far_cases, dev, name, prefill):
    """teacher-forced: a fixed feature sequence fed one frame at a time (prefill = 0), or a 3-frame prefill and then single frames,
    against the oracle's ONE causal pass over the whole sequence"""
    m, P, feat, ref, cfg = far_cases[name]
    T = feat.shape[1]
    fd = feat.to(dev)
    cache = m.init_cache(feat.shape[0])
    outs = []
    if prefill:
        outs.append(m.forward_cached(fd[:, :prefill], cache))
    for t in range(prefill, T):
        outs.append(m.forward_cached(fd[:, t:t + 1], cache))
        assert cache.len == t + 1
    got = torch.cat(outs, dim=1)
    assert got.shape == tuple(ref.shape)
    err = rel(got, ref)
    print("forward_cached %s prefill %d: rel %.3e" % (name, prefill, err))
    assert err < TOL


def test_forward_cached_every_frame_vs_prefix_pass(far_cases, dev):
    """frame t of the cached path against the last frame of the oracle's pass over frames 0 .. t"""
    m, P, feat, _, cfg = far_cases["six"]
    fd = feat.to(dev)
    cache = m.init_cache(feat.shape[0])
    for t in range(feat.shape[1]):
        got = m.forward_cached(fd[:, t:t + 1], cache)
        ref = O.far_forward(P, feat[:, :t + 1], cfg)[:, -1:]
        err = rel(got, ref)
        print("frame %d: rel %.3e" % (t, err))
        assert err < TOL


# ------------------------------------------------------------------------------------------------------ 5. rollouts
def test_cached_train_rollout_matches_oracle(pkg, dev):
    """far_rollout(kv_cache=True), mode 'train', against the oracle loop of test_02::test_rollouts_match_oracle (same config, seeds)"""
    from vptr_amd.inference import far_rollout
    feat, HW, N = 48, 64, 2
    enc = pkg.VPTREnc(1, feat, 3, "reflect").eval()
    dec = pkg.VPTRDec(1, feat, 3, "Sigmoid", "reflect").eval()
    fill.apply_fill(enc, 71)
    fill.apply_fill(dec, 72)
    Pe, Pd = dict(enc.state_dict()), dict(dec.state_dict())
    cfgf = dict(Tp=3, Tf=3, H=8, W=8, C=feat, nhead=8, window_size=4, num_encoder_layers=2, rpe=True)
    Tf_ = build_transformer(pkg, cfgf, True)
    fill.apply_fill(Tf_, 75)
    Pf = dict(Tf_.state_dict())
    past = fill.rand_input((N, 3, 1, HW, HW), 76)
    num_pred = 3
    pf = O.enc_forward(Pe, past)
    pred_feats = O.far_forward(Pf, pf, cfgf)
    inp = pf
    for i in range(num_pred - 1):
        if i == 0:
            inp = torch.cat([pf, pred_feats[:, -1:]], dim=1)
        else:
            inp = torch.cat([inp, O.enc_forward(Pe, O.dec_forward(Pd, pred_feats[:, -1:], out_layer="Sigmoid"))], dim=1)
        pred_feats = O.far_forward(Pf, inp, cfgf)
    frames = O.dec_forward(Pd, pred_feats, out_layer="Sigmoid")
    gp, gf = far_rollout(enc.to(dev), dec.to(dev), Tf_.to(dev), past.to(dev), num_pred, kv_cache=True)
    assert gf.shape == (N, num_pred, 1, HW, HW) and gp.shape == (N, 2, 1, HW, HW)
    ef, ep = rel(gf, frames[:, -num_pred:]), rel(gp, frames[:, :-num_pred])
    print("cached train rollout: future %.3e past %.3e" % (ef, ep))
    assert ef < TOL and ep < TOL


def test_cached_rip_ril_rollouts_match_reference_notebook(pkg, dev):
    """modes 'RIP' / 'RIL' with kv_cache=True against the tensors the reference's notebook functions returned (five predictions with
    horizon 3: cached while the window grows, the full recompute once it slides)"""
    from vptr_amd.inference import far_rollout
    z = load("rollouts_tiny")
    meta = jload(z, "meta")
    enc = pkg.VPTREnc(1, meta["feat"], 3, "reflect").eval()
    dec = pkg.VPTRDec(1, meta["feat"], 3, "Sigmoid", "reflect").eval()
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 1)
    enc, dec = enc.to(dev), dec.to(dev)
    far = build_transformer(pkg, jload(z, "cfg_far"), True)
    fill.apply_fill(far, meta["seed"] + 2)
    far = far.to(dev)
    past = torch.from_numpy(z["far_past"]).to(dev)
    n_pred = z["far_rip"].shape[1]
    assert n_pred > far.num_future_frames          # the window slides in this fixture
    for mode in ("RIP", "RIL"):
        got = far_rollout(enc, dec, far, past, n_pred, mode=mode, kv_cache=True)
        ref = z["far_rip" if mode == "RIP" else "far_ril"]
        assert got.shape == tuple(ref.shape)
        err = rel(got, ref)
        print("cached %s rollout: rel %.3e" % (mode, err))
        assert err < TOL, "FAR %s rollout: %.3e" % (mode, err)


# ------------------------------------------------------------------------------------------------------ 6. guards
def test_forward_cached_guards(far_cases, dev):
    m, P, feat, _, cfg = far_cases["six"]
    fd = feat.to(dev)
    N, T = feat.shape[:2]
    cache = m.init_cache(N)
    assert cache.len == 0 and len(cache.k) == cfg["num_encoder_layers"]
    assert tuple(cache.k[0].shape) == (T, N * cfg["H"] * cfg["W"], cfg["C"]) and cache.k[0].device.type == "cuda"
    m.forward_cached(fd, cache)                                  # fills the cache to its capacity
    assert cache.len == T
    with pytest.raises(ValueError):
        m.forward_cached(fd[:, :1], cache)                       # one frame past Tcap
    cache = m.init_cache(N)
    m.forward_cached(fd[:, :2], cache)
    with pytest.raises(ValueError):
        m.forward_cached(fd[:, 2:4], cache)                      # Tn > 1 into a non-empty cache
    with pytest.raises(ValueError):
        m.forward_cached(fd[:1, 2:3], cache)                     # batch-size mismatch
    assert cache.len == 2
    m.train()
    try:
        with pytest.raises(ValueError):
            m.forward_cached(fd[:, 2:3], cache)                  # training mode
    finally:
        m.eval()
