"""Shared test helpers (CPU + GPU)."""
import json
import os

import numpy as np
import torch

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


_current_test = [""]     # set per test by conftest.py; with VPTR_MARGIN_LOG every rel() value is logged under it (how far from the bar?)


def rel(a, b, floor=0.0):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    v = float((a - b).norm() / (b.norm() + floor + 1e-300))
    path = os.environ.get("VPTR_MARGIN_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"rel": v, "test": _current_test[0]}) + "\n")
    return v


def margin(name, value, bound):
    """bookkeeping for the noise-derived bounds of the self-comparison tests: with VPTR_MARGIN_LOG=<file> every checked (value, bound)
    pair is appended to the file, so a run over several boxes shows how far each assertion is from failing (profiles/r04_margins.log)"""
    path = os.environ.get("VPTR_MARGIN_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"check": name, "value": value, "bound": bound, "ratio": (value / bound) if bound else None}) + "\n")
    return value


def collect(q, procs, n, timeout=600):
    """n results from the workers' queue; a worker that died (a c10d watchdog abort, a segfault) fails the test at once instead of
    holding the GPU box until the queue timeout"""
    import queue
    import time
    out, t0 = [], time.time()
    while len(out) < n:
        try:
            out.append(q.get(timeout=5))
        except queue.Empty:
            dead = [p.exitcode for p in procs if not p.is_alive() and p.exitcode not in (0, None)]
            if dead:
                raise RuntimeError("worker process died with exit code(s) %s before reporting" % dead)
            if all(not p.is_alive() for p in procs) and q.empty():
                raise RuntimeError("workers exited without reporting")
            if time.time() - t0 > timeout:
                raise
    return out


def jload(z, key):
    return json.loads(str(z[key]))


def build_transformer(pkg, cfg, far, dropout=0.0):
    """pkg: a module exposing VPTRFormerNAR / VPTRFormerFAR (vptr_amd.model)."""
    if far:
        return pkg.VPTRFormerFAR(cfg["Tp"], cfg["Tf"], cfg["H"], cfg["W"], cfg["C"], cfg["nhead"], cfg["num_encoder_layers"],
                                 dropout, cfg["window_size"], 4, cfg["rpe"])
    return pkg.VPTRFormerNAR(cfg["Tp"], cfg["Tf"], cfg["H"], cfg["W"], cfg["C"], cfg["nhead"], cfg["num_encoder_layers"],
                             cfg["num_decoder_layers"], dropout, cfg["window_size"], 4, bool(cfg.get("TSLMA", False)), cfg["rpe"])


def grad_floor(norms):
    """Gradients that are analytically zero (biases in front of a train-mode BatchNorm, the k-bias of a softmax) are pure
    round-off; errors are measured against ||ref|| + 1e-2 * median gradient norm (same rule as oracle/make_golden.py)."""
    return 1e-2 * float(np.median(list(norms)))


ZERO_CLASS = 1e-4   # a gradient whose reference norm is below ZERO_CLASS x the median gradient norm of the model is ANALYTICALLY zero


# parameter names whose gradient is zero in exact arithmetic (the class is an explicit allow-list, the norm rule only confirms it)
# -- the bias of anything that only feeds a train-mode BatchNorm (NAR encoder blocks: norm2.bias in front of the conv-FFN's BN chain,
# SpatialFFN.fc1 / dw3x3 / fc2 bias), the k-bias of a softmax, and -- NAR decoder layer 0, whose input is the all-zero query tensor
# (VidHRFormer.py:45-47): every token of a window has the same value vector, so its attention weights (q_proj, k_proj, the relative position
# table) and the LayerNorm gain in front of them (x_hat = 0) cannot move the loss.
ZERO_NAME_PATTERNS = ("encoder.layers.*.norm2.bias", "encoder.layers.*.SpatialFFN.fc1.bias", "encoder.layers.*.SpatialFFN.dw3x3.bias",
                      "encoder.layers.*.SpatialFFN.fc2.bias", "*.k_proj.bias", "decoder.layers.0.SLMHSA.attn.q_proj.*",
                      "decoder.layers.0.SLMHSA.attn.k_proj.*", "decoder.layers.0.SLMHSA.attn.relative_position_bias_table",
                      "decoder.layers.0.norm1.weight")


def analytic_zero(ref_norm, norms, name=None):
    """True for gradients that are zero in exact arithmetic -- the bias of anything that feeds a train-mode BatchNorm only (the NAR
    encoder's `norm2.bias` and `SpatialFFN.fc1.bias`: BatchNorm subtracts the batch mean, a per-channel constant in front of it cannot
    move the loss), the k-bias of a softmax.  The reference's own value for such a tensor is its fp32 round-off (2e-6 of the median
    gradient norm at KTH128 N = 2), ours is the split-bf16 operand round-off (2^-17 per GEMM operand: 1.2e-5 of the median) summed over
    20 480 tokens whose true contributions cancel exactly.  A RELATIVE error between two noises means nothing; what parity can ask is
    that ours is zero by the same criterion that classes the reference's as zero: norm < ZERO_CLASS x median gradient norm (8x margin
    measured).  DESIGN.md section 3 lists this class in the tolerance table."""
    small = float(ref_norm) < ZERO_CLASS * float(np.median(list(norms)))
    if small and name is not None and float(ref_norm) > 0.0:   # (an EXACT zero of the reference -- a branch the fixture does not exercise -- needs no name)
        # a tensor with a small but REAL gradient must not slip into the zero class: only the known analytically-zero names may
        import fnmatch
        assert any(fnmatch.fnmatch(name, "*" + pat) for pat in ZERO_NAME_PATTERNS), \
            "%s: reference gradient norm %.3e classes as zero but the name is not in helpers.ZERO_NAME_PATTERNS" % (name, float(ref_norm))
    return small


def post_step_params_close(state_dict, z, rel_tol=1e-4, lr=1e-4, max_flip_frac=0.02):
    """Post-step parameters vs the `post:` arrays of a golden step record.  The first AdamW updates are ~lr * sign(g), so
    elements whose gradient is analytically zero move by +-lr on rounding noise alone (and atomics make that noise
    run-dependent): compare the concatenated parameters globally and bound the share of updates that differ by > lr/2."""
    num = den = 0.0
    bad = tot = 0
    worst = []
    for k in z.files:
        if not k.startswith("post:"):
            continue
        r = torch.from_numpy(z[k]).double()
        d = state_dict[k[5:]].detach().cpu().double() - r
        num += float((d * d).sum())
        den += float((r * r).sum())
        nb = int((d.abs() > 0.5 * lr).sum())
        bad += nb
        tot += d.numel()
        worst.append((nb / max(d.numel(), 1), nb, d.numel(), k[5:]))
    relerr = (num / den) ** 0.5
    assert relerr < rel_tol, relerr
    assert bad <= max_flip_frac * tot, (bad, tot, sorted(worst, reverse=True)[:12])
    return relerr


def sampled_post_params_close(state_dicts, z, lr, rel_tol, max_flip_frac=0.03):
    """as post_step_params_close, for fixtures that keep a strided sample (<= ~4096 elements) of every tensor under
    `post:<tag>:<name>`; state_dicts maps tag -> state_dict.  BatchNorm running statistics are buffers, not optimizer-updated
    parameters: they count in the rel-L2 figure but not among the "updates that differ by more than lr / 2" (a running variance of
    O(1) that agrees to 1e-4 relative is inside the parity bar and outside lr / 2)."""
    num = den = 0.0
    bad = tot = 0
    per = int(z["sample"]) if "sample" in z.files else 4096
    worst = []
    for k in z.files:
        if not k.startswith("post:"):
            continue
        _, tag, name = k.split(":", 2)
        flat = state_dicts[tag][name].detach().cpu().double().flatten()
        d = flat[::max(1, flat.numel() // per)] - torch.from_numpy(z[k]).double()
        num += float((d * d).sum())
        den += float((torch.from_numpy(z[k]).double() ** 2).sum())
        if "running_" in name:
            continue
        nb = int((d.abs() > 0.5 * lr).sum())
        bad += nb
        tot += d.numel()
        worst.append((nb / d.numel(), nb, d.numel(), "%s:%s" % (tag, name)))
    relerr = (num / den) ** 0.5
    assert relerr < rel_tol, relerr
    assert bad <= max_flip_frac * tot, (bad, tot, sorted(worst, reverse=True)[:12])
    return relerr


# ---- fp64 reference builders of the stage-1 op tests (tests/test_09_stage1_ops_gpu.py) and the TSLMA core test; each one is checked against an
# independent formulation on the CPU (tests/test_cpu.py) so that a wrong reference fails there, not on the GPU box
def unfold_kkc(x, KH, KW, stride, pad, pad_mode="zero"):
    """im2col of an NCHW tensor in the column order of vptr_im2col_nhwc: [(b, oy, ox), (ky, kx, c)].  F.unfold orders its columns (c, ky, kx);
    the padding is applied first (zeros or F.pad's reflection), so the patches are plain strided windows of the padded image."""
    import torch.nn.functional as F
    B, C = x.shape[:2]
    if pad:
        x = F.pad(x, (pad,) * 4, mode="reflect") if pad_mode == "reflect" else F.pad(x, (pad,) * 4)
    cols = F.unfold(x, (KH, KW), stride=stride)                              # [B, C * KH * KW, OH * OW]
    L = cols.shape[-1]
    return cols.reshape(B, C, KH, KW, L).permute(0, 4, 2, 3, 1).reshape(B * L, KH * KW * C)


def ts_rows(N, T, H, W, ws):
    """token rows of every (window, sequence element) of the temporal-spatial window attention: [N * (H/ws) * (W/ws), T * ws * ws] int64 with
    window b = (n, qh, qw), element s = (t, ph, pw) -> row ((n * T + t) * H + qh * ws + ph) * W + qw * ws + pw (H, W multiples of ws)"""
    n, qh, qw, t, ph, pw = torch.meshgrid(torch.arange(N), torch.arange(H // ws), torch.arange(W // ws), torch.arange(T), torch.arange(ws),
                                          torch.arange(ws), indexing="ij")
    rows = ((n * T + t) * H + qh * ws + ph) * W + qw * ws + pw
    return rows.reshape(N * (H // ws) * (W // ws), T * ws * ws)


def ts_gather(x, N, T, H, W, ws):
    """tokens [(n, t, h, w), C] -> [windows, T * ws * ws, C] (explicit gather by window)"""
    rows = ts_rows(N, T, H, W, ws)
    return x[rows.reshape(-1)].reshape(rows.shape[0], rows.shape[1], x.shape[-1])


def ts_scatter(xw, N, T, H, W, ws):
    """inverse of ts_gather: every token belongs to exactly one (window, element), so the scatter is a gather by the inverse permutation"""
    rows = ts_rows(N, T, H, W, ws).reshape(-1)
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(rows.numel())
    return xw.reshape(rows.numel(), xw.shape[-1])[inv]


def reflect_fold_ref(dxpad, pad):
    """adjoint of F.pad(mode="reflect"): dxpad [B, C, H + 2p, W + 2p] -> [B, C, H, W]; padded index q belongs to source |q - p| mirrored at
    n - 1, and every padded row / column is ADDED onto the source row / column it mirrors (one axis after the other)"""
    def fold(t, dim):
        n = t.shape[dim] - 2 * pad
        src = (torch.arange(n + 2 * pad) - pad).abs()
        src = torch.where(src > n - 1, 2 * (n - 1) - src, src)
        shape = list(t.shape)
        shape[dim] = n
        return torch.zeros(shape, dtype=t.dtype).index_add_(dim, src, t)
    return fold(fold(dxpad, 2), 3)


# ---- fp64 reference builders of the deferred-backward op tests (tests/test_09b_deferred_bwd_gpu.py); like the ones above, each is checked on the
# CPU against an independent closed-form formulation (tests/test_cpu.py)
def ln_bwd_ref(x, gamma, dy, dy2=None, dx_add=None, eps=1e-5):
    """backward of LayerNorm(C) as the trainers' backward node runs it (vptr_layernorm_bwd*): fp64 autograd of F.layer_norm on x [rows, C] with the
    upstream gradient dy + dy2 (dy2: the gradient of the position-added second output), dx_add (the residual gradient that passes through the
    node) added onto dx.  Returns fp64 dx [rows, C], dgamma, dbeta [C] and the row statistics mean, rstd [rows] of the fp32 x."""
    import torch.nn.functional as F
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros_like(gr).requires_grad_(True)
    g = dy.double() if dy2 is None else dy.double() + dy2.double()
    F.layer_norm(xr, (x.shape[1],), gr, br, eps).backward(g)
    xd = x.double()
    dx = xr.grad if dx_add is None else xr.grad + dx_add.double()
    return {"dx": dx, "dgamma": gr.grad, "dbeta": br.grad, "mean": xd.mean(1), "rstd": (xd.var(1, unbiased=False) + eps).rsqrt()}


KINK, KINK_CAP = 1e-3, 5e-3     # the kink rule of tests/test_09_stage1_ops_gpu.py


def norm_act_ln_bwd_ref(x, w, b, dy, frames, HW, act, mask=None, keep=1.0, rowscale=None, rs_div=1, rs_mod=1, eps=1e-5):
    """backward of y = act(LayerNorm((F,H,W))(x) * w + b) * mask / keep * rowscale[(row // rs_div) % rs_mod] (vptr_norm_act_bwd* with
    per_col = 0) by fp64 autograd.  x, dy, mask: channel-last [frames * HW, F]; w, b: the (F, H, W) affine in the kernels' layout [HW, F]
    -- a frame's HW x F block holds exactly the elements of its (F, H, W) tensor, so F.layer_norm over the trailing (HW, F) of the
    channel-last view is the same normalisation and the same elementwise affine.  act: 0 none, 1 GELU (erf form), 2 ReLU; for ReLU the
    upstream gradient is zeroed where |pre| < KINK * rms(pre) (the returned "dy" is what the kernel must be given, "kink_share" the zeroed
    share).  Returns fp64 dx [rows, F], dw, db [HW, F], the frame statistics mean, rstd [frames], the pre-activation and dy."""
    import torch.nn.functional as F
    rows, Fc = x.shape
    assert rows == frames * HW and tuple(w.shape) == (HW, Fc)
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.layer_norm(xr.view(frames, HW, Fc), (HW, Fc), wr, br, eps).reshape(rows, Fc)
    y = F.gelu(pre) if act == 1 else (torch.relu(pre) if act == 2 else pre)
    if mask is not None:
        y = y * mask.double() / keep
    if rowscale is not None:
        y = y * rowscale.double()[(torch.arange(rows) // rs_div) % rs_mod][:, None]
    g, share = dy.double(), 0.0
    if act == 2:
        near = pre.detach().abs() < KINK * pre.detach().pow(2).mean().sqrt()
        share = float(near.double().mean())
        g = torch.where(near, torch.zeros_like(g), g)
    y.backward(g)
    xf = x.double().view(frames, HW * Fc)
    return {"dx": xr.grad, "dw": wr.grad, "db": br.grad, "mean": xf.mean(1), "rstd": (xf.var(1, unbiased=False) + eps).rsqrt(),
            "pre": pre.detach(), "dy": g, "kink_share": share}


# (frames, HW, F) of the LayerNorm((F,H,W)) backward cases: id -> (deferred call?, frames, HW, F); what each one stresses is said where they run
NORM_ACT_LN_CASES = {
    "plain_13x12x20": (False, 13, 12, 20), "plain_70x16x32": (False, 70, 16, 32), "plain_67x64x256": (False, 67, 64, 256),
    "deferred_64x16x32": (True, 64, 16, 32), "deferred_70x16x32": (True, 70, 16, 32), "deferred_100x4x16": (True, 100, 4, 16),
    "deferred_66x64x1024": (True, 66, 64, 1024),
}


def norm_act_ln_inputs(case):
    """the seeded fp32 inputs of one NORM_ACT_LN_CASES entry: x, dy [rows, F], w, b [HW, F] and a DropPath-like row scale [frames] (0 or 1 / 0.8)"""
    _, frames, HW, Fc = NORM_ACT_LN_CASES[case]
    seed = 3000 + 10 * sorted(NORM_ACT_LN_CASES).index(case)
    x, dy = fill.rand_normal((frames * HW, Fc), seed, 2.0) + 0.3, fill.rand_normal((frames * HW, Fc), seed + 1)
    w, b = fill.rand_normal((HW, Fc), seed + 2).abs() + 0.5, fill.rand_normal((HW, Fc), seed + 3, 0.3)
    rowscale = (fill.rand_input((frames,), seed + 4) > 0.2).float() / 0.8
    return x, dy, w, b, rowscale


# ---- attention cores through the C ABI (tests/test_00b_attn_abi_gpu.py): kernel-family switch, fp64 reference builders, the plain-torch P16
# encoder and the head-class arithmetic of the launchers; each builder is checked against an independent formulation in tests/test_cpu.py
ATTN_MODES = ("default", "attn16", "attn16fwd", "mfma", "vector")


class attn_kernel_mode:
    """scope that routes every attention geometry to one kernel family (the launchers read the variables per call): "default" (problems of at
    most 16 tokens on the MFMA kernels of attn16.hip -- forward without LDS, backward of the second generation when C % 4 == 0; larger ones on the
    LDS-staged MFMA kernels of attn_mfma.hip), "attn16" = VPTR_ATTN16=2 (attn16.hip forward + its first-generation backward), "attn16fwd" =
    VPTR_ATTN16=4 (attn16.hip forward, fp32 vector backward), "mfma" = VPTR_ATTN_MFMA=2 (attn_mfma.hip wherever it covers the geometry) and
    "vector" = VPTR_ATTN_MFMA=0 (the fp32 vector kernels of attn.hip everywhere); the variables' earlier values come back on exit.  The table of
    the switches is in csrc/attn_route.h; attn_route below asks the library which family a call reaches"""

    def __init__(self, mode):
        assert mode in ATTN_MODES, mode
        self.mode = mode

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("VPTR_ATTN_MFMA", "VPTR_ATTN16")}
        os.environ.pop("VPTR_ATTN16", None)
        if self.mode in ("default", "attn16", "attn16fwd"):
            os.environ.pop("VPTR_ATTN_MFMA", None)
            if self.mode != "default":
                os.environ["VPTR_ATTN16"] = "2" if self.mode == "attn16" else "4"
        else:
            os.environ["VPTR_ATTN_MFMA"] = "2" if self.mode == "mfma" else "0"
        return self.mode

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def current_attn_mode():
    """name of the kernel-family routing the environment selects right now (the inverse of attn_kernel_mode)"""
    m, e = os.environ.get("VPTR_ATTN_MFMA"), os.environ.get("VPTR_ATTN16")
    if m is not None and int(m) != 1:
        return "mfma" if int(m) == 2 else "vector"
    return {None: "default", "1": "default", "2": "attn16", "4": "attn16fwd"}.get(e, "VPTR_ATTN16=%s" % e)


ATTN_FAMILIES = ("vector", "vector16", "a16_gen1", "a16_gen2", "am_plain", "am_shared")     # VPTR_ATTN_FAMILY_* of include/vptr_hip.h, in order


def attn_route(kind, Lq, Lk, C, nh, ws=0, causal=0, groups=1, backward=0, aligned16=1):
    """vptr_attn_route (host-side, no GPU) under the switches the environment holds right now: (family name, (a, b), variant)"""
    import ctypes
    from vptr_amd import _lib
    out = (ctypes.c_int * 4)(-1, -1, -1, -1)
    _lib.check(_lib.lib.vptr_attn_route(kind, Lq, Lk, C, nh, ws, int(causal), groups, int(backward), int(aligned16), out, 4), "vptr_attn_route")
    return ATTN_FAMILIES[out[0]], (out[1], out[2]), out[3]


def attn_geom_route(geom, nh, C, backward, aligned16=1):
    """attn_route of a geometry of tests/attn_abi_cases.py: ("win", B, H, W, ws, bias) or ("t", N, Tq, Tk, HW, causal)"""
    if geom[0] == "win":
        _, B, H, W, ws, _ = geom
        return attn_route(0, ws * ws, ws * ws, C, nh, ws, 0, B * (H // ws) * (W // ws), backward, aligned16)
    _, N, Tq, Tk, HW, causal = geom
    return attn_route(1, Tq, Tk, C, nh, 0, causal, N * HW, backward, aligned16)


# (N, Tq, Tk, H, W, ws, C, nh) of the TSLMA core tests: the K64 model's own geometry (head dim 66: 115 KB of dynamic LDS in the backward, 7 key
# groups that leave 50 of the 512 threads without dK / dV ownership, 23 of the 24 accumulators, clamped duplicate keys in the last group); a cross
# case with Tq != Tk on a non-square map with 2 x 3 windows per frame (head dim 6); Lq = 20 (not a multiple of the 16-query chunk); Lq = 12 < 16 at
# head dim 16; 6 heads of 8; Lk = 168 = TS_NACC * (512 / 66), the backward's key limit
TS_GEOMS = [(1, 10, 10, 8, 8, 4, 528, 8), (2, 3, 7, 4, 6, 2, 48, 8), (1, 5, 5, 4, 4, 2, 48, 8), (1, 3, 4, 6, 4, 2, 128, 8), (2, 2, 3, 4, 8, 4, 48, 6),
            (1, 2, 42, 2, 2, 2, 528, 8)]


def _attn_fwd(ins, gather, scatter, nh, bias=None, causal=False, mask=None):
    """differentiable fp64 forward: ins = (q, k, v[, table]); gather(t, which) -> [problems, L, C] (which: 0 query side, 1 key side), scatter its
    inverse for the query side; bias: callable on the table -> [nh, Lq, Lk]; mask [problems, nh, Lq, Lk] multiplies the probabilities"""
    from oracle import vptr_oracle as O
    qw, kw, vw = gather(ins[0], 0), gather(ins[1], 1), gather(ins[2], 1)
    b = bias(ins[3]) if bias is not None else None
    if mask is None:
        return scatter(O._attend(O._heads(qw, nh), O._heads(kw, nh), O._heads(vw, nh), b, causal))
    with O.dropout_masks({"core.probs": mask.double()}):
        return scatter(O._attend(O._heads(qw, nh), O._heads(kw, nh), O._heads(vw, nh), b, causal, drop_site="core.probs"))


def _attn_ref(ins, gather, scatter, go, nh, bias=None, causal=False, mask=None, dq_scale=1.0):
    """o = _attn_fwd(...) and the gradients of the leaves under the upstream gradient go, dq multiplied by dq_scale"""
    o = _attn_fwd(ins, gather, scatter, nh, bias, causal, mask)
    (o * go.double()).sum().backward()
    out = {"o": o.detach(), "dq": ins[0].grad * dq_scale, "dk": ins[1].grad, "dv": ins[2].grad}
    if bias is not None:
        out["dtable"] = ins[3].grad
    return out


def _win_maps(B, H, W, C, nh, ws, rel_index):
    from oracle import vptr_oracle as O
    L = ws * ws
    return (lambda t, _: O.win_partition(t.reshape(B, H, W, C), ws), lambda o: O.win_reverse(o, B, H, W, ws).reshape(B * H * W, C),
            None if rel_index is None else (lambda t: t[rel_index.reshape(-1)].reshape(L, L, nh).permute(2, 0, 1)))


def win_attn_fwd64(q, k, v, table, B, H, W, nh, ws, rel_index=None, mask=None):
    """the differentiable fp64 forward behind win_attn_ref (torch.autograd.gradcheck runs on it in tests/test_cpu.py)"""
    gather, scatter, bias = _win_maps(B, H, W, q.shape[1], nh, ws, rel_index if table is not None else None)
    return _attn_fwd((q, k, v) if table is None else (q, k, v, table), gather, scatter, nh, bias, False, mask)


def win_attn_ref(q, k, v, go, B, H, W, nh, ws, table=None, rel_index=None, mask=None, dq_scale=1.0):
    """fp64 local-window attention of vptr_winattn_fwd / _bwd: q (pre-scaled), k, v, go [B*H*W, C] token-major, table [(2ws-1)^2, nh] with
    rel_index [L, L] or None, mask [windows, nh, L, L] (0 or 1 / keep; windows in (b, wy, wx) order) or None.  Returns fp64 o, dq (the plain
    gradient times dq_scale), dk, dv [B*H*W, C] and, with a table, dtable."""
    ins = [t.double().clone().requires_grad_(True) for t in ((q, k, v) if table is None else (q, k, v, table))]
    gather, scatter, bias = _win_maps(B, H, W, q.shape[1], nh, ws, rel_index if table is not None else None)
    return _attn_ref(ins, gather, scatter, go, nh, bias, False, mask, dq_scale)


def temporal_attn_ref(q, k, v, go, N, Tq, Tk, HW, nh, causal=False, mask=None, dq_scale=1.0):
    """fp64 per-pixel temporal attention of vptr_tattn_fwd / _bwd: q, go [(n, tq, p), C], k, v [(n, tk, p), C]; mask [N * HW, nh, Tq, Tk] with the
    problems in (n, pixel) order"""
    C = q.shape[1]

    def seq(t, which):
        T = Tk if which else Tq
        return t.reshape(N, T, HW, C).permute(0, 2, 1, 3).reshape(N * HW, T, C)
    ins = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    return _attn_ref(ins, seq, lambda o: o.reshape(N, HW, Tq, C).permute(0, 2, 1, 3).reshape(N * Tq * HW, C), go, nh, None, causal, mask, dq_scale)


def ts_attn_ref(q, k, v, go, N, Tq, Tk, H, W, ws, nh, mask=None):
    """fp64 temporal-spatial window attention of vptr_tsattn_fwd / _bwd from the explicit gather by window (ts_gather); mask [windows, nh, Lq, Lk]"""
    ins = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    return _attn_ref(ins, lambda t, which: ts_gather(t, N, Tk if which else Tq, H, W, ws), lambda o: ts_scatter(o, N, Tq, H, W, ws), go, nh, None,
                     False, mask, 1.0)


def split_bf16(x):
    """the hi / lo split of the split-bf16 kernels (split2 of csrc/gemm_shared.h, the P16 format): hi = bf16_rne(x), lo = bf16_rne(x - hi), both bf16"""
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def p16_encode(x):
    """fp32 [rows, C] (C % 16 == 0) -> the P16 tensor of the same shape and dtype with plain torch ops: per 16-channel granule 16 bf16 hi
    (round to nearest even of x) followed by 16 bf16 lo = bf16(x - hi); the inverse of ops.core.p16_decode up to 2^-17 relative per element"""
    C = x.shape[-1]
    assert C % 16 == 0 and x.dtype == torch.float32
    hi, lo = split_bf16(x.contiguous().reshape(-1, C // 16, 16))
    return torch.stack([hi, lo], 2).reshape(-1).view(torch.float32).reshape(x.shape)


def attn_head_classes(hd, C_mod4_zero=True):
    """(plain, second-generation) instantiation classes (nb32, nb16) of an even head dim: the first-generation attn16 kernels and attn_mfma choose
    by (ceil(hd / 32), ceil(hd / 16)); the second-generation attn16 kernels by the same of the head's SPAN, hd + 2 when hd % 4 != 0 (a head
    that starts on an odd channel pair begins 2 channels early).  The launchers' if-chains map the pair onto the compiled instantiation."""
    def inst(n32, n16, gen2):
        if n32 == 1:
            return (1, 1) if n16 == 1 else (1, 2)
        if n32 == 2:
            return (2, 3) if n16 == 3 else (2, 4)
        if n16 == 5:
            return (3, 5)
        if n32 == 3 or not gen2:
            return (3, 6)
        return (4, 7)
    span = hd + (2 if hd % 4 else 0)
    return inst(-(-hd // 32), -(-hd // 16), False), inst(-(-span // 32), -(-span // 16), True)


# ---- the conv-FFN forward kernels through the C ABI (tests/test_09c_convffn_fwd_gpu.py): fp64 reference builders on channel-last rows, the
# launchers' selection arithmetic and an fp32 emulation of the one-pass variance; each is checked in tests/test_cpu.py
def _act64(pre, act):
    import torch.nn.functional as F
    return F.gelu(pre) if act == 1 else (torch.relu(pre) if act == 2 else pre)


def norm_act_fwd_ref(x, w, b, HW, per_col, act, mask=None, keep=1.0, rowscale=None, rs_div=1, rs_mod=1, residual=None, eps=1e-5):
    """fp64 y = rowscale[(row // rs_div) % rs_mod] * (mask / keep) * act(norm(x) * w + b) + residual of vptr_norm_act_fwd on channel-last
    x [rows, F].  per_col: BatchNorm2d batch statistics per column (biased variance), affine [F]; otherwise LayerNorm((F,H,W)) per frame of HW
    rows, affine [HW, F] (see norm_act_ln_bwd_ref).  mask [rows, F]: 0 / 1.  Returns y, the pre-activation and the statistics mean, rstd
    ([F] or [frames])."""
    rows, Fc = x.shape
    xd = x.double()
    if per_col:
        mean, var = xd.mean(0), xd.var(0, unbiased=False)
        rstd = (var + eps).rsqrt()
        pre = (xd - mean) * rstd * w.double() + b.double()
    else:
        frames = rows // HW
        assert rows == frames * HW and tuple(w.shape) == (HW, Fc)
        xf = xd.view(frames, HW * Fc)
        mean = xf.mean(1)
        rstd = (xf.var(1, unbiased=False) + eps).rsqrt()
        pre = (((xf - mean[:, None]) * rstd[:, None]).view(frames, HW, Fc) * w.double() + b.double()).reshape(rows, Fc)
    y = _act64(pre, act)
    if mask is not None:
        y = y * mask.double() / keep
    if rowscale is not None:
        y = y * rowscale.double()[(torch.arange(rows) // rs_div) % rs_mod][:, None]
    if residual is not None:
        y = y + residual.double()
    return {"y": y, "pre": pre, "mean": mean, "rstd": rstd}


def dwconv3x3_fwd_ref(a, w9, b9, frames, H, W):
    """fp64 depthwise 3x3 (padding 1) of channel-last a [frames * H * W, F] with the tap-major weights w9 [9, F] (tap = ky * 3 + kx) by
    F.conv2d(groups = F); returns channel-last rows"""
    import torch.nn.functional as F
    Fc = a.shape[1]
    a4 = a.double().reshape(frames, H, W, Fc).permute(0, 3, 1, 2)
    y = F.conv2d(a4, w9.double().t().reshape(Fc, 1, 3, 3), None if b9 is None else b9.double(), padding=1, groups=Fc)
    return y.permute(0, 2, 3, 1).reshape(frames * H * W, Fc)


def dwconv_norm_fwd_ref(x, aw, ab, w9, b9, frames, H, W, act, eps=1e-5):
    """fp64 reference of vptr_dwconv3x3_norm_fwd: a = act(LayerNorm((F,H,W))(x) * aw + ab) (aw, ab channel-last [H * W, F]), y = dw3x3(a) + b9.
    Returns y, a [rows, F], the frame statistics mean, rstd [frames] and the per-frame sum / sum of squares of y (what frame_stats receives)."""
    n = norm_act_fwd_ref(x, aw, ab, H * W, False, act, eps=eps)
    y = dwconv3x3_fwd_ref(n["y"], w9, b9, frames, H, W)
    yf = y.view(frames, -1)
    return {"y": y, "a": n["y"], "mean": n["mean"], "rstd": n["rstd"], "sum": yf.sum(1), "sumsq": (yf * yf).sum(1)}


def convffn_fwd_class(op, **g):
    """the launch class of a conv-FFN forward call, restated from the launchers (csrc/norm_act.hip, csrc/dwconv.hip):
    op "norm_act" (rows, F, HW, per_col, raw): kernel "col" (norm_act_fwd_kernel<true>), "row" (<false>) or "pos" (norm_act_fwd_pos_kernel), its
        grid, the float4 count, the trips of the longest grid-stride / frame loop and whether the large-mean recompute is armed;
    op "dwconv" (frames, H, W, F, stats): "fwd" / "fwd2" / "fwd3", or "reject";
    op "dwconv_norm" (frames, H, W, F): "lds" / "reg" (with the slab's dynamic LDS bytes), or "reject"."""
    cdiv = lambda a, b: (a + b - 1) // b
    if op == "norm_act":
        rows, Fc, HW, per_col, raw = g["rows"], g["F"], g["HW"], g["per_col"], g.get("raw", False)
        if Fc % 4 or rows <= 0 or HW < 1 or (not per_col and rows % HW) or (raw and per_col):
            return {"kernel": "reject"}
        total, blocks = rows * (Fc // 4), min(cdiv(rows * (Fc // 4), 256), 8192)
        if per_col:
            return {"kernel": "col", "grid": (blocks, 1), "float4": total, "trips": cdiv(total, blocks * 256), "armed": False}
        frames, P = rows // HW, HW * (Fc // 4)
        if frames >= 16 and total >= 1 << 18:
            gy = min(max(frames // 4, 1), 65535)
            return {"kernel": "pos", "grid": (cdiv(P, 256), gy), "float4": total, "trips": cdiv(frames, gy), "armed": bool(raw and P % 256 == 0)}
        return {"kernel": "row", "grid": (blocks, 1), "float4": total, "trips": cdiv(total, blocks * 256),
                "armed": bool(raw and P % 256 == 0 and total % 256 == 0)}
    frames, H, W, Fc = g["frames"], g["H"], g["W"], g["F"]
    if min(frames, H, W, Fc) <= 0 or Fc % 4:
        return {"kernel": "reject"}
    F4, W2 = Fc // 4, W // 2
    if op == "dwconv":
        stats = g.get("stats", False)
        if stats and (W % 2 or (W2 * F4) % 64):
            return {"kernel": "reject"}
        if W % 2 or (not stats and frames * W * F4 < 1 << 16):
            return {"kernel": "fwd"}
        return {"kernel": "fwd3" if 16 % W2 == 0 else "fwd2"}
    assert op == "dwconv_norm", op
    if W % 2 or W2 < 1 or 16 % W2 or (W2 * F4) % 64:
        return {"kernel": "reject"}
    if Fc % 64 == 0 and H * W <= 256 and frames <= 65535:
        return {"kernel": "lds", "lds_bytes": H * W * 256, "grid": (Fc // 64, frames)}
    return {"kernel": "reg", "grid": (cdiv(frames * W2 * F4, 256), 1)}


VAR_GUARD = 1e-2      # the kernels redo the variance around the mean when var < VAR_GUARD * E[x^2]: |mean| > sqrt(1 / VAR_GUARD - 1) = 9.95 std


def onepass_norm_emulation(x, guard, eps=1e-5):
    """fp32 emulation of the frame normalisation from IDEAL producer sums (the fp64 sum and sum of squares of the frame rounded once to fp32):
    mean = S / n, var = E[x^2] - mean^2 in fp32 as the four kernels compute them; when var < guard * E[x^2] the variance is redone around that
    mean (again with ideal sums of the fp32 differences) and the mean corrected.  x: one frame (fp32, any shape).  Returns (rel-L2 of the
    fp32 (x - mean) * rstd against fp64, recompute taken?)."""
    f32 = np.float32
    xv = x.detach().reshape(-1).numpy().astype(f32)
    x64 = xv.astype(np.float64)
    inv_n = f32(1.0) / f32(xv.size)
    m = f32(x64.sum()) * inv_n
    e2 = f32((x64 * x64).sum()) * inv_n
    var = np.maximum(e2 - m * m, f32(0.0))
    redo = bool(var < f32(guard) * e2)
    if redo:
        d = (xv - m).astype(np.float64)               # fp32 differences: exact inputs of the second pass
        dm = f32(d.sum()) * inv_n
        var = np.maximum(f32((d * d).sum()) * inv_n - dm * dm, f32(0.0))
        m = m + dm
    r = f32(1.0) / np.sqrt(var + f32(eps), dtype=f32)
    got = ((xv - m) * r).astype(np.float64)
    want = (x64 - x64.mean()) / np.sqrt(x64.var() + eps)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want)), redo


# ---- the tail of the train step through the C ABI (tests/test_09d_step_tail_gpu.py): fp64 reference builders of the fused losses and of
# clip + AdamW, an integer emulation of the counter-based RNG of csrc/common.h, an fp32 emulation of the AdamW update and the launchers'
# arithmetic restated; each is checked in tests/test_cpu.py
def mse_gdl_ref(pred, gt, g_mse, g_gdl):
    """fp64 MSELoss + GDL(alpha = 1) of pred, gt [planes, H, W] by the oracle's mse_loss / gdl_loss and autograd of g_mse * mse + g_gdl * gdl
    (None = 0).  Returns mse, gdl (floats) and dpred [planes, H, W]."""
    from oracle import vptr_oracle as O
    pr = pred.double().unsqueeze(1).clone().requires_grad_(True)
    gd = gt.double().unsqueeze(1)
    lm, lg = O.mse_loss(gd, pr), O.gdl_loss(gd, pr)
    (float(g_mse or 0.0) * lm + float(g_gdl or 0.0) * lg).backward()
    return {"mse": float(lm.detach()), "gdl": float(lg.detach()), "dpred": pr.grad.squeeze(1)}


def gdl_sign_disagreements(pred, gt):
    """how many sign arguments of the GDL gradient (|gd| - |pd| and pd of every vertical and horizontal pair) have another sign evaluated in
    fp32 than in fp64: the gradient is a sum of signs, so only inputs for which this is 0 let every element be compared"""
    def args(p, g):
        pdh, gdh = p[:, 1:, :] - p[:, :-1, :], g[:, 1:, :] - g[:, :-1, :]
        pdw, gdw = p[:, :, :-1] - p[:, :, 1:], g[:, :, :-1] - g[:, :, 1:]
        return [gdh.abs() - pdh.abs(), pdh, gdw.abs() - pdw.abs(), pdw]
    return sum(int((torch.sign(a) != torch.sign(b).float()).sum()) for a, b in zip(args(pred.float(), gt.float()), args(pred.double(), gt.double())))


def nce_ref(g, p, frames, L, tau, gout):
    """fp64 reference of vptr_nce_fwd / _bwd on token-major g, p [frames * L, C]: F.normalize(p = 2, dim = channel) + the oracle's bipatch_nce
    (the frame's L tokens as an L x 1 patch grid), autograd of gout * loss.  Returns loss, dg, dp and the scratch sections the forward leaves:
    inv [2 R] (1 / max(|x|, 1e-12), rows of g first), S [frames, L, L] (scores / tau), rlse, clse [frames, L] (log-sum-exp of rows / columns)."""
    import torch.nn.functional as F
    from oracle import vptr_oracle as O
    C = g.shape[1]
    gd, pd = g.double().clone().requires_grad_(True), p.double().clone().requires_grad_(True)

    def as5(t):
        return t.reshape(1, frames, L, 1, C).permute(0, 1, 4, 2, 3)
    loss = O.bipatch_nce(F.normalize(as5(gd), p=2.0, dim=2), F.normalize(as5(pd), p=2.0, dim=2), tau)
    (float(gout) * loss).backward()
    with torch.no_grad():
        inv = 1.0 / torch.cat([gd.norm(dim=1), pd.norm(dim=1)]).clamp_min(1e-12)
        gh, ph = (gd * inv[:frames * L, None]).view(frames, L, C), (pd * inv[frames * L:, None]).view(frames, L, C)
        S = gh @ ph.transpose(1, 2) / tau
    return {"loss": float(loss.detach()), "dg": gd.grad, "dp": pd.grad, "inv": inv, "S": S, "rlse": torch.logsumexp(S, 2), "clse": torch.logsumexp(S, 1)}


def f32(x):
    """the value a float argument of the C ABI has on the other side"""
    return float(np.float32(x))


def adamw_ref(p, g, m, v, step, lr, b1, b2, eps, wd, sumsq=None, max_norm=1.0, grad_scale=1.0, abi_hyper=True):
    """one step of torch.optim.AdamW (decoupled decay, bias correction) with clip_grad_norm_ folded in, evaluated in fp64 on the fp32 state:
    g' = g * grad_scale; with sumsq (the sum of squares of the UNSCALED gradients, as vptr_sumsq leaves it) g' *= min(1, max_norm /
    (|g'| + 1e-6)); then torch's formulas.  abi_hyper: the hyper-parameters rounded to fp32 as vptr_adamw receives them (otherwise the
    doubles torch.optim.AdamW itself works with).  Returns fp64 p, m, v."""
    h = f32 if abi_hyper else float
    lr, b1, b2, eps, wd, max_norm, grad_scale = (h(x) for x in (lr, b1, b2, eps, wd, max_norm, grad_scale))
    gd = g.double() * grad_scale
    if sumsq is not None:
        gd = gd * min(1.0, max_norm / (float(sumsq) ** 0.5 * grad_scale + 1e-6))
    pd = p.double() * (1.0 - lr * wd)
    md = b1 * m.double() + (1.0 - b1) * gd
    vd = b2 * v.double() + (1.0 - b2) * gd * gd
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    pd = pd - (lr / bc1) * md / (vd.sqrt() / bc2 ** 0.5 + eps)
    return pd, md, vd


def adamw_f32_emulation(p, g, m, v, step, lr, b1, b2, eps, wd, coef=1.0):
    """the formula of adamw_kernel in fp32 (numpy, one rounding per operation; coef: the clip coefficient times grad_scale the raw gradient is
    multiplied by), with bias corrections free of cancellation: 1 - b^k = -expm1(k log1p(b - 1)).  What a correct fp32 evaluation of the
    update is expected to reach against adamw_ref."""
    F = np.float32
    lr, b1, b2, eps, wd, k = (F(x) for x in (lr, b1, b2, eps, wd, step))
    pi, gi, mi, vi = (t.detach().numpy().astype(F) for t in (p, g, m, v))
    gi = gi * F(coef)
    bc1, bc2 = -np.expm1(k * np.log1p(b1 - F(1))), -np.expm1(k * np.log1p(b2 - F(1)))
    assert bc1.dtype == F and bc2.dtype == F
    pi = pi * (F(1) - lr * wd)
    mi = b1 * mi + (F(1) - b1) * gi
    vi = b2 * vi + ((F(1) - b2) * gi) * gi
    denom = np.sqrt(vi) * (F(1) / np.sqrt(bc2)) + eps
    pi = pi - (lr / bc1) * mi / denom
    assert pi.dtype == F and mi.dtype == F and vi.dtype == F
    return torch.from_numpy(pi), torch.from_numpy(mi), torch.from_numpy(vi)


M32 = 0xFFFFFFFF


def _mul32(x, c):
    """(x * c) mod 2^32 for 0 <= x, c < 2^32 on Python ints or int64 tensors without leaving 63 bits"""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & M32


def mix32_emu(x):
    """vptr_mix32 (csrc/common.h)"""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def hash3_emu(seed, site, idx):
    """vptr_hash3 (csrc/common.h): seed a Python int read as uint64, site a Python int read as uint32, idx an int64 tensor of element indices
    below 2^63.  Returns the 32-bit words as an int64 tensor."""
    seed, site = int(seed) & 0xFFFFFFFFFFFFFFFF, int(site) & M32
    key = mix32_emu((seed & M32) ^ mix32_emu(((seed >> 32) + _mul32((site + 1) & M32, 0x9E3779B9)) & M32))
    idx = torch.as_tensor(idx, dtype=torch.int64)
    return mix32_emu((((idx & M32) ^ key) + _mul32(idx >> 32, 0xC2B2AE35)) & M32)


def drop_scale_emu(seed, site, idx, p):
    """vptr_drop_scale: fp32 1 / (1 - p) where the element's word reaches the threshold uint32(p * 2^32), else 0 (p as the ABI's float)"""
    pf = np.float32(p)
    thr = int(float(pf) * 4294967296.0)
    keep = float(np.float32(1.0) / (np.float32(1.0) - pf))
    return torch.where(hash3_emu(seed, site, idx) >= thr, keep, 0.0).float()


def droppath_emu(keep, maxcount, seed, site0):
    """vptr_droppath_scales: out[r][k] = floor(keep[r] + u) / keep[r] in fp32 with u = (hash3(seed, site0 + r, k) >> 8) / 2^24"""
    out = []
    for r, kp in enumerate(keep.float().tolist()):
        u = (hash3_emu(seed, int(site0) + r, torch.arange(maxcount)) >> 8).float() * (1.0 / 16777216.0)
        kt = torch.tensor(kp, dtype=torch.float32)
        out.append(torch.floor(kt + u) / kt)
    return torch.stack(out)


def step_tail_class(op, **g):
    """the launch class of a call of the step's tail, restated from the launchers (csrc/losses.hip, csrc/optim.hip):
    "mse_gdl" (planes, H, W): bands of 16 rows, partials = workgroups of the forward, rows of the last band, trips of a workgroup's element loop
        and of the final kernel's loop over the partials, workgroups of the backward, scratch floats;
    "nce" (frames, L, C): NV instantiation of the backward (or "reject"), its dynamic LDS bytes and grid, 64-row blocks, dead rows of the last
        one, 16-token chunks and whether the last is partial, trips of the final kernel, whether the scores' channel guard is live, scratch floats;
    "sumsq" (n, aligned): workgroups, unrolled trips, full single-float4 trips, threads of a partial trip, scalar tail (all-scalar trips if not
        aligned);
    "adamw" (n, aligned): workgroups, float4 trips, scalar-tail elements (or the trips of the all-scalar path)."""
    cdiv = lambda a, b: (a + b - 1) // b
    if op == "mse_gdl":
        planes, H, W = g["planes"], g["H"], g["W"]
        if planes <= 0 or H < 2 or W < 2:
            return {"kernel": "reject"}
        bands = cdiv(H, 16)
        return {"bands": bands, "partials": planes * bands, "last_band_rows": H - 16 * (bands - 1), "band_trips": cdiv(min(H, 16) * W, 256),
                "final_trips": cdiv(planes * bands, 256), "bwd_blocks": cdiv(planes * H * W, 256), "scratch": planes * bands * 3}
    if op == "nce":
        frames, L, C = g["frames"], g["L"], g["C"]
        R, nb, C4 = frames * L, cdiv(L, 64), cdiv(C, 4)
        out = {"nb": nb, "dead_rows": nb * 64 - L, "chunks": cdiv(L, 16), "partial_chunk": L % 16 != 0, "final_trips": cdiv(frames, 256),
               "channel_guard": C % 16 != 0, "scratch": R * (4 + L) + frames, "fwd_grid": frames * nb * nb}
        if C > 640 or C % 4:
            out["nv"] = "reject"
            return out
        out["nv"] = 4 if C4 <= 16 else (16 if C4 <= 64 else (34 if C4 <= 136 else 40))
        out["lds_bytes"], out["bwd_grid"] = (64 * 17 + 16 * C4 * 4) * 4, frames * nb * 2
        return out
    n, aligned = g["n"], g.get("aligned", True)
    if op == "sumsq":
        blocks = min(cdiv(n, 1024), 256)                # workgroups of 1024 threads
        stride, n4 = blocks * 1024, n // 4
        if not aligned:
            return {"blocks": blocks, "scalar_trips": cdiv(n, stride)}
        unrolled = 0                                   # thread 0 of workgroup 0 takes the most trips of every loop
        while unrolled * 4 * stride + 3 * stride < n4:
            unrolled += 1
        rest = n4 - unrolled * 4 * stride              # float4 left to the single loop: `rest // stride` full trips, then `rest % stride` threads
        return {"blocks": blocks, "unrolled": unrolled, "singles": max(rest, 0) // stride, "partial_threads": max(rest, 0) % stride, "tail": n - 4 * n4}
    assert op == "adamw", op
    blocks = min((n // 4 + 255) // 256 + 1, 4096)
    stride = blocks * 256
    if not aligned:
        return {"blocks": blocks, "vec_trips": 0, "scalar_trips": cdiv(n, stride), "tail": n}
    return {"blocks": blocks, "vec_trips": cdiv(n // 4, stride), "scalar_trips": 1 if n % 4 else 0, "tail": n % 4}


def nce_f32_emulation(g, p, frames, L, tau, gout):
    """vptr_nce_fwd / _bwd in torch fp32 in the kernels' operation order (inverse norms, scores scaled by both and by 1 / tau and STORED in fp32,
    fp32 log-sum-exps, per-frame fp32 loss partials added in double; coefficients exp(S - lse) with the diagonal's second term, the fp32
    matrix product against the normalised other tokens, the normalisation's backward) with libm's exp / log.  What fp32 storage and
    arithmetic alone cost against nce_ref (most where the softmax is saturated -- a small loss at a small temperature -- and lse - S cancels):
    tests/test_cpu.py asserts that this stays inside the bars of every case, i.e. that they are reachable in fp32.  Returns loss (float), dg, dp."""
    F = torch.float32
    C, R = g.shape[1], frames * L
    g, p = g.to(F), p.to(F)
    inv_tau, go = torch.tensor(1.0, dtype=F) / torch.tensor(tau, dtype=F), torch.tensor(gout, dtype=F)
    inv_g = 1.0 / (g * g).sum(1).sqrt().clamp_min(1e-12)
    inv_p = 1.0 / (p * p).sum(1).sqrt().clamp_min(1e-12)
    S = torch.einsum("fic,fjc->fij", g.view(frames, L, C), p.view(frames, L, C)) * (inv_g.view(frames, L, 1) * inv_tau) * inv_p.view(frames, 1, L)
    rlse, clse = torch.logsumexp(S, 2), torch.logsumexp(S, 1)
    diag = torch.diagonal(S, dim1=1, dim2=2)
    loss = float(((rlse - 2.0 * diag).sum(1) + clse.sum(1)).double().sum() * 0.5 / R)
    cmean, eye = torch.tensor(0.5, dtype=F) / R, torch.eye(L, dtype=F)
    Mg = (torch.exp(S - rlse[:, :, None]) + eye * (torch.exp(S - clse[:, None, :]) - 2.0)) * cmean                     # [f, g token, p token]
    Mp = (torch.exp(S - clse[:, None, :]) + eye * (torch.exp(S - rlse[:, :, None]) - 2.0)).transpose(1, 2) * cmean     # [f, p token, g token]
    gh, ph = (g * inv_g[:, None]).view(frames, L, C), (p * inv_p[:, None]).view(frames, L, C)
    out = []
    for M, Y, x, iv in ((Mg, ph, g, inv_g), (Mp, gh, p, inv_p)):
        acc = (M @ Y).reshape(R, C) * (go * inv_tau)
        dot = (x * acc).sum(1) * iv
        dot = torch.where(iv >= 1e12, torch.zeros_like(dot), dot)
        out.append((acc - x * (iv * dot)[:, None]) * iv[:, None])
    assert out[0].dtype == F and S.dtype == F
    return loss, out[0], out[1]


# ---- the nt P16 GEMM through the C ABI (tests/test_01b_gemm_p16_abi_gpu.py): the launcher's conditions restated
def gemm_p16_class(fields, cus):
    """the launch class of a vptr_gemm call with P16 operands, restated from vptr_gemm_p16_launch and from the run-time choice of the EPI 0
    instantiations (csrc/gemm_p16.hip).  fields: vptr_gemm_desc members by name, pointers as integer addresses (0 / missing = NULL), everything
    missing = 0; cus: the device's compute units.  Returns (EPI, NST, epilogue) with epilogue "batched" (gemm_epilogue_rows_halves_batched),
    "rows_halves" or "serial", or ("refuse", k) with k the launcher's VPTR_CHECK that refuses the descriptor, counted from 1 in source order."""
    f = lambda k: fields.get(k, 0) or 0

    def bits(*ks):
        v = 0
        for k in ks:
            v |= int(f(k))
        return v
    if not (f("a_mode") == 5 and f("b_mode") == 3):
        return ("refuse", 1)
    if f("K") % 16 or f("lda") % 16 or f("ldb") % 16:
        return ("refuse", 2)
    if not (f("split_k") <= 1 and f("precision") == 3 and not f("a_rowsum") and not f("D_planes")):
        return ("refuse", 3)
    batch, ksegs = max(f("batch"), 1), max(f("ksegs"), 1)
    sa, sb, sd = f("batch_stride_a"), f("batch_stride_b"), f("batch_stride_d")
    strided = sd != 0
    if strided and not (ksegs == 1 and batch <= 4096 and not any(f(k) for k in ("Dpre", "residual", "atomic", "batch_accum", "frame_stats", "act_grad_src",
                                                                                "rowscale", "colscale", "act", "act_after")) and f("dropout_p") == 0
                        and ((sa | sb | sd) & 15) == 0 and sa >= 0 and sb >= 0 and sd > 0):
        return ("refuse", 4)
    if not ((strided or batch <= 3) and ksegs <= 3 and (batch == 1 or ksegs == 1)):
        return ("refuse", 5)
    extra = 0 if strided else (batch if batch > 1 else ksegs) - 1
    opb = bits("A", "B")
    if extra >= 1:
        if not (f("A_x1") and f("B_x1")):
            return ("refuse", 6)
        opb |= bits("A_x1", "B_x1")
    if extra >= 2:
        if not (f("A_x2") and f("B_x2")):
            return ("refuse", 7)
        opb |= bits("A_x2", "B_x2")
    if opb & 63:
        return ("refuse", 8)
    members = batch > 1 and not strided
    if members and not (f("D_x1") and (batch < 3 or f("D_x2")) and not f("Dpre") and not f("residual") and not f("atomic")):
        return ("refuse", 9)
    if f("rowscale") and not (f("rs_div") >= 1 and f("rs_mod") >= 1):
        return ("refuse", 10)
    p = f("dropout_p")
    if p > 0 and not (f("seed_dev") and p < 1):
        return ("refuse", 11)
    N, ldd, ldr = f("N"), f("ldd"), f("ldr")
    if f("d_p16") and not (not f("atomic") and N % 16 == 0 and ldd % 16 == 0 and ldr % 4 == 0 and (bits("D", "D_x1", "D_x2") & 63) == 0
                           and (bits("residual", "bias", "colscale", "Dpre", "bias_x1", "bias_x2") & 15) == 0):
        return ("refuse", 12)
    tiles = -(-f("M") // 128) * -(-N // 176) * batch
    ebits = bits("D", "residual", "bias")
    if members:
        ebits |= bits("D_x1", "D_x2", "bias_x1", "bias_x2")
    vec = N % 4 == 0 and ldd % 4 == 0
    plain = not f("colscale") and not f("Dpre") and not f("act_after") and not f("atomic")
    lean = bool(plain and not f("rowscale") and f("act") == 0 and p == 0 and (ebits & 15) == 0 and vec and ldr % 4 == 0)
    lean3 = bool(not lean and plain and (f("rowscale") or p > 0) and f("act") == 0 and not f("frame_stats") and (ebits & 15) == 0 and vec and ldr % 4 == 0)
    lean4 = bool(not lean and not lean3 and not f("colscale") and not f("rowscale") and not f("residual") and not f("act_after") and not f("atomic")
                 and f("act") != 0 and not f("act_grad_src") and not f("frame_stats") and batch == 1 and not f("batch_accum")
                 and ((ebits | bits("Dpre")) & 15) == 0 and vec)
    nst = 4 if tiles <= cus else 2
    if f("frame_stats") and not (f("frame_rows") >= 64 and f("frame_rows") % 64 == 0 and f("M") % 64 == 0 and not f("act_grad_src") and lean and batch == 1):
        return ("refuse", 13)
    if f("act_grad_src"):
        if not (not any(f(k) for k in ("colscale", "Dpre", "rowscale", "residual", "bias", "act_after", "atomic")) and batch == 1 and ksegs == 1
                and f("act") != 0 and ((ebits | bits("act_grad_src")) & 15) == 0 and vec):
            return ("refuse", 14)
        return (2, nst, "batched")
    if f("batch_accum") and not (lean and batch > 1 and not f("d_p16") and (f("batch_accum") >> batch) == 0):
        return ("refuse", 15)
    if lean4:
        return (4, nst, "batched")
    if lean3:
        return (3, nst, "batched")
    if lean:
        return (1, nst, "batched")
    # EPI 0 chooses in the kernel: epi_vec_ok looks at D, Dpre, residual, bias, colscale (+ the members' D / bias), N, ldd, ldr
    vbits = bits("D", "Dpre", "residual", "bias", "colscale")
    if members:
        vbits |= bits("D_x1", "D_x2", "bias_x1", "bias_x2")
    vec_ok = (vbits & 15) == 0 and vec and ldr % 4 == 0
    if f("atomic") or not vec_ok:
        return (0, nst, "serial")
    return (0, nst, "batched" if nst == 4 else "rows_halves")


# ---- the fp32-staged GEMM through the C ABI (tests/test_01c_gemm_f32_abi_gpu.py): vptr_gemm's host decisions restated
GEMM_F32_MIN_TILES = 384      # kV4MinTiles of csrc/gemm.hip: grids below it take the pipelined loop


def gemm_f32_nfn(N):
    """nfn_for (csrc/gemm.hip): column fragments of the tile, exact 176-wide tiles when they divide N, else least padding"""
    if N % 176 == 0:
        return 11
    if N <= 64:
        return 4
    if N <= 128:
        return 8
    w11, w8, w4 = -(-N // 176) * 176, -(-N // 128) * 128, -(-N // 64) * 64
    nfn, best = 11, w11
    if w8 < best:
        best, nfn = w8, 8
    if w4 < best:
        best, nfn = w4, 4
    return nfn


def gemm_f32_plan(fields):
    """k_chunk, splits, NFN, tiles_m, tiles_n and the grid size exactly as vptr_gemm computes them (after its checks)"""
    f = lambda k: fields.get(k, 0) or 0
    split_k, batch = max(f("split_k"), 1), max(f("batch"), 1)
    M, N, K = f("M"), f("N"), f("K")
    k_chunk = -(-(-(-K // split_k)) // 32) * 32
    splits = -(-K // k_chunk)
    nfn = gemm_f32_nfn(N)
    tiles_m, tiles_n = -(-M // 128), -(-N // (16 * nfn))
    return dict(k_chunk=k_chunk, splits=splits, nfn=nfn, tiles_m=tiles_m, tiles_n=tiles_n, batch=batch, grid=tiles_m * tiles_n * splits * batch)


def gemm_f32_class(fields):
    """the launch class of a vptr_gemm call with fp32-staged operands (a_mode 0 .. 2, b_mode 0 / 1), restated from vptr_gemm, launch_one and the
    epilogue choice of the two kernels (csrc/gemm.hip).  fields: vptr_gemm_desc members by name, pointers as integer addresses (0 / missing =
    NULL), everything missing = 0.  Returns (loop, epilogue, NFN, A stager, B stager, NPASS) with loop "P" (vptr_gemm_kernel_p) or "S"
    (vptr_gemm_kernel), epilogue "rows", "frag" (gemm_epilogue<NFN, 1>), "rows_halves" or "serial", the stagers "kc", "ks2", "conv" / "kc", "ks";
    or ("refuse", k) with k the VPTR_CHECK of vptr_gemm that refuses the descriptor, counted from 1 at the empty-problem check in source order
    over the checks these operands can reach (30 = launch_modes' unsupported mode pair).  No device property enters the decision."""
    f = lambda k: fields.get(k, 0) or 0

    def bits(*ks):
        v = 0
        for k in ks:
            v |= int(f(k))
        return v
    M, N, K, am, bm = f("M"), f("N"), f("K"), f("a_mode"), f("b_mode")
    if not (M > 0 and N > 0 and K > 0):
        return ("refuse", 1)
    if not (f("A") and f("B") and (f("D") or f("D_planes"))):
        return ("refuse", 2)
    if f("D_planes") and am != 3:
        return ("refuse", 3)
    if f("precision") not in (1, 3):
        return ("refuse", 4)
    if f("batch_accum") or f("batch_stride_d"):
        return ("refuse", 5)
    if f("d_p16"):
        return ("refuse", 6)
    split_in = f("split_k")
    if (f("d_row_w") > 0 or f("d_row_off") != 0) and not (f("d_row_w") > 0 and am <= 2 and not f("residual") and not f("Dpre") and f("batch") <= 1
                                                         and not f("atomic") and split_in <= 1):
        return ("refuse", 7)
    if f("act_grad_src") or f("frame_stats"):
        return ("refuse", 8)
    if am == 4:
        return ("refuse", 9)
    if bits("A", "B") & 15:
        return ("refuse", 10)
    if not (am == 1 and bm == 1) and K % 4:
        return ("refuse", 11)
    if am == 0 and f("lda") % 4:
        return ("refuse", 12)
    if am == 1 and (f("lda") % 4 or M % 4):
        return ("refuse", 13)
    if bm == 0 and f("ldb") % 4:
        return ("refuse", 14)
    if bm == 1 and (f("ldb") % 4 or N % 4):
        return ("refuse", 15)
    if am == 2:
        if f("conv_Cin") % 4:
            return ("refuse", 16)
        if K != f("conv_KH") * f("conv_KW") * f("conv_Cin"):
            return ("refuse", 17)
        if not (f("conv_stride") >= 1 and f("conv_OH") > 0 and f("conv_OW") > 0):
            return ("refuse", 18)
    split_k = max(split_in, 1)
    p = f("dropout_p")
    if split_k > 1 and not (f("act") == 0 and not f("act_after") and p == 0 and not f("rowscale") and not f("Dpre")):
        return ("refuse", 19)
    if p > 0 and not (f("seed_dev") and p < 1):
        return ("refuse", 20)
    if f("rowscale") and not (f("rs_div") >= 1 and f("rs_mod") >= 1):
        return ("refuse", 21)
    batch, ksegs = max(f("batch"), 1), max(f("ksegs"), 1)
    if not (batch <= 3 and ksegs <= 3):
        return ("refuse", 22)
    if batch > 1 or ksegs > 1:
        if not (batch == 1 or ksegs == 1):
            return ("refuse", 23)
        if not (split_k == 1 and am != 2 and not f("a_rowsum")):
            return ("refuse", 24)
        extra = (batch if batch > 1 else ksegs) - 1
        if not (f("A_x1") and f("B_x1") and not bits("A_x1", "B_x1") & 15):
            return ("refuse", 25)
        if extra > 1 and not (f("A_x2") and f("B_x2") and not bits("A_x2", "B_x2") & 15):
            return ("refuse", 26)
        if batch > 1 and not (f("D_x1") and (extra < 2 or f("D_x2"))):
            return ("refuse", 27)
        if batch > 1 and (f("Dpre") or f("residual") or f("atomic")):
            return ("refuse", 28)
    if f("a_rowsum") and am != 1:
        return ("refuse", 29)
    if not ((am, bm) in ((0, 0), (0, 1), (1, 1), (1, 0), (2, 0))):
        return ("refuse", 30)
    plan = gemm_f32_plan(fields)
    loop = "P" if plan["grid"] < GEMM_F32_MIN_TILES or f("a_rowsum") else "S"
    use_atomic = bool(f("atomic")) or (batch <= 1 and plan["splits"] > 1)
    vbits = bits("D", "Dpre", "residual", "bias", "colscale")
    if batch > 1:
        vbits |= bits("D_x1", "D_x2", "bias_x1", "bias_x2")
    vec_ok = (vbits & 15) == 0 and N % 4 == 0 and f("ldd") % 4 == 0 and f("ldr") % 4 == 0
    rows = not use_atomic and vec_ok and f("d_row_w") == 0
    if loop == "P":
        epi = "rows" if rows else "frag"
    else:
        epi = "rows_halves" if plan["nfn"] == 11 and rows else "serial"
    return (loop, epi, plan["nfn"], ("kc", "ks2", "conv")[am], ("kc", "ks")[bm], f("precision"))


# ---- the 7x7 end convolutions through the C ABI (tests/test_09k_conv7_abi_gpu.py): the launchers' selection arithmetic of csrc/conv7.hip restated
CONV7_CLASSES = (
    "in_fwd/fwd2", "in_fwd/fwd2c", "in_fwd/fwd2c_attr", "in_fwd/gen1", "in_fwd/reject",
    "in_fwd_planes/fwd2", "in_fwd_planes/fwd2c", "in_fwd_planes/fwd2c_attr", "in_fwd_planes/reject",
    "in_bwd_weight/chunks", "in_bwd_weight/one_wg", "in_bwd_weight/reject",
    "out_fwd/fwd2", "out_fwd/gen1", "out_fwd/reject",
    "out_bwd_data/data2", "out_bwd_data/gen1", "out_bwd_data/reject",
    "out_bwd_weight/fpb4", "out_bwd_weight/fpb16", "out_bwd_weight/reject",
    "out_bwd_weight_ws/ws", "out_bwd_weight_ws/ws_attr", "out_bwd_weight_ws/fallback", "out_bwd_weight_ws/reject",
)


def conv7_class(op, **g):
    """the launch class of a call of csrc/conv7.hip, restated from its launchers.  Geometry keywords: B, Cimg, H, W and, where the entry point
    takes them, Cout / Cin (default 64), aligned (the plane buffer on 128 bytes, the workspace on 16; default True), deterministic (default
    False), ws_floats (None = a NULL workspace; default: exactly vptr_conv7_out_bwd_weight_workspace).  Returns {"class": one of CONV7_CLASSES}
    plus what the class walks:
    in_fwd / in_fwd_planes  fwd2: bands of 8 rows, rows of the last band; fwd2c: the same, 64-column chunks, quads of the last chunk (nq), dynamic
                            LDS bytes (fwd2c_attr: above 64 KB, the launcher raises the kernel's limit); gen1: workgroups of 64 pixels, pixels of
                            the last one;
    in_bwd_weight           chunks of 2048 pixels, pixels of the last one (deterministic: one workgroup);
    out_fwd                 fwd2: 4 x 16 patches, grid (x, Cimg), live waves of the last workgroup; gen1: 2 x 8 patches, the same;
    out_bwd_data            data2: bands of 8 rows, rows of the last band, LDS bytes; gen1: 16-channel groups per pixel (ngrp), pixels per workgroup;
    out_bwd_weight          frames per workgroup (fpb 4 / 16), grid y, frames of the last one;
    out_bwd_weight_ws       ws: partials (3 per frame), LDS bytes (ws_attr: above 64 KB); fallback: the reason and the plain call's class."""
    cdiv = lambda a, b: (a + b - 1) // b
    B, Cimg, H, W = g["B"], g["Cimg"], g["H"], g["W"]
    rej = {"class": op + "/reject"}
    if op in ("in_fwd", "in_fwd_planes"):
        planes = op == "in_fwd_planes"
        if planes:
            if not (B > 0 and 1 <= Cimg <= 4 and H > 3 and W > 3 and W % 4 == 0 and W <= (1024 if Cimg == 1 else 512) and g.get("Cout", 64) == 64) \
                    or not g.get("aligned", True):
                return rej
        elif not (B > 0 and Cimg > 0 and H > 3 and W > 3) or g.get("Cout", 64) != 64:
            return rej
        bands = cdiv(H, 8)
        walk = {"bands": B * bands, "last_band_rows": H - 8 * (bands - 1)}
        if Cimg == 1 and W % 4 == 0 and W <= 1024:
            return dict(walk, **{"class": op + "/fwd2", "lds": 4 * 14 * (W + 8)})
        if Cimg <= 4 and W % 4 == 0 and W <= 512:
            lds = 4 * Cimg * 14 * (W + 8)
            return dict(walk, **{"class": op + ("/fwd2c_attr" if lds > 65536 else "/fwd2c"), "lds": lds, "chunks": cdiv(W, 64),
                                 "last_nq": min(16, (W - 64 * (cdiv(W, 64) - 1)) // 4)})
        if 4 * Cimg * 49 * 64 > 65536:
            return rej
        npix = B * H * W
        return {"class": op + "/gen1", "blocks": cdiv(npix, 64), "last_pixels": npix - 64 * (cdiv(npix, 64) - 1)}
    if op == "in_bwd_weight":
        if not (B > 0 and Cimg > 0 and H > 3 and W > 3) or g.get("Cout", 64) != 64:
            return rej
        npix = B * H * W
        if g.get("deterministic", False):
            return {"class": op + "/one_wg", "chunks": 1, "last_pixels": npix}
        return {"class": op + "/chunks", "chunks": cdiv(npix, 2048), "last_pixels": npix - 2048 * (cdiv(npix, 2048) - 1)}
    Cin = g.get("Cin", 64)
    if op == "out_fwd":
        if not (B > 0 and H > 3 and W > 3 and Cimg > 0) or Cin != 64:
            return rej
        if Cimg <= 4 and H % 4 == 0 and W % 16 == 0:
            patches = B * (H // 4) * (W // 16)
            return {"class": op + "/fwd2", "grid": (cdiv(patches, 4), Cimg), "last_waves": patches - 4 * (cdiv(patches, 4) - 1)}
        if 4 * Cimg * 49 * 64 > 65536:
            return rej
        patches = B * ((H + 1) // 2) * ((W + 7) // 8)
        return {"class": op + "/gen1", "grid": (cdiv(patches, 4), 1), "last_waves": patches - 4 * (cdiv(patches, 4) - 1)}
    if op == "out_bwd_data":
        if not (B > 0 and Cin > 0 and Cin % 16 == 0 and 256 % (Cin // 16) == 0 and H > 6 and W > 6 and Cimg > 0):
            return rej
        lds2 = 4 * Cimg * (H + 12) * 80
        if Cimg <= 4 and Cin == 64 and W == 64 and lds2 <= 80 * 1024:
            bands = cdiv(H, 8)
            return {"class": op + "/data2", "bands": B * bands, "last_band_rows": H - 8 * (bands - 1), "lds": lds2}
        if 4 * Cimg * 49 * Cin > 65536:
            return rej
        ppb = 256 // (Cin // 16)
        return {"class": op + "/gen1", "ngrp": Cin // 16, "pixels_per_wg": ppb, "blocks": cdiv(B * H * W, ppb)}

    def plain():
        if not (B > 0 and Cin == 64 and H % 8 == 0 and W % 8 == 0 and 1 <= Cimg <= 3):
            return {"class": "out_bwd_weight/reject"}
        fpb = 16 if B >= 64 else 4
        return {"class": "out_bwd_weight/fpb%d" % fpb, "fpb": fpb, "grid": ((H // 8) * (W // 8), cdiv(B, fpb)), "last_frames": B - fpb * (cdiv(B, fpb) - 1)}
    if op == "out_bwd_weight":
        return plain()
    assert op == "out_bwd_weight_ws", op
    need = B * 3 * Cimg * 49 * 64
    GW = 4 * ((W + 6 + 3) // 4) + 8
    lds = max(4 * (cdiv(H + 6, 3) + 1 + 6) * GW, 4 * 4 * 49 * 64)
    ws_floats = g.get("ws_floats", need)
    reason = ("null" if ws_floats is None else "short" if ws_floats < need else "lds" if lds > 150 * 1024 else "small" if H < 8 or W < 8 else None)
    if reason:
        p = plain()
        return {"class": op + ("/fallback" if p["class"] != "out_bwd_weight/reject" else "/reject"), "reason": reason, "plain": p}
    if not (B > 0 and Cin == 64 and 1 <= Cimg <= 3) or not g.get("aligned", True):
        return rej
    return {"class": op + ("/ws_attr" if lds > 65536 else "/ws"), "partials": 3 * B, "lds": lds}
