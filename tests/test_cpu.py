"""CPU-only tests: the oracle against the golden vectors captured from the reference, host-side logic (module tree,
state_dict keys, position tables, init), and that the C-ABI library loads and exports every declared symbol."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from helpers import build_transformer, grad_floor, jload, load, rel
from oracle import fill
from oracle import vptr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- oracle pinning
@pytest.mark.parametrize("name", ["nar_tiny", "nar_tiny_norpe", "far_tiny", "nar_tiny_pad", "nar_tiny_T", "nar_tiny_tslma", "nar_tiny_tslma_pad"])
def test_oracle_matches_reference_golden(name):
    z = load(name)
    cfg, far = jload(z, "cfg"), bool(int(z["far"]))
    tmpl = jload(z, "template")
    P = fill.fill_state([tuple(t) for t in tmpl], int(z["seed"]))
    for k, shape, dt in tmpl:  # entries the fill does not produce
        if k not in P:
            if "buf:" + k in z.files:
                P[k] = torch.from_numpy(z["buf:" + k])
            elif k.endswith("relative_position_index"):
                P[k] = O.rpe_index(cfg["window_size"])
            elif k.endswith("num_batches_tracked"):
                P[k] = torch.zeros((), dtype=torch.long)
    leaves = {}
    for k, shape, dt in tmpl:
        if "grad:" + k in z.files:
            P[k] = P[k].clone().requires_grad_(True)
            leaves[k] = P[k]
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    fwd = O.far_forward if far else O.nar_forward
    with torch.no_grad():
        Pe = {k: v.detach().clone() for k, v in P.items()}
        assert rel(fwd(Pe, x, cfg, training=False), z["out_eval"]) < 1e-5
    out = fwd(P, x, cfg, training=True)
    assert rel(out, z["out_train"]) < 1e-5
    (out * torch.from_numpy(z["g"])).sum().backward()
    assert rel(x.grad, z["dx"]) < 1e-5
    floor = grad_floor(np.linalg.norm(z[k]) for k in z.files if k.startswith("grad:"))
    for k, t in leaves.items():
        assert rel(t.grad, z["grad:" + k], floor) < 2e-4, k
    for k in z.files:
        if k.startswith("bn_after:"):
            assert rel(P[k[9:]], z[k]) < 1e-5


@pytest.mark.parametrize("name", ["ae_tiny_reflect", "ae_tiny_zero"])
def test_oracle_autoencoder_golden(name):
    z = load(name)
    meta = jload(z, "meta")
    Pe = fill.fill_state([tuple(t) for t in jload(z, "enc_template")], meta["seed"])
    Pd = fill.fill_state([tuple(t) for t in jload(z, "dec_template")], meta["seed"] + 10)
    x = torch.from_numpy(z["x"])
    with torch.no_grad():
        f = O.enc_forward(Pe, x, padding_type=meta["padding_type"])
    assert rel(f, z["feat"]) < 1e-5
    fin = torch.from_numpy(z["feat"]).requires_grad_(True)
    y = O.dec_forward(Pd, fin, out_layer=meta["out_layer"])
    assert rel(y, z["y"]) < 1e-5
    (y * torch.from_numpy(z["g"])).sum().backward()
    assert rel(fin.grad, z["dfeat"]) < 1e-5


def test_oracle_losses_golden():
    import torch.nn.functional as F
    z = load("losses_tiny")
    gt, gf = torch.from_numpy(z["gt"]), torch.from_numpy(z["gf"])
    pr, pf = torch.from_numpy(z["pr"]).requires_grad_(True), torch.from_numpy(z["pf"]).requires_grad_(True)
    l = O.gdl_loss(gt, pr) + O.mse_loss(pr, gt) + 0.1 * O.bipatch_nce(F.normalize(gf, p=2.0, dim=2), F.normalize(pf, p=2.0, dim=2))
    l.backward()
    assert abs(l.item() - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    assert rel(pr.grad, z["dpr"]) < 1e-6 and rel(pf.grad, z["dpf"]) < 1e-6
    assert abs(O.mse_loss(pr, gt).item() - float(z["mse"])) < 1e-6 and abs(O.gdl_loss(gt, pr).item() - float(z["gdl"])) < 1e-6


def test_oracle_position_tables_golden():
    z = load("pos_tables")
    for tag in ("6_96_4", "20_528_4", "50_528_8"):
        T, E, ws = (int(s) for s in tag.split("_"))
        assert rel(O.pos1d(T, E), z["p1:" + tag]) < 1e-6
        assert rel(O.pos2d(E, ws, ws), z["p2:" + tag]) < 1e-6
        if "p3:" + tag in z.files:
            assert rel(O.pos3d(E, T, ws, ws), z["p3:" + tag]) < 1e-6
        else:
            n, s = fill.digest(O.pos3d(E, T, ws, ws))
            assert abs(n - float(z["p3n:" + tag])) < 1e-5 * n and rel(s, z["p3s:" + tag]) < 1e-6
    for ws in (4, 8):
        assert np.array_equal(O.rpe_index(ws).numpy(), z[f"rpe_index:{ws}"])


def test_oracle_train_step_golden():
    z = load("step_tiny")
    cfg, meta = jload(z, "cfg"), jload(z, "meta")
    Pe = fill.fill_state([tuple(t) for t in jload(z, "enc_template")], meta["seed"])
    Pd = fill.fill_state([tuple(t) for t in jload(z, "dec_template")], meta["seed"] + 10)
    tm = jload(z, "T_template")
    PT = fill.fill_state([tuple(t) for t in tm], meta["seed"] + 20)
    PT["temporal_pos"] = O.pos1d(cfg["Tp"] + cfg["Tf"], cfg["C"])
    PT["lw_pos"] = O.pos2d(cfg["C"], cfg["window_size"], cfg["window_size"])
    for k, s, d in tm:
        if k.endswith("relative_position_index"):
            PT[k] = O.rpe_index(cfg["window_size"])
        elif k.endswith("num_batches_tracked"):
            PT[k] = torch.zeros((), dtype=torch.long)
    for P, t in ((Pe, jload(z, "enc_template")), (Pd, jload(z, "dec_template"))):
        for k, s, d in t:
            if k.endswith("num_batches_tracked"):
                P[k] = torch.zeros((), dtype=torch.long)
    st = O.NARStep(Pe, Pd, PT, cfg)
    for s, ref in enumerate(jload(z, "records")):
        past = (fill.rand_input((meta["N"], cfg["Tp"], 1, meta["HW"], meta["HW"]), meta["seed"] + 100 + s) - 0.6013795) / 2.7570653
        fut = (fill.rand_input((meta["N"], cfg["Tf"], 1, meta["HW"], meta["HW"]), meta["seed"] + 200 + s) - 0.6013795) / 2.7570653
        r = st.step(past, fut)
        for k in ref:
            assert abs(r[k] - ref[k]) <= 2e-4 * abs(ref[k]) + 1e-7, (k, r[k], ref[k])
    worst = max(rel(st.P_T[k[5:]], z[k]) for k in z.files if k.startswith("post:"))
    assert worst < 1e-4


# ------------------------------------------------------------------------------------------------------ host-side logic
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "vptr_hip.h")).read()
    declared = set(re.findall(r"\b(vptr_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"vptr_gemm_desc"}
    from vptr_amd import _lib
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.lib.vptr_abi_version() == 10
    assert ctypes.sizeof(_lib.GemmDesc) % 8 == 0


def test_wgrad_kernel_counts_query():
    """vptr_wgrad_kernel_counts (which grouped weight-gradient kernel ran): host-side counters, all zero in a freshly loaded library (a
    child process: in a GPU run of the whole suite this process has launched them); n outside 1 .. 5 and a null output are rejected"""
    import subprocess
    code = ("import ctypes\n"
            "from vptr_amd import _lib\n"
            "out = (ctypes.c_int * 5)(*([-1] * 5))\n"
            "assert _lib.lib.vptr_wgrad_kernel_counts(out, 5) == 0\n"
            "print(list(out))\n"
            "one = (ctypes.c_int * 5)(*([-1] * 5))\n"
            "assert _lib.lib.vptr_wgrad_kernel_counts(one, 1) == 0 and list(one) == [0, -1, -1, -1, -1]\n"
            "for n in (0, 6, -1):\n"
            "    assert _lib.lib.vptr_wgrad_kernel_counts(out, n) != 0 and b'1 .. 5' in _lib.lib.vptr_last_error(), n\n"
            "assert _lib.lib.vptr_wgrad_kernel_counts(None, 5) != 0\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == "[0, 0, 0, 0, 0]", r.stdout


# vptr_attn_route: expected routes transcribed from the launchers' cascade as it stood before csrc/attn_route.h took it over (vptr_attn_mfma_ok,
# vptr_attn16_ok, the heads of vptr_attn16_fwd / _bwd, rows16_fits and the prefetch split of the entry points), never from the code under test.
# Columns: the geometries below in order, "forward/backward"; g1 / g2 = attn16 first / second generation, amp / ams = attn_mfma plain / tile-sharing
# backward, v16 / vec = 16-token / generic fp32 vector kernels; "+" = the variant bit (attn16: unmasked 16 x 16; v16: prefetch; attn_mfma: Lq > 16)
ROUTE_GEOMS = {"win4": (0, 16, 16, 4, 0, 12), "win8": (0, 64, 64, 8, 0, 2), "win2": (0, 4, 4, 2, 0, 12), "t5_causal": (1, 5, 5, 0, 1, 18),
               "t3x7": (1, 3, 7, 0, 0, 18), "t20_causal": (1, 20, 20, 0, 1, 5), "t40x33": (1, 40, 33, 0, 0, 3), "t10_1551px": (1, 10, 10, 0, 0, 1551),
               "t16_1551px": (1, 16, 16, 0, 0, 1551), "t17": (1, 17, 17, 0, 0, 18)}     # kind, Lq, Lk, ws, causal, groups
ROUTE_HEADS = {24: (2, 48), 66: (8, 528), 94: (2, 188), 96: (2, 192), 98: (2, 196), 22: (2, 44), 18: (3, 54)}      # head dim: (nh, C); C = 54: C % 4 != 0
ROUTE_PAIRS = {24: (1, 2), 66: (3, 5), 94: (3, 6), 96: (3, 6), 22: (1, 2), 18: (1, 2)}   # of the matrix-unit families (hd 94: second-generation span 96)
ROUTE_ENVS = {"default": {}, "attn16": {"VPTR_ATTN16": "2"}, "attn16fwd": {"VPTR_ATTN16": "4"}, "mfma": {"VPTR_ATTN_MFMA": "2"},
              "vector": {"VPTR_ATTN_MFMA": "0"}, "fwd1": {"VPTR_ATTN16_FWD1": "1"}}
_BIG = "amp+/ams+"
_OVER = "vec/vec vec/vec vec/vec v16/v16 v16/v16 vec/vec vec/vec v16/v16 v16/v16 vec/vec"      # hd 98; hd 94 / 96 on the vector kernels (rows16_fits fails)
_G1_VEC = "g1+/v16 %s vec/vec g1/v16 g1/v16 %s %s g1/v16+ g1+/v16+ %s" % ((_BIG,) * 4)         # first-generation forward, 16-token vector backward
ROUTE_TABLE = {
    "default": {(24, 66, 94, 96, 22): "g2+/g2+ %s vec/vec g2/g2 g2/g2 %s %s g2/g2 g2+/g2+ %s" % ((_BIG,) * 4), (18,): _G1_VEC, (98,): _OVER},
    "attn16": {(24, 66, 94, 96, 22, 18): "g1+/g1+ %s vec/vec g1/g1 g1/g1 %s %s g1/g1 g1+/g1+ %s" % ((_BIG,) * 4), (98,): _OVER},
    "attn16fwd": {(24, 22, 18): _G1_VEC, (66,): "g1+/v16 %s vec/vec g1/v16 g1/v16 %s %s g1/v16+ g1+/v16 %s" % ((_BIG,) * 4),     # 16 * 34 = 544 > 384
                  (94, 96): "g1+/vec %s vec/vec g1/v16 g1/v16 %s %s g1/v16 g1+/v16 %s" % ((_BIG,) * 4), (98,): _OVER},
    "mfma": {(24, 66, 94, 96, 22, 18): "amp/amp %s amp/amp amp/amp amp/amp %s %s amp/amp amp/amp %s" % ((_BIG,) * 4), (98,): _OVER},
    "vector": {(24, 22, 18): "v16/v16 vec/vec vec/vec v16/v16 v16/v16 vec/vec vec/vec v16+/v16+ v16+/v16+ vec/vec",
               (66,): "v16/v16 vec/vec vec/vec v16/v16 v16/v16 vec/vec vec/vec v16+/v16+ v16/v16 vec/vec", (94, 96, 98): _OVER},
    "fwd1": {(24, 66, 94, 96, 22): "g1+/g2+ %s vec/vec g1/g2 g1/g2 %s %s g1/g2 g1+/g2+ %s" % ((_BIG,) * 4), (18,): _G1_VEC, (98,): _OVER},
}
_ROUTE_CHILD = """
import ctypes, json, os, sys
from vptr_amd import _lib
job = json.loads(sys.argv[1])
res = []
for env, calls in job:
    for k in ("VPTR_ATTN_MFMA", "VPTR_ATTN16", "VPTR_ATTN16_FWD1"):
        os.environ.pop(k, None)
    os.environ.update(env)
    for c in calls:
        out = (ctypes.c_int * 4)(-1, -1, -1, -1)
        assert _lib.lib.vptr_attn_route(*c, out, 4) == 0, c
        res.append(list(out))
out = (ctypes.c_int * 5)(*([-7] * 5))
for n in (0, 5, -1):
    assert _lib.lib.vptr_attn_route(0, 16, 16, 48, 2, 4, 0, 12, 0, 1, out, n) != 0 and b"1 .. 4" in _lib.lib.vptr_last_error(), n
assert _lib.lib.vptr_attn_route(0, 16, 16, 48, 2, 4, 0, 12, 0, 1, None, 4) != 0 and list(out) == [-7] * 5
assert _lib.lib.vptr_attn_route(0, 16, 16, 48, 2, 4, 0, 12, 0, 1, out, 2) == 0 and list(out) == [3, 1, -7, -7, -7]
print(json.dumps(res))
"""


def test_attn_route_table():
    """vptr_attn_route (which kernel family serves an attention call) in a child process, the switches set per mode: the five ATTN_MODES and
    VPTR_ATTN16_FWD1=1 over seven head classes x ten geometries x forward / backward against the table above, the unaligned fallback, a tensor of
    2^31 elements; n outside 1 .. 4 and a null output are rejected"""
    import json
    import subprocess
    from helpers import ATTN_FAMILIES, ATTN_MODES, attn_kernel_mode
    fam = {"vec": "vector", "v16": "vector16", "g1": "a16_gen1", "g2": "a16_gen2", "amp": "am_plain", "ams": "am_shared"}
    job, want = [], []
    for mode, env in ROUTE_ENVS.items():
        if mode in ATTN_MODES:           # the helper the GPU tests switch families with sets the same variables
            with attn_kernel_mode(mode):
                assert {k: os.environ.get(k) for k in ("VPTR_ATTN_MFMA", "VPTR_ATTN16")} == {"VPTR_ATTN_MFMA": env.get("VPTR_ATTN_MFMA"),
                                                                                              "VPTR_ATTN16": env.get("VPTR_ATTN16")}
        rows = {hd: row.split() for hds, row in ROUTE_TABLE[mode].items() for hd in hds}
        assert sorted(rows) == sorted(ROUTE_HEADS) and all(len(r) == len(ROUTE_GEOMS) for r in rows.values())
        calls = []
        for hd, (nh, C) in ROUTE_HEADS.items():
            for (kind, Lq, Lk, ws, causal, groups), cell in zip(ROUTE_GEOMS.values(), rows[hd]):
                for backward, tok in enumerate(cell.split("/")):
                    calls.append((kind, Lq, Lk, C, nh, ws, causal, groups, backward, 1))
                    f = fam[tok.rstrip("+")]
                    want.append([ATTN_FAMILIES.index(f), *(ROUTE_PAIRS[hd] if f[0] == "a" else (0, 0)), int(tok.endswith("+"))])
        job.append((env, calls))
    assert set(ATTN_MODES) < set(ROUTE_ENVS) and len(want) == 6 * 7 * 10 * 2
    # default mode, win4 at hd 66 with a tensor off the 16-byte grid: first generation both ways; t20 causal with 2^18 pixels at C = 528 (20 * 2^18 *
    # 528 >= 2^31 elements): the 32-bit row offsets of attn_mfma do not reach, generic vector kernels
    job.append(({}, [(0, 16, 16, 528, 8, 4, 0, 12, b, 0) for b in (0, 1)] + [(1, 20, 20, 528, 8, 0, 1, 1 << 18, b, 1) for b in (0, 1)]))
    want += [[2, 3, 5, 1], [2, 3, 5, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert 20 * (1 << 18) * 528 >= 1 << 31
    r = subprocess.run([sys.executable, "-c", _ROUTE_CHILD, json.dumps(job)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    flat = [(m, c) for (_, calls), m in zip(job, list(ROUTE_ENVS) + ["extra"]) for c in calls]
    bad = [(m, c, g, w) for (m, c), g, w in zip(flat, got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:8]


def test_graft_entry_build_runs():
    """the driver's build check (`__graft_entry__.build()`): compiles what changed, imports the package, checks the ABI version"""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.build()


def test_product_path_has_no_cpu_fallback():
    import vptr_amd.ops as ops
    x = torch.randn(8, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(x, torch.randn(4, 16), None)
    for root, _, files in os.walk(os.path.join(ROOT, "vptr_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


@pytest.mark.parametrize("name", ["nar_tiny", "nar_tiny_norpe", "far_tiny", "nar_tiny_tslma", "nar_k64_digest", "far_bair_digest"])
def test_state_dict_keys_match_reference(name):
    import vptr_amd.model as pkg
    z = load(name)
    cfg, far = jload(z, "cfg"), bool(int(z["far"]))
    m = build_transformer(pkg, cfg, far)
    assert [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()] == \
        [tuple(t) if False else (t[0], t[1], t[2]) for t in jload(z, "template")]
    for k in ("temporal_pos", "lw_pos", "Tlw_pos"):
        if "buf:" + k in z.files:
            assert torch.equal(m.state_dict()[k], torch.from_numpy(z["buf:" + k])), k


def test_autoencoder_keys_and_api():
    import vptr_amd.model as pkg
    import model as shim
    assert shim.VPTREnc is pkg.VPTREnc and shim.VPTRFormerNAR is pkg.VPTRFormerNAR and shim.init_weights is pkg.init_weights
    for name in ("ae_tiny_reflect", "ae_tiny_zero"):
        z = load(name)
        meta = jload(z, "meta")
        enc = pkg.VPTREnc(meta["img_ch"], meta["feat"], 3, meta["padding_type"])
        dec = pkg.VPTRDec(meta["img_ch"], meta["feat"], 3, meta["out_layer"], meta["padding_type"])
        assert [(k, list(v.shape)) for k, v in enc.state_dict().items()] == [(k, s) for k, s, _ in jload(z, "enc_template")]
        assert [(k, list(v.shape)) for k, v in dec.state_dict().items()] == [(k, s) for k, s, _ in jload(z, "dec_template")]
    with pytest.raises(ValueError):
        pkg.VPTRDec(1, 48, 3, "Softmax")
    with pytest.raises(NotImplementedError):
        pkg.VPTREnc(1, 48, 3, "circular")
    enc = pkg.VPTREnc(1, 48, 3)
    pkg.init_weights(enc)
    w = enc.encoder.model[1].weight
    assert abs(float(w.std()) - 0.02) < 0.005
    assert abs(float(enc.encoder.model[2].weight.mean()) - 1.0) < 0.02


def test_reset_parameters_quirks():
    """xavier over every dim>1 parameter: RPE table, frame_queries and the 3-D LayerNorm affines are re-initialised
    (VPTR_modules.py:149-152, SURVEY.md section 8b 'Init semantics')."""
    import vptr_amd.model as pkg
    torch.manual_seed(0)
    m = pkg.VPTRFormerNAR(2, 2, 8, 8, 48, 8, 1, 1, 0.1, 4, 4, False, True)
    assert m.num_future_frames == 2 and callable(m.NCE_projector)
    ln = m.transformer.decoder.layers[0].SpatialFFN.norm1
    assert ln.weight.dim() == 3 and float(ln.weight.abs().max()) < 0.2       # not ones any more
    assert float(m.frame_queries.std()) < 0.1                                   # not randn any more
    bn = m.transformer.encoder.layers[0].SpatialFFN.norm1
    assert isinstance(bn, torch.nn.BatchNorm2d) and float(bn.weight.min()) == 1.0
    assert m.transformer.encoder.layers[0]._site != m.transformer.decoder.layers[0]._site


def test_losses_cpu_match_oracle():
    import torch.nn.functional as F
    import vptr_amd.model as pkg
    z = load("losses_tiny")
    gt, gf = torch.from_numpy(z["gt"]), torch.from_numpy(z["gf"])
    pr, pf = torch.from_numpy(z["pr"]), torch.from_numpy(z["pf"])
    N, T, C, h, w = gf.shape
    l = pkg.GDL(alpha=1)(gt, pr) + pkg.MSELoss()(pr, gt) + 0.1 * pkg.BiPatchNCE(N, T, h, w, 1.0)(
        F.normalize(gf, p=2.0, dim=2), F.normalize(pf, p=2.0, dim=2))
    assert abs(l.item() - float(z["loss"])) < 1e-6 * abs(float(z["loss"]))
    w = pkg.temporal_weight_func(10)
    assert abs(float(w[-1]) - 10.0) < 1e-4 and float(w[0]) == 1.0


# ------------------------------------------------------------------------------------------- checkpoints (section 8f rank 1)
def _tiny_modules():
    import vptr_amd.model as M
    T = M.VPTRFormerNAR(2, 2, 8, 8, 48, 8, 1, 1, 0.0, 4, 4, False, True)
    enc = M.VPTREnc(1, 48, 3, "reflect")
    return enc, T


def test_checkpoint_roundtrip_and_ddp_prefix(tmp_path):
    from vptr_amd import checkpoint as C
    enc, T = _tiny_modules()
    fill.apply_fill(enc, 1)
    fill.apply_fill(T, 2)
    opt = torch.optim.AdamW(T.parameters(), lr=1e-4)
    for p in T.parameters():
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    loss_dict = C.init_loss_dict(["T_MSE", "T_total"])
    loss_dict["T_MSE"].train.append(0.5)
    loss_dict["epochs"] = 1
    f = C.save_ckpt({"VPTR_Enc": enc, "VPTR_Transformer": T}, {"optimizer_T": opt}, 7, loss_dict, tmp_path)
    assert f.name == "epoch_7.tar"
    raw = open(f, "rb").read() if not __import__("zipfile").is_zipfile(f) else b"".join(
        __import__("zipfile").ZipFile(f).read(n) for n in __import__("zipfile").ZipFile(f).namelist() if n.endswith("data.pkl"))
    assert b"utils.train_summary" in raw and b"Loss_tuple" in raw and b"vptr_amd" not in raw  # loadable by the reference
    msd, osd, epoch, ld, code = C.load_ckpt(f)
    assert epoch == 7 and ld["T_MSE"].train == [0.5] and isinstance(ld["T_total"], C.LossTuple) and code == {}
    enc2, T2 = _tiny_modules()
    opt2 = torch.optim.AdamW(T2.parameters(), lr=3e-4)
    ld2, start = C.resume_training({"VPTR_Enc": enc2, "VPTR_Transformer": T2}, {"optimizer_T": opt2}, f, ["T_MSE", "T_total", "T_new"])
    assert start == 7 and ld2["T_new"].train == [0]
    for (k, a), (_, b) in zip(T.state_dict().items(), T2.state_dict().items()):
        assert torch.equal(a, b), k
    assert opt2.state_dict()["param_groups"][0]["lr"] == 1e-4
    # a checkpoint written under DistributedDataParallel: every key prefixed with `module.` (train_summary.py:16-21)
    ddp_sd = {"module." + k: v for k, v in T.state_dict().items()}
    torch.save({"epoch": 3, "loss_dict": {"epochs": 0}, "Module_state_dict": {"VPTR_Transformer": ddp_sd},
                "optimizer_state_dict": {}, "code": {}}, tmp_path / "ddp.tar")
    _, T3 = _tiny_modules()
    start, hist = C.resume_training({"VPTR_Transformer": T3}, {}, tmp_path / "ddp.tar", None, map_location="cpu")
    assert start == 3 and torch.equal(T3.state_dict()["frame_queries"], T.state_dict()["frame_queries"])


def _pickle_globals(f):
    """the (module, name) globals the data.pkl of a torch.save zip file references -- what an unpickler has to resolve"""
    import pickletools
    import zipfile
    z = zipfile.ZipFile(f)
    raw = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    return {tuple(arg.split(" ", 1)) for op, arg, _ in pickletools.genops(raw) if op.name == "GLOBAL"}


def test_checkpoint_interop_with_reference(tmp_path):
    """a checkpoint written by the REFERENCE's save_ckpt (tests/golden/ckpt_ref_nar24.tar, oracle/make_golden.py::ckpt_case) loads
    here, and one written here loads through the reference's load_ckpt: a bare torch.load that resolves only globals a reference-written
    file holds, with the same top-level layout and a state dict of the same keys, shapes and dtypes"""
    import vptr_amd.model as M
    from vptr_amd import checkpoint as C
    ref_file = os.path.join(ROOT, "tests", "golden", "ckpt_ref_nar24.tar")

    def tiny():
        return M.VPTRFormerNAR(2, 2, 8, 8, 24, 4, 1, 1, 0.0, 4, 4, False, True)
    Tr = tiny()
    fill.apply_fill(Tr, 5)      # the fill the reference's module got before its save_ckpt
    T = tiny()
    loss_dict, start = C.resume_training({"VPTR_Transformer": T}, {}, ref_file, ["T_MSE"])
    assert start == 2 and loss_dict["T_MSE"].val == [0.25]
    for (k, a), (k2, b) in zip(Tr.state_dict().items(), T.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    f = C.save_ckpt({"VPTR_Transformer": T}, {}, 4, loss_dict, tmp_path / "ours")
    # what the reference's load_ckpt does (train_summary.py:150-160) is a plain torch.load: every global of this file must be one that a
    # file the reference wrote references too (utils.train_summary.Loss_tuple, torch storages, OrderedDict), nothing of vptr_amd
    want = _pickle_globals(ref_file)
    assert ("utils.train_summary", "Loss_tuple") in want
    assert _pickle_globals(f) <= want, _pickle_globals(f) - want
    assert ("utils.train_summary", "Loss_tuple") in _pickle_globals(f)
    ck, rk = C.load_ckpt(f), C.load_ckpt(ref_file)
    assert ck[2] == 4 and ck[3]["T_MSE"].val == [0.25]
    ours, theirs = ck[0]["VPTR_Transformer"], rk[0]["VPTR_Transformer"]
    assert [(k, tuple(v.shape), v.dtype) for k, v in ours.items()] == [(k, tuple(v.shape), v.dtype) for k, v in theirs.items()]
    # the reference's Module.load_state_dict on that state dict: the same tensors come back
    T2 = tiny()
    T2.load_state_dict(ours)
    for (k, a), (_, b) in zip(T2.state_dict().items(), Tr.state_dict().items()):
        assert torch.equal(a, b), k


def test_flat_adamw_state_dict_is_torch_adamw_compatible():
    from vptr_amd.train import FlatAdamW
    torch.manual_seed(0)
    lin = torch.nn.Sequential(torch.nn.Linear(8, 5), torch.nn.Linear(5, 3))
    ref_opt = torch.optim.AdamW(lin.parameters(), lr=2e-4, weight_decay=0.02)
    for _ in range(3):
        for p in lin.parameters():
            p.grad = torch.randn_like(p)
        ref_opt.step()
    sd = ref_opt.state_dict()
    lin2 = torch.nn.Sequential(torch.nn.Linear(8, 5), torch.nn.Linear(5, 3))
    fo = FlatAdamW(lin2.parameters(), lr=1e-4)
    fo.load_state_dict(sd)
    assert fo.lr == 2e-4 and fo.weight_decay == 0.02 and float(fo.step_dev) == 3.0
    off = 0
    for i, p in enumerate(lin.parameters()):
        n = p.numel()
        assert torch.equal(fo.m[off:off + n].view(p.shape), sd["state"][i]["exp_avg"])
        assert torch.equal(fo.v[off:off + n].view(p.shape), sd["state"][i]["exp_avg_sq"])
        off += n
    back = torch.optim.AdamW(lin2.parameters(), lr=1.0)
    back.load_state_dict(fo.state_dict())
    b = back.state_dict()
    assert b["param_groups"][0]["lr"] == 2e-4
    for i in sd["state"]:
        assert torch.equal(b["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"]) and float(b["state"][i]["step"]) == 3.0


def test_flat_adamw_state_dict_channel_last_params():
    """Parameters that FlatAdamW STORES channel-last (LayerNorm((C,H,W)) affines, depthwise 3x3 weights) must cross the
    torch.optim.AdamW state format in their logical layout, both ways (round-1 bug: slab order leaked into the state)."""
    from vptr_amd.train import FlatAdamW
    torch.manual_seed(1)

    def make():
        return torch.nn.ModuleList([torch.nn.Conv2d(4, 4, 3, groups=4), torch.nn.LayerNorm((3, 2, 2)), torch.nn.Linear(6, 5)])
    ref = make()
    ref_opt = torch.optim.AdamW(ref.parameters(), lr=3e-4, weight_decay=0.01)
    for _ in range(2):
        for p in ref.parameters():
            p.grad = torch.randn_like(p)
        ref_opt.step()
    sd = ref_opt.state_dict()
    ours = make()
    ours.load_state_dict(ref.state_dict())
    cl = [id(ours[0].weight), id(ours[1].weight), id(ours[1].bias)]
    fo = FlatAdamW(ours.parameters(), lr=1e-4, channel_last=cl)
    for a_, b_ in zip(ours.parameters(), ref.parameters()):
        assert torch.equal(a_.detach(), b_.detach())          # re-pointing into the slab keeps the logical values
    assert not ours[0].weight.is_contiguous()                  # ... while the storage order really is channel-last
    fo.load_state_dict(sd)
    for i, p in enumerate(ours.parameters()):
        off, n, layout = fo._layout[i]
        m_logical = fo.m[off:off + n].view(layout[0]).permute(layout[1]) if layout else fo.m[off:off + n].view(p.shape)
        assert torch.equal(m_logical, sd["state"][i]["exp_avg"]), "moment of parameter %d scrambled on load" % i
        # the slab itself holds the moment in the SAME storage order as the parameter
        if layout:
            assert torch.equal(fo.m[off:off + n], sd["state"][i]["exp_avg"].permute(*[*range(1, p.dim()), 0]).reshape(-1))
    out = fo.state_dict()
    for i in sd["state"]:
        assert out["state"][i]["exp_avg"].is_contiguous()
        assert torch.equal(out["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(out["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    back = torch.optim.AdamW(make().parameters(), lr=1.0)
    back.load_state_dict(out)     # shapes are the logical ones: torch accepts the state as its own
    with pytest.raises(ValueError):
        bad = {"param_groups": sd["param_groups"], "state": {k: dict(v) for k, v in sd["state"].items()}}
        bad["state"][0]["exp_avg"] = bad["state"][0]["exp_avg"].reshape(-1)
        fo.load_state_dict(bad)


def test_oracle_far_train_step_golden():
    z = load("step_far_tiny")
    cfg, meta = jload(z, "cfg"), jload(z, "meta")
    import vptr_amd.model as M
    enc = M.VPTREnc(1, meta["feat"], 3, "reflect")
    dec = M.VPTRDec(1, meta["feat"], 3, meta["out_layer"], "reflect")
    T = build_transformer(M, cfg, True)
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 10)
    fill.apply_fill(T, meta["seed"] + 20)
    st = O.FARStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(T.state_dict()), cfg, out_layer=meta["out_layer"])
    for s, ref in enumerate(jload(z, "records")):
        past = fill.rand_input((meta["N"], cfg["Tp"], 1, meta["HW"], meta["HW"]), meta["seed"] + 100 + s)
        fut = fill.rand_input((meta["N"], cfg["Tf"], 1, meta["HW"], meta["HW"]), meta["seed"] + 200 + s)
        r = st.step(past, fut)
        for k in ref:
            assert abs(r[k] - ref[k]) <= 2e-4 * abs(ref[k]) + 1e-7, (k, r[k], ref[k])
    worst = max(rel(st.P_T[k[5:]], z[k]) for k in z.files if k.startswith("post:"))
    assert worst < 1e-4


def test_oracle_ae_gan_step_golden():
    z = load("step_ae_tiny")
    meta = jload(z, "meta")
    import vptr_amd.model as M
    enc = M.VPTREnc(meta["cimg"], meta["feat"], 3, "reflect")
    dec = M.VPTRDec(meta["cimg"], meta["feat"], 3, "Tanh", "reflect")
    disc = M.VPTRDisc(meta["cimg"], ndf=64, n_layers=3)
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 10)
    fill.apply_fill(disc, meta["seed"] + 20)
    st = O.AEStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(disc.state_dict()), lam_gan=meta["lam_gan"])
    shape = (meta["N"], meta["T"], meta["cimg"], meta["HW"], meta["HW"])
    for s, ref in enumerate(jload(z, "records")):
        past = (fill.rand_input(shape, meta["seed"] + 100 + s) - 0.6013795) / 2.7570653
        fut = (fill.rand_input(shape, meta["seed"] + 200 + s) - 0.6013795) / 2.7570653
        r = st.step(past, fut)
        for k in ref:
            assert abs(r[k] - ref[k]) <= 2e-4 * abs(ref[k]) + 1e-7, (k, r[k], ref[k])
    P = {"enc": st.P_enc, "dec": st.P_dec, "disc": st.P_disc}
    for k in z.files:
        if k.startswith("post:"):
            _, tag, name = k.split(":", 2)
            flat = P[tag][name].detach().flatten()
            assert rel(flat[::max(1, flat.numel() // 4096)], z[k]) < 1e-4, k


def test_metrics_match_reference_golden():
    from vptr_amd import metrics as M
    z = load("metrics_tiny")
    exp = jload(z, "expected")
    for tag, e in exp.items():
        x, y = torch.from_numpy(z["x:" + tag]), torch.from_numpy(z["y:" + tag])
        assert abs(M.PSNR(x, y) - e["psnr"]) < 1e-4 and abs(M.PSNR(x * 255, y * 255, 255) - e["psnr255"]) < 1e-4
        assert abs(M.MSEScore(x, y) - e["mse"]) < 1e-5 * abs(e["mse"])
        assert abs(float(M.SSIM()(x, y)) - e["ssim"]) < 2e-6
        assert np.allclose(M.SSIM(size_average=False)(x, y).numpy(), np.array(e["ssim_each"]), atol=2e-6)


def test_oracle_nar_gan_step_golden():
    z = load("step_nar_gan_tiny")
    cfg, meta = jload(z, "cfg"), jload(z, "meta")
    import vptr_amd.model as M
    enc = M.VPTREnc(1, meta["feat"], 3, "reflect")
    dec = M.VPTRDec(1, meta["feat"], 3, "Tanh", "reflect")
    disc = M.VPTRDisc(1, ndf=64, n_layers=3)
    T = build_transformer(M, cfg, False)
    fill.apply_fill(enc, meta["seed"])
    fill.apply_fill(dec, meta["seed"] + 10)
    fill.apply_fill(T, meta["seed"] + 20)
    fill.apply_fill(disc, meta["seed"] + 30)
    st = O.NARStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(T.state_dict()), cfg, P_disc=dict(disc.state_dict()),
                   lam_gan=meta["lam_gan"])
    for s, ref in enumerate(jload(z, "records")):
        past = (fill.rand_input((meta["N"], cfg["Tp"], 1, meta["HW"], meta["HW"]), meta["seed"] + 100 + s) - 0.6013795) / 2.7570653
        fut = (fill.rand_input((meta["N"], cfg["Tf"], 1, meta["HW"], meta["HW"]), meta["seed"] + 200 + s) - 0.6013795) / 2.7570653
        r = st.step(past, fut)
        for k in ref:
            assert abs(r[k] - ref[k]) <= 2e-4 * abs(ref[k]) + 1e-7, (k, r[k], ref[k])


def test_rollout_loops_match_reference_notebook_on_cpu():
    """The rollout LOOPS of vptr_amd.inference (model-agnostic host logic) driven with oracle-backed callables vs the tensors the
    reference's own notebook functions produced (tests/golden/rollouts_tiny.npz, see oracle/make_golden.py::rollout_case)."""
    from oracle import vptr_oracle as O
    from vptr_amd.inference import far_rollout, nar_bair_2_to_28, nar_rollout
    import vptr_amd.model as pkg
    z = load("rollouts_tiny")
    meta = jload(z, "meta")

    class Fn:
        def __init__(self, f, **attrs):
            self.f = f
            self.__dict__.update(attrs)

        def eval(self):
            return self

        def __call__(self, x):
            return self.f(x)

    def state(module, seed):
        fill.apply_fill(module, seed)
        return {k: v.detach().clone() for k, v in module.state_dict().items()}
    Pe = state(pkg.VPTREnc(1, meta["feat"], 3, "reflect"), meta["seed"])
    Pd = state(pkg.VPTRDec(1, meta["feat"], 3, "Sigmoid", "reflect"), meta["seed"] + 1)
    enc = Fn(lambda x: O.enc_forward(Pe, x))
    dec = Fn(lambda f: O.dec_forward(Pd, f, out_layer="Sigmoid"))
    cfg = jload(z, "cfg_far")
    Pf = state(build_transformer(pkg, cfg, True), meta["seed"] + 2)
    far = Fn(lambda f: O.far_forward(Pf, f, cfg), num_future_frames=cfg["Tf"])
    past = torch.from_numpy(z["far_past"])
    for mode, key in (("RIP", "far_rip"), ("RIL", "far_ril")):
        got = far_rollout(enc, dec, far, past, z[key].shape[1], mode=mode)
        assert got.shape == tuple(z[key].shape) and rel(got, z[key]) < 2e-5, (mode, rel(got, z[key]))
    cfgn = jload(z, "cfg_nar")
    Pn = state(build_transformer(pkg, cfgn, False), meta["seed"] + 5)
    nar = Fn(lambda f: O.nar_forward(Pn, f, cfgn), num_future_frames=cfgn["Tf"])
    got = nar_rollout(enc, dec, nar, torch.from_numpy(z["nar_past"]), rounds=2, chain="feats")
    assert rel(got, z["nar_chained"]) < 2e-5
    cfgb = jload(z, "cfg_bair")
    Pb = state(build_transformer(pkg, cfgb, False), meta["seed"] + 8)
    narb = Fn(lambda f: O.nar_forward(Pb, f, cfgb), num_future_frames=cfgb["Tf"])
    got = nar_bair_2_to_28(enc, dec, narb, torch.from_numpy(z["bair_past"]))
    assert got.shape == tuple(z["bair_frames"].shape) and rel(got, z["bair_frames"]) < 2e-5
    with pytest.raises(ValueError):
        nar_rollout(enc, dec, narb, torch.from_numpy(z["bair_past"]), rounds=2, chain="feats")   # Tf != Tp cannot chain features


def test_bench_refuses_fewer_devices_than_asked():
    """`python bench.py --gpus 2` on a host with fewer than 2 visible GPUs (this container has none) must exit non-zero with a clear
    message and print no result line -- never a silent one-GPU measurement labelled n_gpus 1"""
    import subprocess
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("this host can run --gpus 2")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VPTR_BENCH_SHARE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "GPU(s) visible" in (r.stderr + r.stdout) and "--gpus 2" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    # a launcher that brought up a different number of ranks than --gpus says is refused too, in either direction
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                       env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "does not match WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_refuses_zero_timed_steps():
    """--steps sets the number of timed steps, and ms_per_step is measured over them: a run with none is refused before any set-up"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("rows_mode", [128, 256])
@pytest.mark.parametrize("allow_sync", [True, False])
def test_wgrad_launch_plan_partitions_every_problem(rows_mode, allow_sync):
    """host logic of the grouped weight-gradient flush (vptr_amd.ops.plan_wgrad_launches, pure): whatever tile geometry is chosen, the
    sub-problems of the launches cover every (row, token) of every weight's gradient exactly once, with consistent operand / destination /
    bias-gradient addresses; a launch vouched for the panel-synchronous kernel walks one token count; the column sums of a flipped
    problem land in exactly one row range whose last tile has a free 16-row fragment."""
    from vptr_amd import ops
    F, C = 2112, 528
    shapes = [(F, C), (C, F), (C, C), (3 * C, C), (C, C), (F, C)]          # (N, K) of dW = dY^T X: fc1, fc2, projections, packed in_proj, ...
    probs, meta = [], {}
    addr = 1 << 20
    for li, tokens in enumerate((10240, 10240, 5120)):                      # two token counts: encoder / decoder layers of KTH128
        for (N, K) in shapes:
            flip = N < K and N % 176 == 0 and K % 128 != 0 and 128 - K % 128 >= 32      # the rule of ops._launch_wgrad_group
            rows, cols = (K, N) if flip else (N, K)
            ap, bp, dp, rp = addr, addr + (1 << 30), addr + (2 << 30), addr + (3 << 30)
            addr += 1 << 24
            lda, ldb, ldd = rows, cols, K                                    # token-major operands, dW [N][K]
            probs.append((ap, bp, dp, rp, lda, ldb, ldd, rows, cols, tokens, 1.0, flip))
            meta[dp] = (ap, bp, dp, rp, lda, ldb, ldd, rows, cols, tokens, flip)
    launches = ops.plan_wgrad_launches(probs, 176, True, 1, allow_sync, rows_mode)
    assert launches
    cover = {dp: [] for dp in meta}
    for subs, vouch in launches:
        trs = {(s[12] if len(s) > 12 else 128) for s in subs}
        assert len(trs) == 1, "one tile geometry per launch"
        tr = trs.pop()
        if vouch:
            assert allow_sync and len({s[9] for s in subs}) == 1, "a vouched launch walks one token count"
        for s in subs:
            (ap, bp, dp, rp, lda, ldb, ldd, rows, cols, tokens, alpha, flip) = s[:12]
            owner = max(k for k in meta if k <= dp)
            (ap0, bp0, dp0, rp0, lda0, ldb0, ldd0, rows0, cols0, tokens0, flip0) = meta[owner]
            assert (lda, ldb, ldd, cols, flip) == (lda0, ldb0, ldd0, cols0, flip0)
            r0 = ((dp - dp0) // 4) if flip else ((dp - dp0) // (4 * ldd))
            assert dp - dp0 == (r0 * 4 if flip else r0 * ldd * 4)
            da = ap - ap0                                                    # = token offset * lda * 4 + row offset * 4
            t0, rr = divmod(da // 4, lda)
            assert rr == r0 and da % 4 == 0 and bp - bp0 == t0 * ldb * 4
            assert 0 <= r0 and r0 + rows <= rows0 and 0 <= t0 and t0 + tokens <= tokens0 and t0 % 32 == 0
            if rp:
                assert rp == rp0 + (0 if flip else r0 * 4)
                if flip:   # column sums: the tile that holds the last rows of this range must have a free 16-row fragment
                    assert r0 + rows == rows0 and ((rows + tr - 1) // tr) * tr - rows >= 16, (rows, tr)
            elif not flip:
                raise AssertionError("a row range of a non-flipped problem lost its bias gradient")
            cover[owner].append((r0, rows, t0, tokens, bool(rp)))
    for dp0, pieces in cover.items():
        rows0, tokens0, flip0 = meta[dp0][7], meta[dp0][9], meta[dp0][10]
        assert sum(r * t for (_, r, _, t, _) in pieces) == rows0 * tokens0, "rows x tokens not covered exactly once"
        cells = set()
        for (r0, r, t0, t, _) in pieces:
            key = (r0, r, t0, t)
            assert key not in cells
            cells.add(key)
        row_ranges = sorted({(r0, r) for (r0, r, _, _, _) in pieces})
        assert row_ranges[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(row_ranges, row_ranges[1:])) and sum(r for _, r in row_ranges) == rows0
        for (r0, r) in row_ranges:
            toks = sorted((t0, t) for (a, b, t0, t, _) in pieces if (a, b) == (r0, r))
            assert toks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(toks, toks[1:])) and sum(t for _, t in toks) == tokens0
        if flip0:   # exactly one row range carries the column sums (once per token range)
            assert len({(r0, r) for (r0, r, _, _, has) in pieces if has}) == 1


def test_wgrad_launch_plan_cuts_small_groups_into_token_ranges():
    """one layer's weight (the launches of a torch.distributed job / torch.autograd.grad): 15 tiles become ~500 by token ranges of >= 1024
    tokens, all accumulating into the same destination"""
    from vptr_amd import ops
    C, tokens = 528, 10240
    prob = (1 << 20, 1 << 30, 2 << 30, 3 << 30, C, C, C, C, C, tokens, 1.0, False)
    (subs, vouch), = ops.plan_wgrad_launches([prob], 176, True, 1, True, 256)
    assert len(subs) == 10 and not any(len(s) > 12 and s[12] != 128 for s in subs)
    assert all(s[2] == prob[2] and s[3] == prob[3] for s in subs) and sum(s[9] for s in subs) == tokens and min(s[9] for s in subs) >= 1024
    (subs1, _), = ops.plan_wgrad_launches([prob], 176, True, 1, True, 256, token_split=False)
    assert len(subs1) == 1


def test_analytic_zero_class_is_an_allow_list():
    """every gradient the norm rule of helpers.analytic_zero classes as zero in a committed fixture carries a name from the explicit
    allow-list: a small-but-real gradient can not slip into the class"""
    import glob
    import json
    import numpy as np
    from helpers import analytic_zero
    classed = 0
    for f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.npz"))):
        z = np.load(f, allow_pickle=False)
        if "grad_norms" not in z.files:
            continue
        gn = json.loads(str(z["grad_norms"]))
        classed += sum(analytic_zero(gn[k], gn.values(), k) for k in gn)   # asserts inside on a name outside the list
    assert classed > 0


def test_winograd_filter_transform_matches_direct_convolution():
    """host side of the frozen encoder's Winograd path (vptr_amd/ops/conv.py::_WINO_G, the G of F(4x4, 3x3)) against the kernels' B^T and A^T
    (csrc/winograd.hip wino_bt6 / wino_at4, restated here): A^T [(G g G^T) . (B^T d B)] A == the direct 3 x 3 convolution of a 6 x 6 patch"""
    from vptr_amd.ops.conv import _WINO_G
    G = torch.tensor(_WINO_G, dtype=torch.float64)
    BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                       [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
    AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)
    g = torch.randn(5, 3, 3, 3, dtype=torch.float64)          # [Cout, Cin, 3, 3]
    d = torch.randn(1, 3, 6, 6, dtype=torch.float64)
    U = torch.einsum("ia,kcab,jb->ijkc", G, g, G)             # as ops.wino_filter
    V = torch.einsum("ij,cjk,lk->ilc", BT, d[0], BT)          # B^T d B per channel
    M = torch.einsum("ijkc,ijc->ijk", U, V)
    Y = torch.einsum("ai,ijk,bj->kab", AT, M, AT)             # [Cout, 4, 4]
    ref = torch.nn.functional.conv2d(d, g)[0]
    assert float((Y - ref).abs().max()) < 1e-12


# ---- the fp64 reference builders of the stage-1 / TSLMA op tests, each against an independent formulation ----------------------------------
@pytest.mark.parametrize("K,stride,pad,pad_mode", [(3, 1, 1, "zero"), (3, 2, 1, "zero"), (4, 2, 1, "zero"), (4, 1, 1, "zero"), (3, 1, 1, "reflect"),
                                                   (7, 1, 3, "reflect")])
def test_unfold_kkc_is_the_conv_patch_matrix(K, stride, pad, pad_mode):
    """helpers.unfold_kkc: patches [(b, oy, ox), (ky, kx, c)] @ weight[(co), (ky, kx, ci)]^T == F.conv2d on a non-square map (a swapped ky / kx
    or a channel-major column order would not)"""
    import torch.nn.functional as F
    from helpers import unfold_kkc
    B, C, Co, H, W = 2, 3, 5, 9, 7
    x, w = fill.rand_normal((B, C, H, W), 1).double(), fill.rand_normal((Co, C, K, K), 2).double()
    xp = F.pad(x, (pad,) * 4, mode="reflect") if pad_mode == "reflect" else F.pad(x, (pad,) * 4)
    ref = F.conv2d(xp, w, stride=stride)
    P = unfold_kkc(x, K, K, stride, pad, pad_mode)
    assert P.shape == (B * ref.shape[2] * ref.shape[3], K * K * C)
    out = (P @ w.permute(0, 2, 3, 1).reshape(Co, -1).t()).reshape(B, ref.shape[2], ref.shape[3], Co).permute(0, 3, 1, 2)
    assert rel(out, ref) < 1e-14


def test_ts_gather_matches_oracle_tslma():
    """helpers.ts_gather / ts_scatter (explicit index gather by window) + O._heads + O._attend == the inner nn.MultiheadAttention of O.tslma
    (which goes through O._ts_permute's pad / reshape / permute) on a tiny non-square case with several windows per frame and Tq != Tk"""
    import torch.nn.functional as F
    from helpers import ts_gather, ts_rows, ts_scatter
    N, T1, T2, H, W, ws, C, nh = 2, 3, 2, 4, 6, 2, 12, 3
    P = {"a.attn.in_proj_weight": fill.rand_normal((3 * C, C), 3, C ** -0.5).double(), "a.attn.in_proj_bias": fill.rand_normal((3 * C,), 4).double(),
         "a.attn.out_proj.weight": fill.rand_normal((C, C), 5, C ** -0.5).double(), "a.attn.out_proj.bias": fill.rand_normal((C,), 6).double()}
    mem, query = fill.rand_normal((N, T1, H, W, C), 7).double(), fill.rand_normal((N, T2, H, W, C), 8).double()
    Tlw = fill.rand_normal((T1 + T2, ws, ws, C), 9).double()
    ref = O.tslma(P, "a.", mem, query, Tlw, ws, nh)
    rows = ts_rows(N, T2, H, W, ws)
    assert sorted(rows.reshape(-1).tolist()) == list(range(N * T2 * H * W))            # a permutation of all tokens
    Wq, Wk, Wv = P["a.attn.in_proj_weight"].chunk(3)
    bq, bk, bv = P["a.attn.in_proj_bias"].chunk(3)
    qw = ts_gather(query.reshape(-1, C), N, T2, H, W, ws) + Tlw[T1:].reshape(1, -1, C)
    mw = ts_gather(mem.reshape(-1, C), N, T1, H, W, ws)
    q = F.linear(qw, Wq, bq) * (C // nh) ** -0.5
    k, v = F.linear(mw + Tlw[:T1].reshape(1, -1, C), Wk, bk), F.linear(mw, Wv, bv)
    o = O._attend(O._heads(q, nh), O._heads(k, nh), O._heads(v, nh))
    o = F.linear(ts_scatter(o, N, T2, H, W, ws), P["a.attn.out_proj.weight"], P["a.attn.out_proj.bias"])
    assert rel(o, ref.reshape(-1, C)) < 1e-13
    x = fill.rand_normal((N * T2 * H * W, C), 10)
    assert torch.equal(ts_scatter(ts_gather(x, N, T2, H, W, ws), N, T2, H, W, ws), x)


@pytest.mark.parametrize("H,W,pad", [(5, 7, 1), (2, 3, 1), (4, 6, 3), (8, 5, 3), (6, 6, 2)])
def test_reflect_fold_ref_is_the_adjoint_of_reflection_padding(H, W, pad):
    """helpers.reflect_fold_ref == torch.autograd.grad of F.pad(mode="reflect"), down to H = pad + 1 (a border pixel with three pre-images)"""
    import torch.nn.functional as F
    from helpers import reflect_fold_ref
    x = fill.rand_normal((2, 3, H, W), 11).double().requires_grad_(True)
    g = fill.rand_normal((2, 3, H + 2 * pad, W + 2 * pad), 12).double()
    (ref,) = torch.autograd.grad(F.pad(x, (pad,) * 4, mode="reflect"), x, g)
    assert rel(reflect_fold_ref(g, pad), ref) < 1e-15


# ---- the fp64 reference builders of the deferred-backward op tests (tests/test_09b_deferred_bwd_gpu.py) --------------------------------------------
def _ln_closed_form(g, xhat, wgt, rstd, dims):
    """rstd * (g*w - mean(g*w) - xhat * mean(g*w*xhat)), the means over `dims`"""
    gw = g * wgt
    return rstd * (gw - gw.mean(dims, keepdim=True) - xhat * (gw * xhat).mean(dims, keepdim=True))


@pytest.mark.parametrize("with_dy2,with_add", [(True, True), (False, False), (False, True)])
@pytest.mark.parametrize("rows,C", [(37, 48), (9, 260)])
def test_ln_bwd_ref_matches_closed_form(rows, C, with_dy2, with_add):
    """helpers.ln_bwd_ref (autograd of F.layer_norm) == the closed form with explicit statistics, dy2 and dx_add included"""
    from helpers import ln_bwd_ref
    x, gamma = fill.rand_normal((rows, C), 21, 2.0) + 0.3, fill.rand_normal((C,), 22).abs() + 0.5
    dy = fill.rand_normal((rows, C), 23)
    dy2 = fill.rand_normal((rows, C), 24) if with_dy2 else None
    add = fill.rand_normal((rows, C), 25) if with_add else None
    ref = ln_bwd_ref(x, gamma, dy, dy2, add)
    xd = x.double()
    mean = xd.sum(1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).sum(1, keepdim=True) / C + 1e-5)
    xhat = (xd - mean) * rstd
    g = dy.double() + (dy2.double() if with_dy2 else 0.0)
    dx = _ln_closed_form(g, xhat, gamma.double(), rstd, 1) + (add.double() if with_add else 0.0)
    assert rel(ref["dx"], dx) < 1e-10
    assert rel(ref["dgamma"], (g * xhat).sum(0)) < 1e-10 and rel(ref["dbeta"], g.sum(0)) < 1e-10
    assert rel(ref["mean"], mean[:, 0]) < 1e-10 and rel(ref["rstd"], rstd[:, 0]) < 1e-10


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_norm_act_ln_bwd_ref_matches_closed_form(act, p):
    """helpers.norm_act_ln_bwd_ref (autograd, channel-last [HW, F] affine) == the closed form written in the module's own NCHW layout:
    statistics over (F, H, W) of a [frames, F, H, W] tensor, affine parameters as (F, H, W), analytic activation derivatives, mask / keep
    and the per-row scale folded into the upstream gradient (a transposed affine, a mask on the wrong side of the activation or a row
    scale indexed by frame instead of by row would not agree)"""
    from helpers import KINK, norm_act_ln_bwd_ref
    frames, H, W, Fc = 5, 2, 3, 8
    HW, rows = H * W, frames * H * W
    x, dy = fill.rand_normal((rows, Fc), 31, 2.0) + 0.3, fill.rand_normal((rows, Fc), 32)
    w, b = fill.rand_normal((HW, Fc), 33).abs() + 0.5, fill.rand_normal((HW, Fc), 34, 0.3)
    rs = torch.tensor([1.25, 0.0, 1.25])
    rs_div, rs_mod = 4, 3                                                # runs of 4 rows: not the frame length
    mask = (fill.rand_input((rows, Fc), 35) >= p).float() if p > 0 else None
    ref = norm_act_ln_bwd_ref(x, w, b, dy, frames, HW, act, mask, 1.0 - p, rs, rs_div, rs_mod)

    def nchw(t):
        return t.double().reshape(-1, H, W, Fc).permute(0, 3, 1, 2)
    x4, w4, b4 = nchw(x), nchw(w)[0], nchw(b)[0]
    n = Fc * H * W
    mean = x4.sum((1, 2, 3), keepdim=True) / n
    rstd = 1.0 / torch.sqrt(((x4 - mean) ** 2).sum((1, 2, 3), keepdim=True) / n + 1e-5)
    xhat = (x4 - mean) * rstd
    pre = xhat * w4 + b4
    if act == 1:
        slope = 0.5 * (1.0 + torch.erf(pre / 2 ** 0.5)) + pre * torch.exp(-0.5 * pre * pre) / (2 * np.pi) ** 0.5
    else:
        slope = (pre > 0).double() if act == 2 else torch.ones_like(pre)
    g = nchw(dy)
    if act == 2:
        g = torch.where(pre.abs() < KINK * (pre ** 2).mean().sqrt(), torch.zeros_like(g), g)
    scale = nchw(rs.double()[(torch.arange(rows) // rs_div) % rs_mod][:, None].expand(rows, Fc))
    if p > 0:
        scale = scale * nchw(mask) / (1.0 - p)
    g = g * scale * slope
    dx = _ln_closed_form(g, xhat, w4, rstd, (1, 2, 3))

    def cl(t):      # [.., F, H, W] -> channel-last rows
        return t.permute(*range(t.dim() - 3), -2, -1, -3).reshape(-1, Fc)
    assert rel(ref["dx"], cl(dx)) < 1e-10
    assert rel(ref["dw"], cl((g * xhat).sum(0))) < 1e-10 and rel(ref["db"], cl(g.sum(0))) < 1e-10
    assert rel(ref["mean"], mean.reshape(-1)) < 1e-10 and rel(ref["rstd"], rstd.reshape(-1)) < 1e-10
    assert rel(ref["pre"], cl(pre)) < 1e-10


def test_deferred_bwd_cases_input_conditions():
    """conditions on the seeded inputs of the LayerNorm((F,H,W)) backward cases that need no GPU: the share of ReLU pre-activations next to the
    kink stays under the cap of the kink rule, and the DropPath-like row scale has both dropped and kept frames"""
    from helpers import KINK, KINK_CAP, NORM_ACT_LN_CASES, norm_act_ln_inputs
    for case in sorted(NORM_ACT_LN_CASES):
        _, frames, HW, Fc = NORM_ACT_LN_CASES[case]
        x, dy, w, b, rs = norm_act_ln_inputs(case)
        pre = torch.nn.functional.layer_norm(x.double().view(frames, HW, Fc), (HW, Fc), w.double(), b.double(), 1e-5)
        share = float((pre.abs() < KINK * pre.pow(2).mean().sqrt()).double().mean())
        assert share <= KINK_CAP, (case, share)
        assert 0 < int((rs == 0).sum()) < frames, case


# ---- the attention cores through the C ABI (tests/test_00b_attn_abi_gpu.py): reference builders, P16 encoder, head classes, emulated cases ---------
def _sdpa_heads(t, nh):
    P, L, C = t.shape
    return t.reshape(P, L, nh, C // nh).transpose(1, 2)


@pytest.mark.parametrize("with_table", [True, False])
def test_win_attn_ref_matches_sdpa(with_table):
    """helpers.win_attn_ref (O.win_partition + O._heads + O._attend) == F.scaled_dot_product_attention in fp64 with scale = 1 and the bias as an
    additive mask, on windows gathered by explicit row indices (helpers.ts_rows with T = 1), non-square map, several windows per frame;
    gradients by autograd of that formulation, dq times dq_scale"""
    import torch.nn.functional as F
    from helpers import ts_rows, win_attn_ref
    B, H, W, ws, nh, C = 2, 4, 6, 2, 3, 12
    L, n, sc = ws * ws, B * H * W, 0.37
    q, k, v, go = (fill.rand_normal((n, C), 40 + i, 0.5 if i < 2 else 1.0) for i in range(4))
    table, idx = (fill.rand_normal(((2 * ws - 1) ** 2, nh), 44, 0.5), O.rpe_index(ws)) if with_table else (None, None)
    ref = win_attn_ref(q, k, v, go, B, H, W, nh, ws, table, idx, None, sc)
    rows = ts_rows(B, 1, H, W, ws).reshape(-1)
    ins = [t.double().requires_grad_(True) for t in ((q, k, v, table) if with_table else (q, k, v))]
    g = [_sdpa_heads(t[rows].reshape(-1, L, C), nh) for t in ins[:3]]
    bias = ins[3][idx.reshape(-1)].reshape(L, L, nh).permute(2, 0, 1) if with_table else None
    o = F.scaled_dot_product_attention(g[0], g[1], g[2], attn_mask=bias, scale=1.0).transpose(1, 2).reshape(-1, C)
    full = torch.zeros(n, C, dtype=torch.float64).index_add(0, rows, o)
    grads = torch.autograd.grad((full * go.double()).sum(), ins)
    assert rel(ref["o"], full) < 1e-13
    assert rel(ref["dq"], grads[0] * sc) < 1e-12 and rel(ref["dk"], grads[1]) < 1e-12 and rel(ref["dv"], grads[2]) < 1e-12
    if with_table:
        assert rel(ref["dtable"], grads[3]) < 1e-12


@pytest.mark.parametrize("Tq,Tk,causal", [(5, 5, True), (3, 7, False)])
def test_temporal_attn_ref_matches_sdpa(Tq, Tk, causal):
    """helpers.temporal_attn_ref == F.scaled_dot_product_attention (fp64, scale = 1, causal as an additive -inf mask) per (n, pixel) sequence
    gathered by explicit row arithmetic (row = (n * T + t) * HW + pixel)"""
    import torch.nn.functional as F
    from helpers import temporal_attn_ref
    N, HW, nh, C, sc = 2, 3, 2, 8, 0.5
    q, go = fill.rand_normal((N * Tq * HW, C), 50, 0.5), fill.rand_normal((N * Tq * HW, C), 53)
    k, v = fill.rand_normal((N * Tk * HW, C), 51, 0.5), fill.rand_normal((N * Tk * HW, C), 52)
    ref = temporal_attn_ref(q, k, v, go, N, Tq, Tk, HW, nh, causal, None, sc)

    def rows(T):
        n, p, t = torch.meshgrid(torch.arange(N), torch.arange(HW), torch.arange(T), indexing="ij")
        return ((n * T + t) * HW + p).reshape(-1)
    ins = [t.double().requires_grad_(True) for t in (q, k, v)]
    g = [_sdpa_heads(t[rows(T)].reshape(N * HW, T, C), nh) for t, T in zip(ins, (Tq, Tk, Tk))]
    am = torch.zeros(Tq, Tk, dtype=torch.float64).masked_fill(torch.arange(Tk)[None, :] > torch.arange(Tq)[:, None], float("-inf")) if causal else None
    o = F.scaled_dot_product_attention(g[0], g[1], g[2], attn_mask=am, scale=1.0).transpose(1, 2).reshape(-1, C)
    full = torch.zeros(N * Tq * HW, C, dtype=torch.float64).index_add(0, rows(Tq), o)
    grads = torch.autograd.grad((full * go.double()).sum(), ins)
    assert rel(ref["o"], full) < 1e-13
    assert rel(ref["dq"], grads[0] * sc) < 1e-12 and rel(ref["dk"], grads[1]) < 1e-12 and rel(ref["dv"], grads[2]) < 1e-12


def test_win_attn_ref_gradients_gradcheck():
    """the differentiable forward behind helpers.win_attn_ref on 2 windows of head dim 4 with a bias table and a dropout mask: analytic vs
    numerical Jacobians (torch.autograd.gradcheck, fp64), and win_attn_ref's gradients == autograd.grad of that forward"""
    from helpers import win_attn_fwd64, win_attn_ref
    B, H, W, ws, nh, C = 1, 2, 4, 2, 2, 8
    n = B * H * W
    q, k, v, go = (fill.rand_normal((n, C), 60 + i, 0.5 if i < 2 else 1.0) for i in range(4))
    table, idx = fill.rand_normal((9, nh), 64, 0.5), O.rpe_index(ws)
    mask = (fill.rand_input((2, nh, 4, 4), 65) >= 0.2).double() / 0.8
    ins = [t.double().requires_grad_(True) for t in (q, k, v, table)]
    assert torch.autograd.gradcheck(lambda a, b, c, d: win_attn_fwd64(a, b, c, d, B, H, W, nh, ws, idx, mask), ins, eps=1e-6, atol=1e-7, rtol=1e-5)
    grads = torch.autograd.grad((win_attn_fwd64(*ins, B, H, W, nh, ws, idx, mask) * go.double()).sum(), ins)
    ref = win_attn_ref(q, k, v, go, B, H, W, nh, ws, table, idx, mask, 0.5)
    assert rel(ref["dq"], grads[0] * 0.5) < 1e-14 and rel(ref["dk"], grads[1]) < 1e-14 and rel(ref["dv"], grads[2]) < 1e-14
    assert rel(ref["dtable"], grads[3]) < 1e-14


def test_p16_encode_round_trip():
    """helpers.p16_encode (plain torch: hi = bf16(x) to nearest, lo = bf16(x - hi), 16 hi then 16 lo per granule) against the decoder: the byte
    layout (hi plane alone = bf16(x)), and the round trip within 2^-17 relative per element on seeded data over 12 binades"""
    from helpers import p16_encode
    from attn_abi_cases import p16_decode
    x = fill.rand_normal((37, 48), 70) * torch.exp2(torch.arange(-6, 6).repeat(4).float())[None, :]
    enc = p16_encode(x)
    assert enc.shape == x.shape and enc.dtype == torch.float32
    planes = enc.view(torch.bfloat16).reshape(37, 3, 2, 16)
    assert torch.equal(planes[:, :, 0].reshape(37, 48), x.to(torch.bfloat16))
    dec = p16_decode(enc)
    assert float(((dec.double() - x.double()).abs() / x.double().abs()).max()) <= 2.0 ** -17
    try:
        from vptr_amd.ops.core import p16_decode as lib_decode        # needs the built library; the restated decoder must be the same function
    except (ImportError, OSError):
        return
    assert torch.equal(lib_decode(enc), dec)


def test_attn_head_dims_cover_every_class():
    """(nb32, nb16) of every even head dim 2 .. 98, plain (first-generation attn16, attn_mfma) and of the second-generation span: the head dims
    of the C-ABI cases reach every instantiation that some admissible hd <= 96 reaches, in both chains; the (4, 7) branch of attn16_fwd2 /
    attn16_bwd2 is reached by no admissible head dim (span <= 96 always: hd = 94 has span 96, hd = 96 % 4 == 0)"""
    from attn_abi_cases import HEAD_CLASSES
    from helpers import attn_head_classes
    reach_plain = {attn_head_classes(hd)[0] for hd in range(2, 97, 2)}
    reach_gen2 = {attn_head_classes(hd)[1] for hd in range(2, 97, 2)}
    assert reach_plain == reach_gen2 == {(1, 1), (1, 2), (2, 3), (2, 4), (3, 5), (3, 6)}
    assert (4, 7) not in reach_gen2 and attn_head_classes(98)[1] == (4, 7)        # only hd = 98 would, and attn16_ok refuses hd > 96
    hds = [C // nh for nh, C in HEAD_CLASSES.values() if C // nh <= 96]
    assert {attn_head_classes(hd)[0] for hd in hds} == reach_plain and {attn_head_classes(hd)[1] for hd in hds} == reach_gen2
    assert attn_head_classes(94) == ((3, 6), (3, 6)) and attn_head_classes(66) == ((3, 5), (3, 5)) and attn_head_classes(30) == ((1, 2), (1, 2))
    assert attn_head_classes(14) == ((1, 1), (1, 1)) and attn_head_classes(62) == ((2, 4), (2, 4)) and attn_head_classes(46) == ((2, 3), (2, 3))
    # the library's own ladder (vptr_attn_route, T = 5 with nh = 2: C % 4 == 0): first generation under VPTR_ATTN16=2, second in the default routing
    from helpers import attn_kernel_mode, attn_route
    for hd in range(2, 97, 2):
        with attn_kernel_mode("attn16"):
            assert attn_route(1, 5, 5, 2 * hd, 2) == ("a16_gen1", attn_head_classes(hd)[0], 0), hd
        with attn_kernel_mode("mfma"):
            assert attn_route(1, 5, 5, 2 * hd, 2) == ("am_plain", attn_head_classes(hd)[0], 0), hd
        with attn_kernel_mode("default"):
            assert attn_route(1, 5, 5, 2 * hd, 2) == ("a16_gen2", attn_head_classes(hd)[1], 0), hd
            assert attn_route(1, 5, 5, 2 * hd, 2, backward=1) == ("a16_gen2", attn_head_classes(hd)[1], 0), hd
    for mode in ("default", "attn16", "mfma"):               # hd 98: refused by both matrix-unit families
        with attn_kernel_mode(mode):
            assert attn_route(1, 5, 5, 196, 2)[:2] == ("vector16", (0, 0)) and attn_route(1, 20, 20, 196, 2)[:2] == ("vector", (0, 0))


def _emu():
    from attn_abi_cases import EmuBackend
    return EmuBackend()


@pytest.mark.parametrize("geom", ["win4_B3_8x8_bias", "win8_B1_8x16", "win2_B2_4x6_generic", "t5x5_causal", "t3x7", "t20x20_causal_2qblocks",
                                  "t40x33_tileshare"])
@pytest.mark.parametrize("hc", ["hd24_c12", "hd94_oddpair_span96"])
def test_attn_abi_cases_against_emulation(hc, geom):
    """the direct-call cases of tests/test_00b_attn_abi_gpu.py against a CPU emulation of the C-ABI calls (closed-form backward per head, explicit
    row gathers, P16 outputs through helpers.p16_encode): argument order, layouts, guards, references and bars of the CASES, not the kernels"""
    import attn_abi_cases as A
    nh, C = A.HEAD_CLASSES[hc]
    A.run_parity(_emu(), A.GEOMS[geom], nh, C)


@pytest.mark.parametrize("geom", ["win4_B3_8x8_bias", "win8_B1_8x16", "t5x5_causal", "t3x7", "t20x20_causal_2qblocks"])
def test_attn_abi_dropout_conditions_hold_for_the_oracle(geom):
    """the dropout cases with a stand-in Bernoulli mask of the same shape: zero share in (0.08, 0.12) (the smallest mask, 3 windows x 2 heads x
    16 x 16 = 1536 elements, puts 3 sigma at +-0.023) and a mask-free reference more than 10 x 5e-5 away -- both asserted inside run_dropout"""
    import attn_abi_cases as A
    assert sorted(A.DROP_GEOMS) == sorted(["win4_B3_8x8_bias", "win8_B1_8x16", "t5x5_causal", "t3x7", "t20x20_causal_2qblocks"])
    for hc in A.DROP_HEADS:
        nh, C = A.HEAD_CLASSES[hc]
        A.run_dropout(_emu(), A.GEOMS[geom], nh, C)


def test_attn_abi_contract_cases_against_emulation():
    """table-gradient accumulation, NULL table gradient, the workspace entry point (on the 65-window geometry), TSLMA with P16 outputs, the two
    cases on tensors 8 bytes off the 16-byte grid, the nh = 3 slot-tail cases and the argument guards, emulated"""
    import attn_abi_cases as A
    from helpers import TS_GEOMS
    be = _emu()
    for g in A.TABLE_GEOMS.values():
        A.run_table_contract(be, g, 2, 48)
    A.run_workspace_contract(be, A.LAUNCH_CASES["win4_65win_wpb2_tail"][0], 2, 48)
    A.run_tslma(be, *TS_GEOMS[1])
    A.run_unaligned(be, A.GEOMS["win4_B3_8x8_bias"], 2, 48)
    A.run_unaligned(be, A.GEOMS["t5x5_causal"], 8, 528)
    for name in ("mfma_win4_15prob_4slots", "mfma_t20_15prob_2slots", "mfma_t40_9prob_1slot", "win4_65win_wpb2_tail"):
        geom, hcs, _ = A.LAUNCH_CASES[name]
        A.run_parity(be, geom, *hcs[0])

    def raises(fn):
        with pytest.raises(RuntimeError):
            fn()
    A.run_guards(be, raises)


def test_attn_abi_case_geometries():
    """the launch-class cases have the problem counts their ids promise (1547 = 3 mod 4 = 3 mod 8 windows above every attn16 grid, 65, 2139 =
    3 mod 4 windows, 1551 pixels), and the <true> / <false> split of the 16-token temporal vector kernels falls between T = 11 and T = 12 at hd 66
    (T = 10, the model's, and T = 11 take the prefetching variant, T = 16 the other)"""
    import attn_abi_cases as A
    P = {name: A.problem_dims(g, 0)[0] for name, (g, _, _) in A.LAUNCH_CASES.items()}
    assert P["win4_1547win_loop_wpb8_tail"] == 1547 and 1547 % 4 == 3 and 1547 % 8 == 3 and 1547 > 3072 // 2 and 1547 > 768
    assert P["win4_65win_wpb2_tail"] == 65 and P["win2_2139win_generic_wpb4_tail"] == 2139 and 2139 % 4 == 3 and 2139 >= 2048
    assert P["t5_causal_1551px_4px_per_wave"] == P["t10_hd66_1551px_pf"] == P["t11_hd66_1551px_pf_limit"] == P["t16_hd66_1551px_no_pf"] == 1551

    def att_pitch(hd):
        q = (hd + 3) // 4
        return (q + 1 if q % 2 == 0 else q) * 4
    assert att_pitch(66) == 68 and 11 * att_pitch(66) // 2 <= 384 < 12 * att_pitch(66) // 2 and 16 * att_pitch(66) // 2 > 384
    assert P["mfma_win4_15prob_4slots"] * 3 % 4 != 0 and P["mfma_t20_15prob_2slots"] * 3 % 2 != 0
    # the library's own split (vptr_attn_route, fp32 vector kernels, hd 66 at 1551 pixels): prefetching variant up to T = 11; not below 256 pixels
    from helpers import ATTN_MODES, attn_geom_route, attn_kernel_mode, attn_route
    with attn_kernel_mode("vector"):
        for T in range(1, 17):
            for backward in (0, 1):
                assert attn_route(1, T, T, 132, 2, groups=1551, backward=backward) == ("vector16", (0, 0), int(T * att_pitch(66) // 2 <= 384)), T
        assert attn_route(1, 11, 11, 132, 2, groups=1551)[2] == 1 and attn_route(1, 12, 11, 132, 2, groups=1551)[2] == 0
        assert attn_route(1, 10, 10, 132, 2, groups=256)[2] == 1 and attn_route(1, 10, 10, 132, 2, groups=255)[2] == 0
    # every id of the GPU file reaches, in its mode, the family that the id, the mode (helpers.attn_kernel_mode) and head_modes promise
    A16, AM, VEC = {"a16_gen1", "a16_gen2"}, {"am_plain", "am_shared"}, {"vector", "vector16"}

    def promised(mode, geom, hd):
        """(forward, backward) family; geometry ids: "generic" = no 16-token kernel, "2qblocks" / "tileshare" = more than one query block"""
        Lq, Lk = (geom[4] ** 2, geom[4] ** 2) if geom[0] == "win" else geom[2:4]
        rows = max(Lq, Lk)
        small = rows <= 16 and (geom[0] == "t" or geom[4] == 4)          # what the 16-token kernels (attn16.hip, vector) take
        vec = "vector16" if small and (geom[0] == "t" or hd <= 92) else "vector"
        am = ("am_plain", "am_shared" if Lq > 16 else "am_plain")
        if hd > 96 or mode == "vector":
            return vec, vec
        if mode == "mfma" or rows > 16:
            return am
        if not small:
            return "vector", "vector"
        return {"default": ("a16_gen2", "a16_gen2"), "attn16": ("a16_gen1", "a16_gen1"), "attn16fwd": ("a16_gen1", vec)}[mode]
    cases = [(A.GEOMS[g], nh, C, m, g + " " + hc) for hc, (nh, C) in A.HEAD_CLASSES.items() for g in A.GEOMS for m in A.head_modes(hc, ATTN_MODES)]
    cases += [(g, nh, C, m, name) for name, (g, hcs, modes) in A.LAUNCH_CASES.items() for nh, C in hcs for m in (modes or ATTN_MODES)]
    for geom, nh, C, mode, name in cases:
        assert C % 4 == 0
        with attn_kernel_mode(mode):
            got = attn_geom_route(geom, nh, C, 0), attn_geom_route(geom, nh, C, 1)
        assert (got[0][0], got[1][0]) == promised(mode, geom, C // nh), (name, mode, got)
        fams = {got[0][0], got[1][0]}
        if "over_limit_vector" in name or "generic" in name and mode != "mfma":
            assert fams <= VEC and ("generic" not in name or fams == {"vector"}), (name, mode, got)
        if name.startswith("mfma_") or ("2qblocks" in name or "tileshare" in name) and mode != "vector" and "over_limit" not in name:
            assert fams <= AM and got[1][0] == ("am_plain" if "4slots" in name else "am_shared"), (name, mode, got)
        if "_pf" in name and mode in ("vector", "attn16fwd"):        # the backward runs the 16-token temporal vector kernels in both modes
            assert got[1][0] == "vector16" and got[1][2] == int("no_pf" not in name), (name, mode, got)
        if name.startswith("win4_1547win") and mode == "default":
            assert fams == {"a16_gen2"}
        if name.startswith("win4_65win"):
            assert mode == "vector" and fams == {"vector16"}


def test_winattn16_register_tile_covers_the_lds_tile():
    """index arithmetic of csrc/attn.hip's rows16_load / rows16_store restated: 256 threads x 3 items stage a 16 x (pitch / 2) float2 tile, so the
    16-token window kernels may serve a head dim only while 16 * att_pitch(hd) / 2 <= 768 (rows16_fits in the launchers): hd <= 92.  At hd 94 / 96 /
    98 (pitch 100) row 15 would keep columns 36 .. 99 of whatever the LDS held -- the defect tests/test_00b_attn_abi_gpu.py found at hd 96"""
    def att_pitch(hd):
        q = (hd + 3) // 4
        return (q + 1 if q % 2 == 0 else q) * 4

    def staged(hd):            # (row, float2 column) pairs the three items of 256 threads write
        h2 = att_pitch(hd) // 2
        return {(e // h2, e % h2) for e in range(3 * 256) if e // h2 < 16}
    for hd in range(2, 130, 2):
        h2 = att_pitch(hd) // 2
        whole = staged(hd) == {(l, d) for l in range(16) for d in range(h2)}
        assert whole == (16 * h2 <= 768) == (hd <= 92), hd
    missing = {(l, d) for l in range(16) for d in range(50)} - staged(96)
    assert missing == {(15, d) for d in range(18, 50)}
    # the library's own limit (vptr_attn_route): 4 x 4 windows on the fp32 vector kernels take the 16-token ones up to hd 92, forward and backward
    from helpers import attn_kernel_mode, attn_route
    with attn_kernel_mode("vector"):
        for hd in range(2, 130, 2):
            for backward in (0, 1):
                assert attn_route(0, 16, 16, 2 * hd, 2, ws=4, groups=12, backward=backward)[0] == ("vector16" if hd <= 92 else "vector"), hd


# ---- the conv-FFN forward kernels through the C ABI (tests/test_09c_convffn_fwd_gpu.py): reference builders, launch classes, the one-pass
# variance in fp32, emulated cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2])
def test_convffn_fwd_refs_match_the_nchw_modules(act):
    """helpers.norm_act_fwd_ref / dwconv_norm_fwd_ref (channel-last rows, [HW, F] affine, tap-major [9, F] weights) == the modules' own NCHW
    formulation: nn.LayerNorm((F, H, W)) or F.batch_norm on [frames, F, H, W], the activation, mask / keep, the per-row scale, the residual,
    F.conv2d with the [F, 1, 3, 3] parameter"""
    import torch.nn.functional as Fn
    from helpers import dwconv_norm_fwd_ref, norm_act_fwd_ref
    frames, H, W, Fc = 5, 2, 3, 8
    HW, rows = H * W, frames * H * W
    x, res = fill.rand_normal((rows, Fc), 41, 2.0) + 0.3, fill.rand_normal((rows, Fc), 42)
    w, b = fill.rand_normal((HW, Fc), 43).abs() + 0.5, fill.rand_normal((HW, Fc), 44, 0.3)
    mask = (fill.rand_input((rows, Fc), 45) >= 0.1).float()
    rs, rs_div, rs_mod = torch.tensor([1.25, 0.0, 0.7]), 4, 3                # runs of 4 rows: not the frame length

    def nchw(t):
        return t.double().reshape(-1, H, W, Fc).permute(0, 3, 1, 2)

    def cl(t):
        return t.permute(0, 2, 3, 1).reshape(-1, Fc)

    def actf(t):
        return Fn.gelu(t) if act == 1 else (torch.relu(t) if act == 2 else t)
    tail = nchw(mask) / 0.9 * nchw(rs.double()[(torch.arange(rows) // rs_div) % rs_mod][:, None].expand(rows, Fc))
    ln = torch.nn.LayerNorm((Fc, H, W), eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(nchw(w)[0])
        ln.bias.copy_(nchw(b)[0])
        pre = ln(nchw(x))
        got = norm_act_fwd_ref(x, w, b, HW, False, act, mask, 0.9, rs, rs_div, rs_mod, res)
        assert rel(got["y"], cl(actf(pre) * tail + nchw(res))) < 1e-10 and rel(got["pre"], cl(pre)) < 1e-10
        x4 = nchw(x)
        assert rel(got["mean"], x4.mean((1, 2, 3))) < 1e-10 and rel(got["rstd"], (x4.var((1, 2, 3), unbiased=False) + 1e-5).rsqrt()) < 1e-10
        # BatchNorm2d batch statistics, affine [F]
        wc, bc = w[0], b[0]
        pre = Fn.batch_norm(x4, None, None, wc.double(), bc.double(), True, 0.1, 1e-5)
        got = norm_act_fwd_ref(x, wc, bc, 1, True, act, mask, 0.9, rs, rs_div, rs_mod, res)
        assert rel(got["y"], cl(actf(pre) * tail + nchw(res))) < 1e-10
        assert rel(got["mean"], x4.mean((0, 2, 3))) < 1e-10 and rel(got["rstd"], (x4.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()) < 1e-10
        # the fused operator
        wt, b9 = fill.rand_normal((Fc, 1, 3, 3), 46, 0.3), fill.rand_normal((Fc,), 47, 0.3)
        a = actf(ln(x4))
        y = Fn.conv2d(a, wt.double(), b9.double(), padding=1, groups=Fc)
        got = dwconv_norm_fwd_ref(x, w, b, wt.reshape(Fc, 9).t().contiguous(), b9, frames, H, W, act)
        assert rel(got["y"], cl(y)) < 1e-10 and rel(got["a"], cl(a)) < 1e-10
        assert rel(got["sum"], y.sum((1, 2, 3))) < 1e-10 and rel(got["sumsq"], (y * y).sum((1, 2, 3))) < 1e-10
        assert rel(got["mean"], x4.mean((1, 2, 3))) < 1e-10


def test_convffn_fwd_cases_land_in_their_launch_classes():
    """the launchers' selection arithmetic restated (helpers.convffn_fwd_class): every geometry of tests/convffn_fwd_cases.py reaches the kernel,
    the grid, the trip count and the armed / not-armed state of the large-mean recompute that its row claims"""
    import convffn_fwd_cases as C
    from helpers import convffn_fwd_class
    for gid, (per_col, rows, HW, Fc) in C.NA_GEOMS.items():
        kernel, grid, n4, trips, armed = C.NA_CLASSES[gid]
        for raw in ((False,) if per_col else (False, True)):
            cls = convffn_fwd_class("norm_act", rows=rows, F=Fc, HW=HW, per_col=per_col, raw=raw)
            assert (cls["kernel"], cls["grid"], cls["float4"], cls["trips"], cls["armed"]) == (kernel, grid, n4, trips, armed and raw), (gid, cls)
    assert 615 % 256 != 0 and 2099200 - 8192 * 256 == 2048                       # a partial last workgroup; what the second trip covers
    assert 12 * 20 // 4 == 60 and 256 % 60 != 0                                  # ln_small: workgroups straddle frames
    assert 15 * 64 * 256 < 1 << 18 == 16 * 64 * 256                              # one frame short of / exactly at the switch
    assert 15000 - 58 * 256 == 152 and 18 > 4 * 4                                # ln_pos_ragged: live threads of the last x-workgroup; a fifth trip
    assert convffn_fwd_class("norm_act", rows=24, F=20, HW=4, per_col=True, raw=True)["kernel"] == "reject"
    assert {v for g in C.NA_GEOMS for g2, v in C.na_cases() if g2 == g} == {"plain", "full", "raw", "p16", "relu"}
    assert ("bn_small", "p16") not in C.na_cases() and ("ln_small", "p16") not in C.na_cases() and ("bn_stride", "raw") not in C.na_cases()
    for place, (kind, frames, H, W, Fc) in C.GUARD_PLACES.items():
        if kind == "na":
            cls = convffn_fwd_class("norm_act", rows=frames * H * W, F=Fc, HW=H * W, per_col=False, raw=True)
            assert cls["armed"] and cls["kernel"] == {"ln_armed": "row", "ln_pos_min": "pos"}[place]
        else:
            assert convffn_fwd_class("dwconv_norm", frames=frames, H=H, W=W, F=Fc)["kernel"] == place[4:]
    for geom, kernel in C.DW_STATS_GEOMS.items():
        assert convffn_fwd_class("dwconv", frames=geom[0], H=geom[1], W=geom[2], F=geom[3], stats=True)["kernel"] == kernel, geom
    for geom in C.DW_STATS_REJECTS:
        assert convffn_fwd_class("dwconv", frames=geom[0], H=geom[1], W=geom[2], F=geom[3], stats=True)["kernel"] == "reject", geom
    for geom, kernel in C.DWN_GEOMS.items():
        assert convffn_fwd_class("dwconv_norm", frames=geom[0], H=geom[1], W=geom[2], F=geom[3])["kernel"] == kernel, geom
    for geom in C.DWN_REJECTS.values():
        assert convffn_fwd_class("dwconv_norm", frames=geom[0], H=geom[1], W=geom[2], F=geom[3])["kernel"] == "reject", geom
    assert convffn_fwd_class("dwconv_norm", frames=2, H=16, W=16, F=64)["lds_bytes"] == 64 * 1024
    for frames, H, W, Fc in C.CHAIN_GEOMS:
        assert convffn_fwd_class("dwconv", frames=frames, H=H, W=W, F=Fc, stats=True)["kernel"] == "fwd3"


def test_onepass_variance_guard_threshold():
    """fp32 emulation of E[x^2] - mean^2 from ideal sums on a 64 x 1024 frame x = r + N(0, 1), 12 seeds: below the guard (var < VAR_GUARD E[x^2],
    |mean| > 9.95 std) the cancellation costs about eps32 (mean / std)^2 and stays at or under half the fp32 vector bar; with the recompute
    it does so up to ratio 100.  Under the former guard of 1e-3 (31.6 std) ratio 25 took the one-pass branch and missed the bar itself"""
    from helpers import VAR_GUARD, onepass_norm_emulation
    TOLV = 2e-5

    def worst(r, guard):
        vals = [onepass_norm_emulation(fill.rand_normal((64, 1024), 9100 + s) + float(r), guard) for s in range(12)]
        assert len({redo for _, redo in vals}) == 1, r
        return max(v for v, _ in vals), vals[0][1]
    assert VAR_GUARD == 1e-2 and (1.0 / VAR_GUARD - 1.0) ** 0.5 < 10.0
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vptr_amd", "csrc")
    tests_in = {f: len(re.findall(r"var < ([0-9.e-]+)f \* e2", open(os.path.join(csrc, f)).read())) for f in ("norm_act.hip", "dwconv.hip")}
    lits = {m for f in tests_in for m in re.findall(r"var < ([0-9.e-]+)f \* e2", open(os.path.join(csrc, f)).read())}
    assert tests_in == {"norm_act.hip": 2, "dwconv.hip": 2} and lits == {"1e-2"}, (tests_in, lits)      # the four copies hold the same guard
    for r in (1.0, 5.0, 9.5, 9.8):
        v, redo = worst(r, VAR_GUARD)
        assert not redo and v <= TOLV / 2, (r, v)
    for r in (10.2, 12.0, 25.0, 31.0, 100.0):
        v, redo = worst(r, VAR_GUARD)
        assert redo and v <= TOLV / 2, (r, v)
    v, redo = worst(25.0, 1e-3)
    assert not redo and v > TOLV, v


@pytest.mark.parametrize("part", ["norm_act", "guard", "dwconv_stats", "dwconv_norm", "chain"])
def test_convffn_fwd_cases_against_emulation(part, capsys):
    """the direct-call cases of tests/test_09c_convffn_fwd_gpu.py against a CPU emulation of the three entry points written from the header:
    argument order, layouts, guards, statistics rows, references and bars of the CASES, not the kernels (the three largest norm_act geometries
    are left to the GPU run)"""
    import convffn_fwd_cases as C
    be = C.EmuBackend()
    if part == "norm_act":
        for gid, variant in C.na_cases():
            if gid in ("bn_small", "ln_small", "ln_armed", "ln_pos_ragged"):
                C.run_norm_act(be, gid, variant)
        C.run_norm_act_rejects(be)
    elif part == "guard":
        for place in ("ln_armed", "dwn_lds", "dwn_reg"):
            for r in (9, 25):
                C.run_guard(be, place, r)
    elif part == "dwconv_stats":
        for geom in C.DW_STATS_GEOMS:
            C.run_dwconv_stats(be, geom)
        C.run_dwconv_stats_rejects(be)
    elif part == "dwconv_norm":
        for geom, variant in C.dwn_cases():
            C.run_dwn(be, geom, variant)
        for geom, variant in C.dwn_cases(True):
            C.run_dwn_half_elements(be, geom, variant)
        C.run_dwn_rejects(be)
    else:
        C.run_chain(be, C.CHAIN_GEOMS[0])


def test_gelu_polynomial_leaves_room_for_the_fp16_rounding():
    """vptr_phi's erfc polynomial (coefficients read from csrc/common.h) replayed in fp32 on x in [-10, 0]: the error of x * Phi(x) stays inside
    2^-22 |ref| + 2^-24, what the round-to-nearest bound of the fp16 side copy (2^-11 |ref| + 2^-24) leaves an fp32 value that sits next to a
    power of two; Abramowitz-Stegun's five coefficients (1.5e-7 absolute) exceed it 3.5 times near x = -3.7"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vptr_amd", "csrc", "common.h")).read()
    body = src[src.index("const float poly = t * ("):src.index("const float h = 0.5f * poly * e;")]
    coef = [float(c) for c in re.findall(r"(-?[0-9]+\.[0-9]+)f", body)]
    p = float(re.search(r"1\.0f \+ ([0-9.]+)f \* ax", src).group(1))
    assert len(coef) == 9 and p == 0.3275911
    f32 = np.float32
    x = -np.linspace(0.0, 10.0, 400001).astype(f32)
    x64 = x.astype(np.float64)
    ref = x64 * 0.5 * torch.special.erfc(torch.from_numpy(-x64) / 2 ** 0.5).numpy()

    def worst(cs):
        ax = np.abs(x) * f32(0.70710678118654752)
        t = (f32(1) / (f32(1) + f32(p) * ax)).astype(f32)
        e = np.exp(-(ax * ax).astype(f32)).astype(f32)
        poly = np.full_like(t, f32(cs[-1]))
        for c in cs[-2::-1]:
            poly = (poly * t + f32(c)).astype(f32)
        got = (x * (f32(0.5) * (poly * t).astype(f32) * e).astype(f32)).astype(np.float64)
        return float((np.abs(got - ref) / (2.0 ** -22 * np.abs(ref) + 2.0 ** -24)).max())
    assert worst(coef) <= 1.0, worst(coef)
    assert worst([0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429]) > 3.0


# ---- the tail of the train step through the C ABI (tests/test_09d_step_tail_gpu.py): reference builders, the sign condition of the GDL inputs,
# launch classes, the fp32 emulation the AdamW bars come from, the RNG emulation's own properties, emulated cases ---------------------------------
def test_step_tail_refs_are_the_oracle_and_torch_optim():
    """helpers.nce_ref on token-major rows == F.normalize + the oracle's bipatch_nce on a real (N, T, C, h, w) patch grid; helpers.adamw_ref with
    the double hyper-parameters == clip_grad_norm_ on the scaled gradients + one torch.optim.AdamW step on fp64 parameters from the same
    state, at 1e-12, for the clip absent / active / inactive, grad_scale 0.25 and both weight decays"""
    import torch.nn.functional as Fn
    import step_tail_cases as C
    from helpers import adamw_ref, nce_ref
    frames, h, w, Cc, tau = 3, 2, 5, 12, 0.07
    g, p = fill.rand_normal((frames * h * w, Cc), 51), fill.rand_normal((frames * h * w, Cc), 52)
    gd, pd = g.double().requires_grad_(True), p.double().requires_grad_(True)

    def as5(t):
        return t.reshape(1, frames, h, w, Cc).permute(0, 1, 4, 2, 3)
    loss = O.bipatch_nce(Fn.normalize(as5(gd), p=2.0, dim=2), Fn.normalize(as5(pd), p=2.0, dim=2), tau)
    (1.3 * loss).backward()
    ref = nce_ref(g, p, frames, h * w, tau, 1.3)
    loss = loss.detach()
    assert abs(ref["loss"] - float(loss)) < 1e-12 and rel(ref["dg"], gd.grad) < 1e-12 and rel(ref["dp"], pd.grad) < 1e-12
    S = ref["S"]
    part = (ref["rlse"] + ref["clse"] - 2.0 * torch.diagonal(S, dim1=1, dim2=2)).sum()
    assert abs(float(part) * 0.5 / (frames * h * w) - float(loss)) < 1e-12           # the sections are the ones the loss is made of

    for k in (1, 4):
        for case, (max_norm, gs) in C.ADAMW_CLIP.items():
            for wd in C.ADAMW_WD:
                p0, g0, m0, v0 = C.adamw_inputs(C.ADAMW_N, k, 0.9, 0.999)
                pr = p0.double().clone().requires_grad_(True)
                opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
                opt.state[pr] = {"step": torch.tensor(float(k - 1), dtype=torch.float64), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
                pr.grad = g0.double() * gs
                if max_norm is not None:
                    torch.nn.utils.clip_grad_norm_([pr], max_norm)
                opt.step()
                sumsq = None if max_norm is None else float((g0.double() ** 2).sum())
                got = adamw_ref(p0, g0, m0, v0, k, 1e-3, 0.9, 0.999, 1e-8, wd, sumsq, 1.0 if max_norm is None else max_norm, gs, abi_hyper=False)
                st = opt.state[pr]
                assert rel(got[0] - p0.double(), pr.detach() - p0.double()) < 1e-12, (k, case, wd)
                assert rel(got[1], st["exp_avg"]) < 1e-12 and rel(got[2], st["exp_avg_sq"]) < 1e-12, (k, case, wd)


def test_step_tail_gdl_inputs_have_no_fragile_sign():
    """the GDL gradient is a sum of signs: for the seeded inputs of every geometry an fp32 and an fp64 evaluation of every sign argument agree, so
    no element has to be excluded on the device; the forced ties are there (exact zeros among the arguments)"""
    import step_tail_cases as C
    from helpers import gdl_sign_disagreements
    for geom in C.MSE_GEOMS:
        pred, gt = C.mse_inputs(geom)
        assert gdl_sign_disagreements(pred, gt) == 0, geom
        k = C.mse_tie_rows(geom[1])
        assert torch.equal(pred[:, :k], gt[:, :k]) and bool((pred[:, -1, 0] == pred[:, -1, 1]).all())
        pdw, gdw = pred[:, :, :-1] - pred[:, :, 1:], gt[:, :, :-1] - gt[:, :, 1:]
        assert bool(((gdw.abs() - pdw.abs()) == 0).any()) and bool(((pdw == 0) & (gdw != 0)).any())      # sign(0) in both factors


def test_step_tail_cases_land_in_their_launch_classes():
    """the launchers' arithmetic restated (helpers.step_tail_class): block counts, NV class, trips of each loop for every geometry of
    tests/step_tail_cases.py"""
    import step_tail_cases as C
    from helpers import step_tail_class as cls
    m = {g: cls("mse_gdl", planes=g[0], H=g[1], W=g[2]) for g in C.MSE_GEOMS}
    assert (m[(300, 5, 3)]["partials"], m[(300, 5, 3)]["final_trips"]) == (300, 2)
    assert (m[(2, 17, 9)]["bands"], m[(2, 17, 9)]["last_band_rows"]) == (2, 1)
    assert (m[(1, 2, 2)]["partials"], m[(1, 2, 2)]["bwd_blocks"], m[(1, 2, 2)]["scratch"]) == (1, 1, 3)
    assert (m[(2, 33, 300)]["bands"], m[(2, 33, 300)]["last_band_rows"], m[(2, 33, 300)]["band_trips"]) == (3, 1, 19)
    assert (m[(7, 16, 16)]["bands"], m[(7, 16, 16)]["last_band_rows"], m[(7, 16, 16)]["band_trips"]) == (1, 16, 1)
    assert (m[(40, 64, 64)]["partials"], m[(40, 64, 64)]["final_trips"]) == (160, 1)
    assert all(v["final_trips"] == 1 for g, v in m.items() if g != (300, 5, 3))
    for planes, H, W in C.MSE_REJECTS:
        assert cls("mse_gdl", planes=planes, H=H, W=W) == {"kernel": "reject"}
    for Cc in C.NCE_CHANNELS:
        c = cls("nce", frames=2, L=35, C=Cc)
        assert c["nv"] == C.NCE_NV[Cc] and c["lds_bytes"] <= 64 * 1024 and c["channel_guard"] == (Cc % 16 != 0), Cc
        assert (c["nb"], c["dead_rows"], c["chunks"], c["partial_chunk"]) == (1, 29, 3, True)
    assert {C.NCE_NV[c] for c in C.NCE_CHANNELS} == {4, 16, 34, 40} and sum(c % 16 != 0 for c in C.NCE_CHANNELS) >= 4
    assert cls("nce", frames=2, L=35, C=644)["nv"] == "reject" and cls("nce", frames=2, L=35, C=6)["nv"] == "reject"
    want = {(1, 1): (1, 63, 1, True, 1), (3, 64): (1, 0, 4, False, 1), (2, 80): (2, 48, 5, False, 1), (1, 130): (3, 62, 9, True, 1),
            (2, 256): (4, 0, 16, False, 1), (300, 4): (1, 60, 1, True, 2)}
    for (frames, L), w in want.items():
        c = cls("nce", frames=frames, L=L, C=548)
        assert (c["nb"], c["dead_rows"], c["chunks"], c["partial_chunk"], c["final_trips"]) == w, (frames, L)
        assert c["scratch"] == frames * L * (4 + L) + frames and c["bwd_grid"] == frames * c["nb"] * 2
    assert set(want) == set(C.NCE_GEOMS) and len(C.nce_cases()) == 2 * (len(C.NCE_CHANNELS) + 2 * len(C.NCE_GEOMS))
    big = cls("sumsq", n=C.SUMSQ_BIG)
    assert big == {"blocks": 256, "unrolled": 2, "singles": 2, "partial_threads": 1000, "tail": 2} and C.SUMSQ_BIG * 4 < 50e6
    assert cls("sumsq", n=10007) == {"blocks": 10, "unrolled": 0, "singles": 0, "partial_threads": 2501, "tail": 3}       # test_00's size
    assert cls("sumsq", n=3)["tail"] == 3 and cls("sumsq", n=1024)["tail"] == 0 and cls("sumsq", n=1023)["tail"] == 3
    assert cls("sumsq", n=C.SUMSQ_BIG, aligned=False) == {"blocks": 256, "scalar_trips": 41}
    a = cls("adamw", n=C.ADAMW_BIG)
    assert a == {"blocks": 4096, "vec_trips": 2, "scalar_trips": 1, "tail": 3}
    assert cls("adamw", n=10007) == {"blocks": 11, "vec_trips": 1, "scalar_trips": 1, "tail": 3}                             # test_00's size
    assert cls("adamw", n=C.ADAMW_BIG, aligned=False) == {"blocks": 4096, "vec_trips": 0, "scalar_trips": 5, "tail": C.ADAMW_BIG}
    assert [cls("adamw", n=n)["vec_trips"] for n in (1, 3, 4, 1027)] == [0, 0, 1, 1] and cls("adamw", n=1027)["blocks"] == 2
    assert cls("adamw", n=C.ADAMW_N) == {"blocks": 5, "vec_trips": 1, "scalar_trips": 1, "tail": 3}


def test_adamw_bars_come_from_a_cancellation_free_fp32_evaluation():
    """helpers.adamw_f32_emulation (the kernel's formula in fp32 with 1 - b^k = -expm1(k log1p(b - 1))) on the inputs of the update-precision
    cases: its rel-L2 distance to fp64 is about 1e-7 on the update, m and v at every step count, so the bars (5 x) sit at or below 1e-6.
    The same evaluation with 1 - powf(b, k) is 3 to 60 times further from fp64 on the update at steps 2, 3 and 5 of betas (0.9, 0.999) -- the
    subtraction cancels -- and exactly as close at step 1, where 1 - 0.999f is exact"""
    import step_tail_cases as C
    from helpers import adamw_f32_emulation, adamw_ref
    F = np.float32
    for betas in C.ADAMW_BETAS:
        hyper = dict(C.HYPER, b1=betas[0], b2=betas[1])
        for k in C.ADAMW_STEPS:
            p, g, m, v = C.adamw_inputs(C.ADAMW_N, k, betas[0], betas[1])
            state = (torch.zeros_like(p), g, m, v)
            bars, dist, want = C.adamw_bars(state, k, hyper, None, None, 1.0)
            print("adamw emulation step %d betas %g/%g: update %.3e m %.3e v %.3e" % ((k,) + betas + tuple(dist)))
            # (b1 = 0.5 at step 1: m = 0.5 g is exact in any binary format, its distance and its bar are 0)
            assert all(d < 2e-7 for d in dist) and dist[0] > 0.0 and all(b == 5.0 * d for b, d in zip(bars, dist)), (k, betas, dist)
            # the cancelling form: the update scales with sqrt(bc2) / bc1
            bc = [F(1) - np.power(F(b), F(k), dtype=F) for b in betas]
            exact = [1.0 - float(F(b)) ** k for b in betas]
            scale = (float(bc[1]) / exact[1]) ** 0.5 / (float(bc[0]) / exact[0])
            naive = rel(adamw_f32_emulation(*state, k, **hyper)[0].double() * scale, want[0])
            print("    with 1 - powf(b, k): update %.3e" % naive)
            if k == 1:
                assert scale == 1.0
            if betas == (0.9, 0.999) and k in (2, 3, 5):
                assert naive > bars[0], (k, naive, bars[0])


def test_hash_emulation_properties():
    """helpers.hash3_emu / drop_scale_emu / droppath_emu (the integer emulation of csrc/common.h the device is compared with bit for bit): the
    keep rate of 10^6 elements within 3 sigma of 1 - p; flipping one bit of the seed's low word, of its high word, of the site or of the
    index flips 0.5 +- 0.02 of the 32 output bits on average (the two-multiply finaliser's avalanche bias is under 1 %, the mean over 20 000
    x 32 bits has a sigma of 6e-4); the index's high word takes part; constants as in the source"""
    from helpers import drop_scale_emu, droppath_emu, hash3_emu, mix32_emu
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vptr_amd", "csrc", "common.h")).read()
    for const in ("0x7FEB352Du", "0x846CA68Bu", "0x9E3779B9u", "0xC2B2AE35u", "x >> 16; x *=", "x ^= x >> 15"):
        assert const in src, const
    assert mix32_emu(0) == 0 and mix32_emu(1) == mix32_emu(torch.tensor([1]))[0] and 0 < mix32_emu(1) < 1 << 32
    seed, n = 0x9A3C5E7F12345678, 1000000
    idx = torch.arange(n)
    for p in (0.1, 0.5, 0.999):
        s = drop_scale_emu(seed, 3, idx, p)
        kept = float((s != 0).double().mean())
        assert abs(kept - (1.0 - p)) < 3.0 * (p * (1.0 - p) / n) ** 0.5, (p, kept)
        assert set(torch.unique(s).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    dp = droppath_emu(torch.tensor([0.9, 0.5, 1.0]), 100000, seed, 7)
    for r, kp in enumerate((0.9, 0.5)):
        assert abs(float((dp[r] != 0).double().mean()) - kp) < 3.0 * (kp * (1.0 - kp) / 100000) ** 0.5
    assert bool((dp[2] == 1.0).all())

    def flipped(a, b):
        x = a ^ b
        return float(sum(((x >> i) & 1).double().mean() for i in range(32)) / 32.0)
    idx = torch.arange(20000) * 7919 + 11
    base = hash3_emu(seed, 5, idx)
    for bit in range(32):
        for name, other in (("seed low", hash3_emu(seed ^ (1 << bit), 5, idx)), ("seed high", hash3_emu(seed ^ (1 << (32 + bit)), 5, idx)),
                            ("site", hash3_emu(seed, 5 ^ (1 << bit), idx)), ("index", hash3_emu(seed, 5, idx ^ (1 << bit)))):
            f = flipped(base, other)
            assert 0.48 < f < 0.52, (name, bit, f)
    assert not torch.equal(hash3_emu(seed, 5, idx + (1 << 32)), base) and 0.48 < flipped(hash3_emu(seed, 5, idx + (1 << 32)), base) < 0.52
    assert hash3_emu(seed, 0xFFFFFFFF, idx).max() < 1 << 32 and torch.equal(hash3_emu(seed, -1, idx), hash3_emu(seed, 0xFFFFFFFF, idx))


def test_nce_bars_are_reachable_in_fp32():
    """helpers.nce_f32_emulation (fp32 storage and arithmetic in the kernels' order, libm's exp / log) stays inside test_00's bars -- loss 2e-6,
    gradients 1e-5 -- for every case of tests/step_tail_cases.py, so no bar has to move.  The closest are the saturated softmaxes at tau 0.07,
    where lse - S cancels: 300 x 4 x 548 (gradients at 0.86 - 0.89 of the bar) and 2 x 35 x 544 (loss at 0.68)"""
    import step_tail_cases as C
    worst = {"loss": (0.0, None), "dg": (0.0, None), "dp": (0.0, None)}
    for case in C.nce_cases() + [(2, 35, 6, tau) for tau in C.NCE_TAUS]:
        d = C.nce_emulation_distances(*case, 1.0)
        for k, v in d.items():
            assert v < (C.TOL_NCE if k == "loss" else C.TOL_NCE_GRAD), (case, k, v)
            worst[k] = max(worst[k], (v, case))
    print("nce fp32 emulation, worst distances:", worst)
    assert worst["dg"][1] == (300, 4, 548, 0.07) and worst["dp"][1] == (300, 4, 548, 0.07) and worst["loss"][1] == (2, 35, 544, 0.07)


@pytest.mark.parametrize("part", ["mse_gdl", "nce_channels", "nce_geoms", "sumsq", "adamw", "rng"])
def test_step_tail_cases_against_emulation(part, capsys):
    """the cases of tests/test_09d_step_tail_gpu.py against a CPU emulation of the entry points written from the header: argument order,
    layouts, guards, scratch sizes, references and bars of the CASES, not the kernels"""
    import step_tail_cases as C
    be = C.EmuBackend()
    if part == "mse_gdl":
        for geom in C.MSE_GEOMS:
            for variant in C.MSE_VARIANTS:
                C.run_mse_gdl(be, geom, variant)
        C.run_mse_gdl_rejects(be)
    elif part == "nce_channels":
        for frames, L, Cc, tau in C.nce_cases()[:2 * len(C.NCE_CHANNELS)]:
            C.run_nce(be, frames, L, Cc, tau)
        C.run_nce_c6(be)
        C.run_nce_bwd_rejects(be)
    elif part == "nce_geoms":
        for frames, L, Cc, tau in C.nce_cases()[2 * len(C.NCE_CHANNELS):]:
            C.run_nce(be, frames, L, Cc, tau)
    elif part == "sumsq":
        for n in C.SUMSQ_SIZES:
            for aligned in (True, False):
                C.run_sumsq(be, n, aligned)
        for nws in C.SUMSQ_WS:
            C.run_sumsq_ws(be, nws)
        C.run_sumsq_rejects(be)
    elif part == "adamw":
        for case in C.ADAMW_LAUNCH:
            C.run_adamw_launch(be, case)
        C.run_adamw_paths_equal(be)
        for case in C.ADAMW_CLIP:
            for wd in C.ADAMW_WD:
                C.run_adamw_clip(be, case, wd)
        C.run_adamw_zero_grad(be)
        for betas in C.ADAMW_BETAS:
            for k in C.ADAMW_STEPS:
                C.run_adamw_precision(be, k, betas)
    else:
        for n in C.DROP_SIZES:
            C.run_dropout(be, n)
        for maxcount in C.DROPPATH_COUNTS:
            C.run_droppath(be, maxcount)


# ---- the nt P16 GEMM through the C ABI (tests/test_01b_gemm_p16_abi_gpu.py): the launch-class mirror, the cases against a CPU emulation of the call,
# the kink cap and the mutations of the emulation
_G = dict(a_mode=5, b_mode=3, precision=3, M=300, N=528, K=144, lda=144, ldb=144, ldd=528, A=0x10000, B=0x20000, D=0x30000)     # 3 x 3 tiles
_GX = dict(A_x1=0x11000, B_x1=0x21000, D_x1=0x31000, A_x2=0x12000, B_x2=0x22000, D_x2=0x32000)
# written by hand from vptr_gemm_p16_launch and the EPI 0 branch of vptr_gemm_p16_kernel: (changes to _G, compute units, class)
GEMM_P16_TABLE = [
    (dict(), 256, (1, 4, "batched")), (dict(), 9, (1, 4, "batched")), (dict(), 8, (1, 2, "batched")), (dict(), 0, (1, 2, "batched")),
    (dict(bias=0x40000, residual=0x50000, ldr=528, alpha=0.5), 256, (1, 4, "batched")),
    (dict(bias=0x40004), 256, (0, 4, "serial")), (dict(bias=0x40004), 8, (0, 2, "serial")),
    (dict(residual=0x50008, ldr=528), 256, (0, 4, "serial")), (dict(residual=0x50000, ldr=530), 8, (0, 2, "serial")),
    (dict(N=50, ldd=52), 256, (0, 4, "serial")), (dict(ldd=530), 256, (0, 4, "serial")), (dict(D=0x30010), 256, (1, 4, "batched")),
    (dict(rowscale=0x60004, rs_div=64, rs_mod=5), 256, (3, 4, "batched")), (dict(dropout_p=0.1, seed_dev=0x70000), 8, (3, 2, "batched")),
    (dict(rowscale=0x60000, rs_div=1, rs_mod=1, dropout_p=0.1, seed_dev=0x70000, bias=0x40000, residual=0x50000, ldr=528, d_p16=1), 256, (3, 4, "batched")),
    (dict(rowscale=0x60000, rs_div=0, rs_mod=1), 256, ("refuse", 10)), (dict(dropout_p=0.1), 256, ("refuse", 11)),
    (dict(dropout_p=1.0, seed_dev=0x70000), 256, ("refuse", 11)),
    (dict(act=1), 256, (4, 4, "batched")), (dict(act=3, Dpre=0x80000, dropout_p=0.1, seed_dev=0x70000, bias=0x40000, d_p16=1), 8, (4, 2, "batched")),
    (dict(act=1, Dpre=0x80004), 256, (0, 4, "serial")), (dict(act=2, residual=0x50000, ldr=528), 256, (0, 4, "batched")),
    (dict(act=2, residual=0x50000, ldr=528), 8, (0, 2, "rows_halves")), (dict(act=1, rowscale=0x60000, rs_div=1, rs_mod=1), 8, (0, 2, "rows_halves")),
    (dict(act=1, batch=2, **_GX), 256, (0, 4, "batched")), (dict(act=1, ksegs=3, **_GX), 256, (4, 4, "batched")),
    (dict(colscale=0x90000), 256, (0, 4, "batched")), (dict(colscale=0x90004), 8, (0, 2, "serial")), (dict(act_after=1), 8, (0, 2, "rows_halves")),
    (dict(atomic=1), 256, (0, 4, "serial")), (dict(atomic=1), 8, (0, 2, "serial")), (dict(atomic=1, d_p16=1), 256, ("refuse", 12)),
    (dict(act=1, act_grad_src=0xA0000), 256, (2, 4, "batched")), (dict(act=3, act_grad_src=0xA0000, dropout_p=0.1, seed_dev=0x70000, d_p16=1), 8, (2, 2, "batched")),
    (dict(act_grad_src=0xA0000), 256, ("refuse", 14)), (dict(act=1, act_grad_src=0xA0004), 256, ("refuse", 14)),
    (dict(act=1, act_grad_src=0xA0000, bias=0x40000), 256, ("refuse", 14)), (dict(act=1, act_grad_src=0xA0000, ksegs=2, **_GX), 256, ("refuse", 14)),
    (dict(batch=3, **_GX), 27, (1, 4, "batched")), (dict(batch=3, **_GX), 26, (1, 2, "batched")), (dict(batch=3, bias_x2=0x41004, **_GX), 27, (0, 4, "serial")),
    (dict(batch=2, batch_accum=2, **_GX), 256, (1, 4, "batched")), (dict(batch=2, batch_accum=4, **_GX), 256, ("refuse", 15)),
    (dict(batch=2, batch_accum=1, d_p16=1, **_GX), 256, ("refuse", 15)), (dict(batch_accum=1), 256, ("refuse", 15)),
    (dict(batch=2, batch_accum=1, act=1, **_GX), 256, ("refuse", 15)),
    (dict(batch=2, A_x1=0x11000, B_x1=0x21000), 256, ("refuse", 9)), (dict(batch=2, residual=0x50000, ldr=528, **_GX), 256, ("refuse", 9)),
    (dict(batch=3, A_x1=0x11000, B_x1=0x21000, D_x1=0x31000), 256, ("refuse", 7)), (dict(batch=2), 256, ("refuse", 6)), (dict(ksegs=2, A_x1=0x11000), 256, ("refuse", 6)),
    (dict(batch=4, **_GX), 256, ("refuse", 5)), (dict(ksegs=4, **_GX), 256, ("refuse", 5)), (dict(batch=2, ksegs=2, **_GX), 256, ("refuse", 5)),
    (dict(batch=40, batch_stride_a=4800, batch_stride_b=0, batch_stride_d=16 * 528 * 20), 256, (1, 2, "batched")),
    (dict(batch=28, batch_stride_a=4800, batch_stride_b=16, batch_stride_d=16 * 528 * 20, d_p16=1, bias=0x40000), 252, (1, 4, "batched")),
    (dict(batch=2, batch_stride_a=4800, batch_stride_b=0, batch_stride_d=528 * 300 + 8), 256, ("refuse", 4)),
    (dict(batch=2, batch_stride_a=4800, batch_stride_b=0, batch_stride_d=16 * 528 * 20, act=1), 256, ("refuse", 4)),
    (dict(batch=2, batch_stride_a=-16, batch_stride_b=0, batch_stride_d=16 * 528 * 20), 256, ("refuse", 4)),
    (dict(batch=5000, batch_stride_a=0, batch_stride_b=0, batch_stride_d=16 * 528 * 20), 256, ("refuse", 4)),
    (dict(frame_stats=0xB0000, frame_rows=64, M=320), 256, (1, 4, "batched")), (dict(frame_stats=0xB0000, frame_rows=192, M=320, residual=0x50000, ldr=528), 8, (1, 2, "batched")),
    (dict(frame_stats=0xB0000, frame_rows=64), 256, ("refuse", 13)), (dict(frame_stats=0xB0000, frame_rows=96, M=320), 256, ("refuse", 13)),
    (dict(frame_stats=0xB0000, frame_rows=64, M=320, dropout_p=0.1, seed_dev=0x70000), 256, ("refuse", 13)),
    (dict(frame_stats=0xB0000, frame_rows=64, M=320, batch=2, **_GX), 256, ("refuse", 13)),
    (dict(d_p16=1), 256, (1, 4, "batched")), (dict(d_p16=1, N=100, ldd=112), 256, ("refuse", 12)), (dict(d_p16=1, ldd=536), 256, ("refuse", 12)),
    (dict(d_p16=1, D=0x30010), 256, ("refuse", 12)), (dict(d_p16=1, bias=0x40004), 256, ("refuse", 12)),
    (dict(K=24), 256, ("refuse", 2)), (dict(lda=152), 256, ("refuse", 2)), (dict(precision=1), 256, ("refuse", 3)), (dict(split_k=2), 256, ("refuse", 3)),
    (dict(a_rowsum=0xC0000), 256, ("refuse", 3)), (dict(a_mode=0), 256, ("refuse", 1)), (dict(b_mode=0), 256, ("refuse", 1)),
    (dict(A=0x10010), 256, ("refuse", 8)), (dict(ksegs=2, A_x1=0x11020, B_x1=0x21000), 256, ("refuse", 8)),
]


def test_gemm_p16_class_table():
    """helpers.gemm_p16_class against a table written by hand from the launcher's conditions and the run-time choice of the EPI 0 kernels"""
    from helpers import gemm_p16_class
    bad = []
    for change, cus, want in GEMM_P16_TABLE:
        got = gemm_p16_class(dict(_G, **change), cus)
        if got != want:
            bad.append((change, cus, got, want))
    assert not bad, bad
    assert {w for _, _, w in GEMM_P16_TABLE if w[0] != "refuse"} == set(__import__("gemm_p16_cases").CLASSES)
    assert {w[1] for _, _, w in GEMM_P16_TABLE if w[0] == "refuse"} == set(range(1, 16))


@pytest.mark.parametrize("cus", [16, 256, 304])
def test_gemm_p16_cases_cover_every_launch_class(cus):
    """each of the twelve classes is run by at least two cases whatever the compute-unit count (the NST = 2 geometries grow with it); every case
    asserts its class while it is built"""
    import gemm_p16_cases as C
    census = C.class_census(cus)
    assert len(census) == 12 and all(len(v) >= 2 for v in census.values()), {k: len(v) for k, v in census.items()}
    assert sum(len(v) for v in census.values()) == len(C.CASES)


@pytest.mark.parametrize("part", range(4))
def test_gemm_p16_cases_against_emulation(part, capsys):
    """every case of tests/test_01b_gemm_p16_abi_gpu.py against the fp32 CPU emulation of the call (16 compute units): descriptors, pitches,
    guards, references and bars of the CASES; the emulation's fp32 arithmetic stays inside every bar and leaves at most 1 % of a case's elements
    to the kink rule (asserted per case by the runner)"""
    import gemm_p16_cases as C
    be = C.EmuBackend()
    for cid in C.CASES[part::4]:
        _, figures = C.run_case(be, cid)
        assert all(w <= 1.0 and r < C.TOL3 for w, r in figures)
    if part == 0:
        for k in C.REJECTS:
            C.run_reject(be, k)


# mutation -> cases that have to notice it (a few each; at least one must fail)
GEMM_P16_MUTATION_CASES = {
    "tail_not_zeroed": ["e1_bias_alpha-g10", "e1_bias_alpha-g129", "e1_bias_alpha-n1"], "seg3_reads_seg2": ["e1_kseg3-g129", "e3_both_kseg3-n72"],
    "col_plus4": ["e0_n50-g129n50", "e0_n50-n1n50"], "drop_index_ldd": ["e3_drop-g129", "e4_gelu-g129", "e2_drop-g129"],
    "rs_div_ignored": ["e3_rs-g129", "e0_act_rs_res-g129"], "accum_ignored": ["e1_accum6-g129", "e1_accum7-g129"],
    "dpre_after_act": ["e4_gelu-g129", "e4_lrelu-g129"], "grad_src_pitch_n": ["e2_gelu-g129", "e2_relu-g129"], "p16_without_lo": ["e1_p16-g129", "e1_strided_p16-sb4"],
}


@pytest.mark.parametrize("mut", sorted(GEMM_P16_MUTATION_CASES))
def test_gemm_p16_cases_notice_mutations(mut, capsys):
    """each named mutation of the emulation makes every case listed for it fail (and the unmutated emulation passes them, above)"""
    import gemm_p16_cases as C
    assert sorted(GEMM_P16_MUTATION_CASES) == sorted(C.MUTATIONS)
    be = C.EmuBackend(mut=mut)
    for cid in GEMM_P16_MUTATION_CASES[mut]:
        with pytest.raises(AssertionError):
            C.run_case(be, cid)


# ---- the fp32-staged GEMM through the C ABI (tests/test_01c_gemm_f32_abi_gpu.py): the launch-class mirror, the census, the cases against a CPU
# emulation of the call and the mutations of the emulation
_F = dict(a_mode=0, b_mode=0, precision=3, M=300, N=528, K=144, lda=144, ldb=144, ldd=528, A=0x10000, B=0x20000, D=0x30000)      # 3 x 3 tiles of 128 x 176
_FX = dict(A_x1=0x11000, B_x1=0x21000, D_x1=0x31000, A_x2=0x12000, B_x2=0x22000, D_x2=0x32000)
_FC = dict(a_mode=2, K=36, conv_IH=8, conv_IW=8, conv_Cin=4, conv_OH=8, conv_OW=8, conv_KH=3, conv_KW=3, conv_stride=1, conv_pad=1)
# written by hand from vptr_gemm, launch_one, nfn_for and the epilogue choice of the two kernels: (changes to _F, class)
GEMM_F32_TABLE = [
    (dict(), ("P", "rows", 11, "kc", "kc", 3)), (dict(precision=1), ("P", "rows", 11, "kc", "kc", 1)), (dict(M=128 * 128), ("S", "rows_halves", 11, "kc", "kc", 3)),
    (dict(M=128 * 127 + 1), ("S", "rows_halves", 11, "kc", "kc", 3)), (dict(M=128 * 127), ("P", "rows", 11, "kc", "kc", 3)),      # 384 / 381 workgroups
    (dict(M=128 * 128, N=527, ldd=528), ("S", "serial", 11, "kc", "kc", 3)),                    # N % 4 != 0
    (dict(N=64, ldd=64), ("P", "rows", 4, "kc", "kc", 3)), (dict(N=50, ldd=52), ("P", "frag", 4, "kc", "kc", 3)), (dict(N=65, ldd=68), ("P", "frag", 8, "kc", "kc", 3)), (dict(N=128, ldd=128), ("P", "rows", 8, "kc", "kc", 3)),
    (dict(N=180, ldd=180), ("P", "rows", 4, "kc", "kc", 3)), (dict(N=200, ldd=200), ("P", "rows", 8, "kc", "kc", 3)), (dict(N=340, ldd=340), ("P", "rows", 11, "kc", "kc", 3)),
    (dict(N=129, ldd=132), ("P", "frag", 11, "kc", "kc", 3)), (dict(N=352, ldd=352), ("P", "rows", 11, "kc", "kc", 3)), (dict(N=384, ldd=384), ("P", "rows", 8, "kc", "kc", 3)),
    (dict(M=128 * 384, N=64, ldd=64), ("S", "serial", 4, "kc", "kc", 3)), (dict(M=128 * 384, N=128, ldd=128, b_mode=1), ("S", "serial", 8, "kc", "ks", 3)),
    (dict(ldd=530), ("P", "frag", 11, "kc", "kc", 3)), (dict(D=0x30004), ("P", "frag", 11, "kc", "kc", 3)), (dict(bias=0x40008), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(residual=0x50000, ldr=530), ("P", "frag", 11, "kc", "kc", 3)), (dict(Dpre=0x80004), ("P", "frag", 11, "kc", "kc", 3)), (dict(colscale=0x90004), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(M=128 * 128, D=0x30004), ("S", "serial", 11, "kc", "kc", 3)), (dict(M=128 * 128, atomic=1), ("S", "serial", 11, "kc", "kc", 3)),
    (dict(atomic=1), ("P", "frag", 11, "kc", "kc", 3)), (dict(split_k=2), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(split_k=5), ("P", "frag", 11, "kc", "kc", 3)),                                        # k_chunk 32: 5 splits, 45 workgroups
    (dict(K=100, lda=100, ldb=100, split_k=7, M=128 * 32), ("S", "serial", 11, "kc", "kc", 3)),  # the launcher makes 4 splits: 32 x 3 x 4 = 384
    (dict(K=100, lda=100, ldb=100, split_k=7, M=128 * 31), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(K=100, lda=100, ldb=100, split_k=3, M=128 * 64), ("S", "serial", 11, "kc", "kc", 3)),  # k_chunk 64: 2 splits, 64 x 3 x 2 = 384
    (dict(K=100, lda=100, ldb=100, split_k=3, M=128 * 63), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(a_mode=1, M=300, lda=300), ("P", "rows", 11, "ks2", "kc", 3)), (dict(a_mode=1, b_mode=1, M=300, lda=300, ldb=528, K=33), ("P", "rows", 11, "ks2", "ks", 3)),
    (dict(a_mode=1, M=128 * 128, lda=128 * 128, a_rowsum=0xC0000), ("P", "rows", 11, "ks2", "kc", 3)),        # 384 workgroups, still pipelined
    (dict(a_mode=1, M=128 * 128, lda=128 * 128), ("S", "rows_halves", 11, "ks2", "kc", 3)),
    (dict(_FC), ("P", "rows", 11, "conv", "kc", 3)), (dict(_FC, d_row_w=8, d_row_off=8), ("P", "frag", 11, "conv", "kc", 3)),
    (dict(_FC, M=128 * 128, d_row_w=8), ("S", "serial", 11, "conv", "kc", 3)), (dict(d_row_w=10), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(batch=3, **_FX), ("P", "rows", 11, "kc", "kc", 3)), (dict(batch=3, bias_x2=0x41004, **_FX), ("P", "frag", 11, "kc", "kc", 3)),
    (dict(batch=3, M=128 * 43, **_FX), ("S", "rows_halves", 11, "kc", "kc", 3)),                # 43 x 3 x 3 = 387
    (dict(batch=2, M=128 * 64, D_x1=0x31004, A_x1=0x11000, B_x1=0x21000), ("S", "serial", 11, "kc", "kc", 3)),
    (dict(ksegs=3, **_FX), ("P", "rows", 11, "kc", "kc", 3)), (dict(ksegs=2, M=128 * 128, D_x1=0x31004, A_x1=0x11000, B_x1=0x21000), ("S", "rows_halves", 11, "kc", "kc", 3)),
    # refusals, in source order
    (dict(K=0), ("refuse", 1)), (dict(M=-1), ("refuse", 1)), (dict(A=0), ("refuse", 2)), (dict(D=0), ("refuse", 2)), (dict(D_planes=0xD0000), ("refuse", 3)),
    (dict(precision=2), ("refuse", 4)), (dict(batch_accum=1), ("refuse", 5)), (dict(batch_stride_d=16), ("refuse", 5)), (dict(d_p16=1), ("refuse", 6)),
    (dict(d_row_off=4), ("refuse", 7)), (dict(d_row_w=8, residual=0x50000), ("refuse", 7)), (dict(d_row_w=8, split_k=2), ("refuse", 7)), (dict(d_row_w=8, atomic=1), ("refuse", 7)),
    (dict(d_row_w=8, batch=2, **_FX), ("refuse", 7)), (dict(act_grad_src=0xA0000), ("refuse", 8)), (dict(frame_stats=0xB0000), ("refuse", 8)), (dict(a_mode=4), ("refuse", 9)),
    (dict(A=0x10004), ("refuse", 10)), (dict(B=0x20008), ("refuse", 10)), (dict(K=142), ("refuse", 11)), (dict(a_mode=1, K=33), ("refuse", 11)), (dict(lda=146), ("refuse", 12)),
    (dict(a_mode=1, M=302, lda=304), ("refuse", 13)), (dict(a_mode=1, lda=302), ("refuse", 13)), (dict(ldb=145), ("refuse", 14)), (dict(b_mode=1, ldb=530), ("refuse", 15)),
    (dict(b_mode=1, N=50, ldb=52), ("refuse", 15)), (dict(_FC, conv_Cin=6, conv_KH=2, conv_KW=2, K=24), ("refuse", 16)), (dict(_FC, K=40), ("refuse", 17)),
    (dict(_FC, conv_stride=0), ("refuse", 18)), (dict(_FC, conv_OW=0), ("refuse", 18)), (dict(split_k=2, act=1), ("refuse", 19)), (dict(split_k=2, Dpre=0x80000), ("refuse", 19)),
    (dict(split_k=2, rowscale=0x60000, rs_div=1, rs_mod=1), ("refuse", 19)), (dict(dropout_p=0.1), ("refuse", 20)), (dict(dropout_p=1.0, seed_dev=0x70000), ("refuse", 20)),
    (dict(rowscale=0x60000, rs_div=0, rs_mod=1), ("refuse", 21)), (dict(batch=4, **_FX), ("refuse", 22)), (dict(ksegs=4, **_FX), ("refuse", 22)), (dict(batch=2, ksegs=2, **_FX), ("refuse", 23)),
    (dict(ksegs=2, split_k=2, **_FX), ("refuse", 24)), (dict(_FC, ksegs=2, **_FX), ("refuse", 24)), (dict(a_mode=1, M=300, lda=300, batch=2, a_rowsum=0xC0000, **_FX), ("refuse", 24)),
    (dict(ksegs=2, A_x1=0x11000), ("refuse", 25)), (dict(ksegs=2, A_x1=0x11004, B_x1=0x21000), ("refuse", 25)), (dict(ksegs=3, A_x1=0x11000, B_x1=0x21000), ("refuse", 26)),
    (dict(batch=2, A_x1=0x11000, B_x1=0x21000), ("refuse", 27)), (dict(batch=3, A_x1=0x11000, B_x1=0x21000, A_x2=0x12000, B_x2=0x22000, D_x1=0x31000), ("refuse", 27)),
    (dict(batch=2, residual=0x50000, **_FX), ("refuse", 28)), (dict(batch=2, atomic=1, **_FX), ("refuse", 28)), (dict(a_rowsum=0xC0000), ("refuse", 29)),
    (dict(_FC, a_rowsum=0xC0000), ("refuse", 29)), (dict(_FC, b_mode=1), ("refuse", 30)), (dict(b_mode=2), ("refuse", 30)),
]


def test_gemm_f32_class_table():
    """helpers.gemm_f32_class against a table written by hand from vptr_gemm's checks, its split / tile arithmetic, launch_one's loop choice and
    the kernels' epilogue choice; every (loop, epilogue, NFN) combination and every refusal appears in it"""
    from helpers import gemm_f32_class, gemm_f32_plan
    import gemm_f32_cases as C
    bad = []
    for change, want in GEMM_F32_TABLE:
        got = gemm_f32_class(dict(_F, **change))
        if got != want:
            bad.append((change, got, want))
    assert not bad, bad
    assert {w[:3] for _, w in GEMM_F32_TABLE if w[0] != "refuse"} == set(C.LOOPS_EPIS)
    assert {w[1] for _, w in GEMM_F32_TABLE if w[0] == "refuse"} == set(C.REJECTS) - {0}      # 0: the null descriptor, no fields to mirror
    plan = gemm_f32_plan(dict(_F, K=100, split_k=7))
    assert (plan["k_chunk"], plan["splits"], plan["grid"]) == (32, 4, 36)


def test_gemm_f32_cases_census():
    """the issue's census: the ten (loop, epilogue, NFN) combinations by two cases or more and once with the full epilogue option set at
    precision 3; the five operand-mode pairs, both B stagers at every NFN and every stager at precision 1, in both loops; the named grid sizes"""
    import gemm_f32_cases as C
    census = C.class_census()
    assert not C.census_gaps(census), C.census_gaps(census)
    assert sum(len(v) for v in census.values()) == len(C.CASES)
    assert {1, 3, 7, 9, 13, 385} <= {C.SPEC[n].get("grid") for n in C.CASES}


GEMM_F32_PARTS = 8


@pytest.mark.parametrize("part", range(GEMM_F32_PARTS))
def test_gemm_f32_cases_against_emulation(part, capsys):
    """every case of tests/test_01c_gemm_f32_abi_gpu.py against the fp32 CPU emulation of the call: descriptors, pitches, guards, references and
    bars of the CASES; the emulation's fp32 arithmetic stays inside every bar, and the fp64 reference alone leaves at most 1 % of a case's
    elements to the kink rule (asserted per case by the runner)"""
    import gemm_f32_cases as C
    be = C.EmuBackend()
    for name in C.CASES[part::GEMM_F32_PARTS]:
        _, figures = C.run_case(be, name)
        assert all(w <= 1.0 for w, _ in figures)
    if part == 0:
        for k in C.REJECTS:
            C.run_reject(be, k)


# mutation -> cases that have to notice it (at least one each; every listed case must fail).  a_tail_unmasked: the kernel zeroes the K tail in A
# only and leaves B's clamped loads in place, so the mutation accumulates the products of the two clamped tails
GEMM_F32_MUTATION_CASES = {
    "a_tail_unmasked": ["kc_K36", "kc_K4", "ksks_K33", "kskc_K36", "conv3s1_zero"], "reflect_off_by_one": ["conv3s1_reflect", "conv_map2x3", "conv_map3x2"],
    "parity_dropped": ["convT_s2", "convT_s3"], "seg3_reads_seg2": ["kseg3_K48", "kseg3_ksks"], "d_row_off_ignored": ["subpixel_c12", "subpixel_c6"],
    "bias_every_split": ["split2", "split7", "conv_split2"], "rowsum_clamped_rows": ["rowsum_tiles", "rowsum_split"],
    "drop_index_ldd": ["full_rows4", "full_frag4", "rows_drop_nores"], "lo_dropped": ["kc_K68", "ksks_K65", "conv3s2_zero"],
}


@pytest.mark.parametrize("mut", sorted(GEMM_F32_MUTATION_CASES))
def test_gemm_f32_cases_notice_mutations(mut, capsys):
    """each named mutation of the emulation makes every case listed for it fail (and the unmutated emulation passes them, above)"""
    import gemm_f32_cases as C
    assert sorted(GEMM_F32_MUTATION_CASES) == sorted(C.MUTATIONS)
    be = C.EmuBackend(mut=mut)
    for name in GEMM_F32_MUTATION_CASES[mut]:
        with pytest.raises(AssertionError):
            C.run_case(be, name)


# ---- the 7x7 end convolutions through the C ABI (tests/test_09k_conv7_abi_gpu.py): cases, launch classes, mutations
def test_conv7_cases_land_in_their_launch_classes():
    """the launchers' selection arithmetic restated (helpers.conv7_class): every case of tests/conv7_cases.py reaches the class it names (asserted
    by the runner as well, case by case), every class is reached, and the walks the cases were chosen for are the ones they take"""
    import conv7_cases as C
    from helpers import CONV7_CLASSES, conv7_class
    census = C.class_census()
    assert set(census) == set(CONV7_CLASSES), sorted(set(census) ^ set(CONV7_CLASSES))
    for (B, Cimg, H, W), c in C.IN_FWD.items():
        assert conv7_class("in_fwd", B=B, Cimg=Cimg, H=H, W=W)["class"] == "in_fwd/" + c
    for (B, Cimg, H, W), c in C.IN_PLANES.items():
        assert conv7_class("in_fwd_planes", B=B, Cimg=Cimg, H=H, W=W)["class"] == "in_fwd_planes/" + c
    for (B, Cimg, H, W), c in C.OUT_FWD.items():
        assert conv7_class("out_fwd", B=B, Cimg=Cimg, H=H, W=W)["class"] == "out_fwd/" + c
    for (B, Cimg, H, W, Cin), c in C.OUT_DX.items():
        assert conv7_class("out_bwd_data", B=B, Cimg=Cimg, H=H, W=W, Cin=Cin)["class"] == "out_bwd_data/" + c
    for (B, Cimg, H, W), c in C.OUT_DW.items():
        assert conv7_class("out_bwd_weight", B=B, Cimg=Cimg, H=H, W=W)["class"] == "out_bwd_weight/" + c
    for (B, Cimg, H, W), c in C.OUT_WS.items():
        assert conv7_class("out_bwd_weight_ws", B=B, Cimg=Cimg, H=H, W=W)["class"] == "out_bwd_weight_ws/" + c

    def k(op, B, Cimg, H, W, **kw):
        return conv7_class(op, B=B, Cimg=Cimg, H=H, W=W, **kw)
    # conv7_in: a second band of one row; nq = 16; a second chunk of one quad; three chunks; the LDS sizes past 64 KB; partial last workgroups
    assert k("in_fwd", 1, 1, 9, 8)["last_band_rows"] == 1
    assert (k("in_fwd", 2, 3, 8, 64)["chunks"], k("in_fwd", 2, 3, 8, 64)["last_nq"]) == (1, 16)
    assert (k("in_fwd", 1, 3, 8, 68)["chunks"], k("in_fwd", 1, 3, 8, 68)["last_nq"]) == (2, 1)
    assert k("in_fwd", 1, 3, 5, 132)["chunks"] == 3
    assert k("in_fwd", 1, 3, 4, 384)["lds"] == 65856 and k("in_fwd", 1, 3, 4, 380)["class"] == "in_fwd/fwd2c"
    assert k("in_fwd", 1, 4, 4, 288)["lds"] == 66304 and k("in_fwd", 1, 4, 4, 284)["class"] == "in_fwd/fwd2c"
    assert k("in_fwd", 1, 4, 4, 512)["lds"] == 116480
    assert k("in_fwd", 1, 1, 9, 11)["last_pixels"] == 35 and k("in_fwd", 3, 3, 5, 7)["last_pixels"] == 41
    assert [k("in_bwd_weight", *g)["last_pixels"] for g in ((1, 1, 23, 89), (1, 1, 32, 64), (1, 1, 25, 82), (2, 1, 25, 82))] == [2047, 2048, 2, 4]
    assert [k("in_bwd_weight", *g)["chunks"] for g in ((1, 1, 23, 89), (1, 1, 32, 64), (1, 1, 25, 82), (2, 1, 25, 82))] == [1, 1, 2, 3]
    assert not any(h > 3 and 2049 % h == 0 and 2049 // h > 3 for h in range(1, 2050))       # why 2050 stands in for 2049
    # conv7_out_fwd: three patches in one partial workgroup, gridDim.y = 3
    assert k("out_fwd", 3, 3, 4, 16)["grid"] == (1, 3) and k("out_fwd", 3, 3, 4, 16)["last_waves"] == 3
    # conv7_out_bwd_data: partial bands, the LDS limit between H = 73 and 74, ngrp 2 / 4 / 8
    assert [k("out_bwd_data", 1, 1, h, 64)["last_band_rows"] for h in (7, 8, 9, 20)] == [7, 8, 1, 4]
    assert k("out_bwd_data", 1, 3, 73, 64)["lds"] == 81600 and k("out_bwd_data", 1, 3, 74, 64)["class"] == "out_bwd_data/gen1"
    assert [k("out_bwd_data", 1, 2, 8, 8, Cin=c)["ngrp"] for c in (32, 64, 128)] == [2, 4, 8]
    # weight gradients: ragged frame groups; 3 - 33 partials; the attribute branch and the 150 KB fallback
    assert [k("out_bwd_weight", *g)["last_frames"] for g in C.OUT_DW] == [1, 1, 16, 1]
    assert sorted(k("out_bwd_weight_ws", *g)["partials"] for g in C.OUT_WS if g[1:] == (1, 8, 8)) == [3, 12, 15, 18, 33]
    assert k("out_bwd_weight_ws", 1, 1, 8, 2048)["lds"] == 99072 and k("out_bwd_weight_ws", 1, 1, 8, 4096)["reason"] == "lds"


@pytest.mark.parametrize("part", range(4))
def test_conv7_cases_against_emulation(part, capsys):
    """every case of tests/test_09k_conv7_abi_gpu.py against the fp64 CPU emulation of the calls: argument orders, layouts, guards, references
    and bars of the CASES"""
    import conv7_cases as C
    be = C.EmuBackend()
    if part == 0:
        for g in C.IN_FWD:
            for s in (True, False):
                C.run_in_fwd(be, g, s)
        C.run_in_fwd_rejects(be)
        for g in C.IN_PLANES:
            C.run_in_planes(be, g)
        C.run_in_planes_rejects(be)
    elif part == 1:
        for c in C.in_dw_cases():
            C.run_in_dw(be, *c)
        C.run_in_dw_rejects(be)
        for g in C.OUT_FWD:
            m = C.run_out_fwd(be, g)
            assert max(m.values()) <= 2.0 ** -23        # the emulation's activations are fp64 values rounded once
        C.run_out_fwd_rejects(be)
    elif part == 2:
        for g in C.OUT_DX:
            for a in C.ACTS:
                C.run_out_dx(be, g, a)
        C.run_out_dx_rejects(be)
    else:
        for g in C.OUT_DW:
            for a in C.ACTS:
                C.run_out_dw(be, g, a)
        C.run_out_dw_rejects(be)
        for g in C.OUT_WS:
            for det in (0, 1):
                C.run_out_ws(be, g, C.TANH if det else C.SIGMOID, det)
        C.run_out_ws(be, (2, 3, 9, 11), C.NONE, 0, with_db=False)
        for name in C.OUT_WS_FALLBACKS:
            C.run_out_ws_fallback(be, name)
        C.run_out_ws_rejects(be)


# mutation of the emulation -> cases that have to notice it (every one listed must fail)
CONV7_MUTATION_CASES = {
    "replicate": [("run_in_fwd", (2, 1, 4, 4), False), ("run_out_fwd", (1, 1, 4, 16)), ("run_out_dx", (2, 1, 7, 7, 64), 0), ("run_out_ws", (2, 3, 9, 11), 1, 0),
                  ("run_in_dw", 1, 1, 23, 89, 0)],
    "dx_fold_dropped": [("run_out_dx", (1, 1, 7, 64, 64), 1), ("run_out_dx", (2, 1, 7, 7, 64), 0)],
    "kykx_swapped": [("run_in_fwd", (1, 1, 9, 11), True), ("run_in_planes", (1, 3, 8, 68)), ("run_out_fwd", (2, 3, 9, 11)), ("run_out_dx", (1, 3, 9, 64, 64), 2),
                     ("run_out_dw", (1, 1, 8, 8), 1), ("run_in_dw", 1, 3, 32, 64, 1)],
    "sigmoid_grad_dy": [("run_out_dx", (1, 1, 8, 64, 64), 2), ("run_out_dw", (5, 3, 8, 16), 2), ("run_out_ws", (1, 1, 8, 8), 2, 0)],
    "dw_overwritten": [("run_out_dw", (1, 1, 8, 8), 0), ("run_out_ws", (4, 1, 8, 8), 1, 1), ("run_out_ws_fallback", "null"), ("run_in_dw", 1, 1, 25, 82, 0)],
    "planes_swapped": [("run_in_planes", (2, 1, 4, 4)), ("run_in_planes", (1, 3, 4, 384))],
    "chunk_off_by_quad": [("run_in_fwd", (1, 3, 8, 68), True), ("run_in_fwd", (1, 3, 5, 132), False), ("run_in_planes", (1, 3, 8, 68))],
}


@pytest.mark.parametrize("mut", sorted(CONV7_MUTATION_CASES))
def test_conv7_cases_notice_mutations(mut, capsys):
    """each named defect of the emulation -- replicate instead of reflect, the top border's mirror fold missing from dx, ky and kx swapped, the
    sigmoid's gradient taken from dy alone, dw overwritten instead of accumulated, the hi / lo plane halves swapped, the 64-column chunk boundary
    one quad early -- makes every case listed for it fail (and the unmutated emulation passes them, above)"""
    import conv7_cases as C
    assert sorted(CONV7_MUTATION_CASES) == sorted(C.MUTATIONS)
    be = C.EmuBackend(mut=mut)
    for fn, *args in CONV7_MUTATION_CASES[mut]:
        with pytest.raises(AssertionError):
            getattr(C, fn)(be, *args)
