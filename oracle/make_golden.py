"""TEST INFRASTRUCTURE -- container-only: validate the oracle against the imported reference and
write the golden fixtures under tests/golden/.

Run:  python -m oracle.make_golden            (from /root/repo; needs /root/reference)

What it does
  1. imports the real reference (oracle/ref_import.py), builds its modules with a deterministic
     RandomState fill (oracle/fill.py), dropout = 0;
  2. runs reference forward/backward and the oracle restatement on the same tensors and asserts
     agreement (fp64: <= 1e-10 rel-L2, fp32: <= 2e-5);
  3. saves inputs, expected outputs and expected gradients as .npz (tiny configs: full tensors;
     full-size K64 config: per-tensor L2 norms + 2048 sampled elements).

Fixtures are data only (arrays + JSON strings); no reference source or pickled reference objects -- with one
exception: ckpt_ref_nar24.tar is a checkpoint file as the reference's save_ckpt writes it (tensors, a loss history of
utils.train_summary.Loss_tuple instances; its embedded source-tree copy stubbed out), because reading such a file is
what the checkpoint-interchange test checks.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import fill, vptr_oracle as O  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def template_of(sd):
    return [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items()]


def np_sd(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


def build_nar(ref, cfg, seed, far=False):
    if far:
        m = ref.VPTRFormerFAR(cfg["Tp"], cfg["Tf"], cfg["H"], cfg["W"], cfg["C"], cfg["nhead"],
                              cfg["num_encoder_layers"], 0.0, cfg["window_size"], 4, cfg["rpe"])
    else:
        m = ref.VPTRFormerNAR(cfg["Tp"], cfg["Tf"], cfg["H"], cfg["W"], cfg["C"], cfg["nhead"],
                              cfg["num_encoder_layers"], cfg["num_decoder_layers"], 0.0, cfg["window_size"], 4,
                              bool(cfg.get("TSLMA", False)), cfg["rpe"])
    fill.apply_fill(m, seed)
    return m


def transformer_case(ref, name, cfg, far, N, seed, full=True, check64=True):
    torch.manual_seed(0)
    m = build_nar(ref, cfg, seed, far)
    Tin = cfg.get("Tin", cfg["Tp"])
    Tout = Tin if far else cfg["Tf"]
    x = fill.rand_normal((N, Tin, cfg["C"], cfg["H"], cfg["W"]), seed + 1).abs()  # encoder output is post-ReLU
    g = fill.rand_normal((N, Tout, cfg["C"], cfg["H"], cfg["W"]), seed + 2)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    # keep the cotangent away from the kink of the final ReLU: an implementation that differs by 1e-6 may flip
    # relu'(y) at |y| ~ 0, which is an O(1) change of that element's gradient and not a parity defect.
    with torch.no_grad():
        _, pre = (O.far_forward if far else O.nar_forward)({k: v.clone() for k, v in sd0.items()}, x, cfg, training=True,
                                                           return_pre=True)
    kink = (pre.abs() < 2e-3).reshape(-1).nonzero().reshape(-1)
    g.reshape(-1)[kink] = 0.0

    # ---- reference: train-mode fwd/bwd (dropout 0 => deterministic; BN uses batch statistics)
    m.train()
    xr = x.clone().requires_grad_(True)
    out_r = m(xr)
    (out_r * g).sum().backward()
    grads_r = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    sd_after = {k: v.clone() for k, v in m.state_dict().items()}
    # ---- reference: eval-mode fwd from the ORIGINAL state
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        out_eval_r = m(x)

    # ---- oracle on the same state
    fwd = O.far_forward if far else O.nar_forward
    P = {k: v.clone() for k, v in sd0.items()}
    leaves = {}
    for k, _ in m.named_parameters():
        P[k] = P[k].clone().requires_grad_(True)
        leaves[k] = P[k]
    xo = x.clone().requires_grad_(True)
    out_o = fwd(P, xo, cfg, training=True)
    (out_o * g).sum().backward()
    e_out = rel(out_o, out_r)
    e_dx = rel(xo.grad, xr.grad)
    e_g = 0.0
    for k in grads_r:
        # gradients that are analytically zero (k-bias: softmax shift invariance) are pure round-off: use an
        # absolute floor tied to the typical gradient scale
        floor = 1e-2 * float(np.median([float(v.norm()) for v in grads_r.values()]))
        e = float((leaves[k].grad.double() - grads_r[k].double()).norm() / (grads_r[k].double().norm() + floor))
        if e > 1e-4:
            print("   grad mismatch", k, e, float(grads_r[k].norm()))
        e_g = max(e_g, e)
    assert all((leaves[k].grad is None) == (k not in grads_r) for k in leaves)
    P2 = {k: v.clone() for k, v in sd0.items()}
    with torch.no_grad():
        out_eval_o = fwd(P2, x, cfg, training=False)
    e_eval = rel(out_eval_o, out_eval_r)
    e_bn = 0.0
    for k in sd_after:
        if k.endswith("running_mean") or k.endswith("running_var"):
            e_bn = max(e_bn, rel(P[k], sd_after[k]))
    print(f"[{name}] fp32 oracle-vs-ref: out {e_out:.2e} dx {e_dx:.2e} dparam(max) {e_g:.2e} eval {e_eval:.2e} bn {e_bn:.2e}")
    # two fp32 evaluation orders of the same formulas: 2e-5 on the small nets; the full-size digests (windows of 64 tokens,
    # up to 50 time steps, 12 layers) accumulate a few 1e-5 more -- the fp64 comparison on the tiny cases pins exactness
    lim = 2e-5 if full else 1e-4
    assert max(e_out, e_dx, e_eval, e_bn) < lim and e_g < 10 * lim, name

    if check64:
        m64 = build_nar(ref, cfg, seed, far).double().train()
        o64 = m64(x.double())
        P64 = {k: v.double() for k, v in sd0.items()}
        oo64 = fwd(P64, x.double(), cfg, training=True)
        e64 = rel(oo64, o64)
        print(f"[{name}] fp64 oracle-vs-ref: out {e64:.2e}")
        assert e64 < 1e-10, name

    save = {"cfg": json.dumps(cfg), "far": np.array(int(far)), "seed": np.array(seed), "N": np.array(N),
            "template": json.dumps(template_of(sd0)), "g_zero_idx": kink.numpy()}
    if full:
        save.update({"x": x.numpy(), "g": g.numpy(), "out_train": out_r.detach().numpy(), "out_eval": out_eval_r.numpy(),
                     "dx": xr.grad.numpy()})
        for k, v in grads_r.items():
            save["grad:" + k] = v.numpy()
        for k, v in sd_after.items():
            if k.endswith("running_mean") or k.endswith("running_var"):
                save["bn_after:" + k] = v.numpy()
        for k in ("temporal_pos", "lw_pos", "Tlw_pos"):
            if k in sd0:
                save["buf:" + k] = sd0[k].numpy()
    else:
        n, s = fill.digest(out_r)
        save["out_train_norm"], save["out_train_samples"] = np.array(n), s
        n, s = fill.digest(out_eval_r)
        save["out_eval_norm"], save["out_eval_samples"] = np.array(n), s
        n, s = fill.digest(xr.grad)
        save["dx_norm"], save["dx_samples"] = np.array(n), s
        gn = {}
        for k, v in grads_r.items():
            n, s = fill.digest(v, count=256)
            gn[k] = n
            save["gsamp:" + k] = s
        save["grad_norms"] = json.dumps(gn)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def ae_case(ref, name, img_ch, feat, HW, N, T, padding_type, out_layer, seed):
    enc = ref.VPTREnc(img_ch, feat_dim=feat, n_downsampling=3, padding_type=padding_type)
    dec = ref.VPTRDec(img_ch, feat_dim=feat, n_downsampling=3, out_layer=out_layer, padding_type=padding_type)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    enc.eval(), dec.eval()
    x = fill.rand_input((N, T, img_ch, HW, HW), seed + 1, -0.25, 0.25)
    g = fill.rand_normal((N, T, img_ch, HW, HW), seed + 2)
    with torch.no_grad():
        f_r = enc(x)
    fin = f_r.clone().requires_grad_(True)
    y_r = dec(fin)
    (y_r * g).sum().backward()
    dgr = {k: p.grad.clone() for k, p in dec.named_parameters()}
    Pe, Pd = dict(enc.state_dict()), {k: v.clone() for k, v in dec.state_dict().items()}
    for k, _ in dec.named_parameters():
        Pd[k].requires_grad_(True)
    with torch.no_grad():
        f_o = O.enc_forward(Pe, x, padding_type=padding_type)
    fo_in = f_r.clone().requires_grad_(True)
    y_o = O.dec_forward(Pd, fo_in, out_layer=out_layer)
    (y_o * g).sum().backward()
    e = [rel(f_o, f_r), rel(y_o, y_r), rel(fo_in.grad, fin.grad), max(rel(Pd[k].grad, dgr[k]) for k in dgr)]
    print(f"[{name}] fp32 oracle-vs-ref: enc {e[0]:.2e} dec {e[1]:.2e} dfeat {e[2]:.2e} dparam {e[3]:.2e}")
    assert max(e) < 2e-5, name
    # train-mode (stage-1) forward for completeness
    enc.train(), dec.train()
    sd_e0, sd_d0 = {k: v.clone() for k, v in enc.state_dict().items()}, {k: v.clone() for k, v in dec.state_dict().items()}
    with torch.no_grad():
        y_tr = dec(enc(x))
    Pe2, Pd2 = {k: v.clone() for k, v in sd_e0.items()}, {k: v.clone() for k, v in sd_d0.items()}
    with torch.no_grad():
        y_tr_o = O.dec_forward(Pd2, O.enc_forward(Pe2, x, padding_type=padding_type, training=True), out_layer=out_layer,
                               training=True)
    print(f"[{name}] train-mode AE fwd: {rel(y_tr_o, y_tr):.2e}")
    assert rel(y_tr_o, y_tr) < 2e-5
    save = {"meta": json.dumps(dict(img_ch=img_ch, feat=feat, HW=HW, N=N, T=T, padding_type=padding_type,
                                    out_layer=out_layer, seed=seed)),
            "enc_template": json.dumps(template_of(sd_e0)), "dec_template": json.dumps(template_of(sd_d0)),
            "x": x.numpy(), "g": g.numpy(), "feat": f_r.numpy(), "y": y_r.detach().numpy(), "dfeat": fin.grad.numpy(),
            "y_train": y_tr.numpy()}
    for k, v in dgr.items():
        save["dgrad:" + k] = v.numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def ae_digest_case(ref, name, img_ch, feat, HW, N, T, padding_type, out_layer, seed):
    """FULL-SIZE auto-encoder (feat 528) at a given image size / channel count / padding: eval forward, decoder backward.
    Saves per-tensor norms + sampled elements (inputs are regenerated from the seeds by the test)."""
    enc = ref.VPTREnc(img_ch, feat_dim=feat, n_downsampling=3, padding_type=padding_type)
    dec = ref.VPTRDec(img_ch, feat_dim=feat, n_downsampling=3, out_layer=out_layer, padding_type=padding_type)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    enc.eval(), dec.eval()
    x = fill.rand_input((N, T, img_ch, HW, HW), seed + 1, -0.25, 0.25)
    g = fill.rand_normal((N, T, img_ch, HW, HW), seed + 2)
    with torch.no_grad():
        f_r = enc(x)
    fin = f_r.clone().requires_grad_(True)
    y_r = dec(fin)
    (y_r * g).sum().backward()
    dgr = {k: p.grad.clone() for k, p in dec.named_parameters()}
    Pe, Pd = dict(enc.state_dict()), {k: v.clone() for k, v in dec.state_dict().items()}
    for k, _ in dec.named_parameters():
        Pd[k].requires_grad_(True)
    with torch.no_grad():
        f_o = O.enc_forward(Pe, x, padding_type=padding_type)
    fo_in = f_r.clone().requires_grad_(True)
    y_o = O.dec_forward(Pd, fo_in, out_layer=out_layer)
    (y_o * g).sum().backward()
    e = [rel(f_o, f_r), rel(y_o, y_r), rel(fo_in.grad, fin.grad), max(rel(Pd[k].grad, dgr[k]) for k in dgr)]
    print(f"[{name}] fp32 oracle-vs-ref: enc {e[0]:.2e} dec {e[1]:.2e} dfeat {e[2]:.2e} dparam {e[3]:.2e}")
    assert max(e) < 5e-5, name
    save = {"meta": json.dumps(dict(img_ch=img_ch, feat=feat, HW=HW, N=N, T=T, padding_type=padding_type, out_layer=out_layer,
                                    seed=seed))}
    for tag, t in (("feat", f_r), ("y", y_r.detach()), ("dfeat", fin.grad)):
        n, smp = fill.digest(t)
        save[tag + "_norm"], save[tag + "_samples"] = np.array(n), smp
    gn = {}
    for k, v in dgr.items():
        n, smp = fill.digest(v, count=256)
        gn[k] = n
        save["gsamp:" + k] = smp
    save["grad_norms"] = json.dumps(gn)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def _notebook_rollouts():
    """The reference's own test-time rollout functions, executed from where they lie: the `def`s of Test_VPTR.ipynb cell 5
    (FAR_RIL_test_single_iter, FAR_RIP_test_single_iter, NAR_test_single_iter, NAR_BAIR_2_to_28_test_single_iter).  Nothing of
    the notebook is copied into this repository; the fixture holds inputs and the tensors these functions returned."""
    nb = json.load(open(os.path.join("/root/reference", "Test_VPTR.ipynb")))
    src = [''.join(c["source"]) for c in nb["cells"] if c["cell_type"] == "code" and "def FAR_RIP_test_single_iter" in ''.join(c["source"])]
    assert len(src) == 1
    ns = {"torch": torch}
    exec(compile(src[0], "Test_VPTR.ipynb:cell5", "exec"), ns)
    return ns


def rollout_case(ref, name, seed):
    """Test-time rollouts by the reference's notebook functions on the reference's modules (tiny sizes)."""
    nbf = _notebook_rollouts()
    feat, HW, N = 48, 64, 2
    enc = ref.VPTREnc(1, feat_dim=feat, n_downsampling=3, padding_type="reflect").eval()
    dec = ref.VPTRDec(1, feat_dim=feat, n_downsampling=3, out_layer="Sigmoid", padding_type="reflect").eval()
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 1)
    cpu = torch.device("cpu")
    save = {"meta": json.dumps(dict(feat=feat, HW=HW, N=N, seed=seed))}
    # FAR: Tp = 3, num_future_frames = 3, five predictions -> the window slides for i >= 3
    cfg_far = dict(Tp=3, Tf=3, H=8, W=8, C=feat, nhead=8, window_size=4, num_encoder_layers=2, rpe=True)
    far = build_nar(ref, cfg_far, seed + 2, far=True).eval()
    past = fill.rand_input((N, 3, 1, HW, HW), seed + 3)
    fut = fill.rand_input((N, 5, 1, HW, HW), seed + 4)
    with torch.no_grad():
        rip, _ = nbf["FAR_RIP_test_single_iter"]((past, fut), enc, dec, far, 5, cpu)
        ril, _ = nbf["FAR_RIL_test_single_iter"]((past, fut), enc, dec, far, 5, cpu)
    save.update(cfg_far=json.dumps(cfg_far), far_past=past.numpy(), far_rip=rip.numpy(), far_ril=ril.numpy())
    # NAR, feature-chained rounds: Tp = Tf = 2, four predictions
    cfg_nar = dict(Tp=2, Tf=2, H=8, W=8, C=feat, nhead=8, window_size=4, num_encoder_layers=1, num_decoder_layers=1, rpe=True)
    nar = build_nar(ref, cfg_nar, seed + 5).eval()
    past = fill.rand_input((N, 2, 1, HW, HW), seed + 6)
    fut = fill.rand_input((N, 4, 1, HW, HW), seed + 7)
    with torch.no_grad():
        chained, _ = nbf["NAR_test_single_iter"]((past, fut), enc, dec, nar, 4, cpu)
    save.update(cfg_nar=json.dumps(cfg_nar), nar_past=past.numpy(), nar_chained=chained.numpy())
    # NAR, the BAIR 2 -> 28 recipe (three re-encoded rounds, the last one trimmed by two frames): Tp = 2, Tf = 4 -> 10 frames
    cfg_b = dict(Tp=2, Tf=4, H=8, W=8, C=feat, nhead=8, window_size=4, num_encoder_layers=1, num_decoder_layers=2, rpe=True)
    narb = build_nar(ref, cfg_b, seed + 8).eval()
    past = fill.rand_input((N, 2, 1, HW, HW), seed + 9)
    fut = fill.rand_input((N, 10, 1, HW, HW), seed + 10)
    with torch.no_grad():
        bair, _ = nbf["NAR_BAIR_2_to_28_test_single_iter"]((past, fut), enc, dec, narb, 10, cpu)
    assert bair.shape[1] == 10
    save.update(cfg_bair=json.dumps(cfg_b), bair_past=past.numpy(), bair_frames=bair.numpy())
    # train_FAR.py:103-125 (test_phase=True) is covered by tests against the oracle loops; here also through the reference modules
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)
    print(f"[{name}] rollouts: RIP {tuple(rip.shape)} RIL {tuple(ril.shape)} NAR {tuple(chained.shape)} BAIR {tuple(bair.shape)}")


def losses_case(ref, name, seed):
    N, T, C, h, w = 2, 3, 24, 8, 8
    gt = fill.rand_normal((N, T, 1, 64, 64), seed)
    pr = fill.rand_normal((N, T, 1, 64, 64), seed + 1).requires_grad_(True)
    gf = fill.rand_normal((N, T, C, h, w), seed + 2)
    pf = fill.rand_normal((N, T, C, h, w), seed + 3).requires_grad_(True)
    mse, gdl, nce = ref.MSELoss(), ref.GDL(alpha=1), ref.BiPatchNCE(N, T, h, w, 1.0)
    l = gdl(gt, pr) + mse(pr, gt) + 0.1 * nce(F.normalize(gf, p=2.0, dim=2), F.normalize(pf, p=2.0, dim=2))
    l.backward()
    pr2, pf2 = pr.detach().clone().requires_grad_(True), pf.detach().clone().requires_grad_(True)
    l2 = O.gdl_loss(gt, pr2) + O.mse_loss(pr2, gt) + 0.1 * O.bipatch_nce(F.normalize(gf, p=2.0, dim=2),
                                                                        F.normalize(pf2, p=2.0, dim=2))
    l2.backward()
    e = [abs(l.item() - l2.item()) / abs(l.item()), rel(pr2.grad, pr.grad), rel(pf2.grad, pf.grad)]
    print(f"[{name}] losses: {e}")
    assert max(e) < 1e-5
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), gt=gt.numpy(), pr=pr.detach().numpy(), gf=gf.numpy(),
                        pf=pf.detach().numpy(), loss=np.array(l.item()), dpr=pr.grad.numpy(), dpf=pf.grad.numpy(),
                        mse=np.array(mse(pr, gt).item()), gdl=np.array(gdl(gt, pr).item()),
                        nce=np.array(nce(F.normalize(gf, p=2.0, dim=2), F.normalize(pf, p=2.0, dim=2)).item()))


clip_input = fill.clip_input


def step_case(ref, name, cfg, feat, HW, N, seed, steps=2, sample=0, out_layer="Tanh", norm="kth"):
    """single_iter recipe of train_NAR.py:49-107 with the real reference modules, dropout 0, no GAN.  out_layer="Sigmoid" +
    norm="raw" is the MovingMNIST configuration (Test_VPTR.ipynb cell 3; ResNetAutoEncoder.py:91-96; train_FAR.py:182)."""
    enc = ref.VPTREnc(1, feat_dim=feat, n_downsampling=3, padding_type="reflect").eval()
    dec = ref.VPTRDec(1, feat_dim=feat, n_downsampling=3, out_layer=out_layer, padding_type="reflect").eval()
    T = build_nar(ref, cfg, seed + 20)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    opt = torch.optim.AdamW(T.parameters(), lr=1e-4)
    mse, gdl = ref.MSELoss(), ref.GDL(alpha=1)
    nce = ref.BiPatchNCE(N, cfg["Tf"], cfg["H"], cfg["W"], 1.0)
    st = O.NARStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(T.state_dict()), cfg, out_layer=out_layer)
    recs = []
    for s in range(steps):
        past = clip_input((N, cfg["Tp"], 1, HW, HW), seed + 100 + s, norm)
        fut = clip_input((N, cfg["Tf"], 1, HW, HW), seed + 200 + s, norm)
        with torch.no_grad():
            pf, ff = enc(past), enc(fut)
        T.train()
        T.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        pred_f = T(pf)
        pred = dec(pred_f)
        a = T.NCE_projector(pred_f.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        b = T.NCE_projector(ff.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        l_mse, l_gdl = mse(pred, fut), gdl(fut, pred)
        l_pc = nce(F.normalize(b, p=2.0, dim=2), F.normalize(a, p=2.0, dim=2))
        loss = l_gdl + l_mse + 0.1 * l_pc
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(T.parameters(), max_norm=1.0, norm_type=2)
        opt.step()
        r = st.step(past, fut)
        rec = {"T_total": loss.item(), "T_GDL": l_gdl.item(), "T_MSE": l_mse.item(), "T_bpc": l_pc.item(),
               "grad_norm": float(gn)}
        for k in rec:
            assert abs(rec[k] - r[k]) <= 2e-4 * abs(rec[k]) + 1e-7, (k, rec[k], r[k])
        recs.append(rec)
    e = max(rel(st.P_T[k], v) for k, v in T.state_dict().items() if v.is_floating_point())
    print(f"[{name}] {steps} train steps: losses {recs}; post-step params oracle-vs-ref {e:.2e}")
    assert e < 1e-4
    meta = dict(feat=feat, HW=HW, N=N, seed=seed, steps=steps)
    if out_layer != "Tanh" or norm != "kth":      # the round 1-3 fixtures keep their exact meta
        meta.update(out_layer=out_layer, norm=norm)
    save = {"cfg": json.dumps(cfg), "meta": json.dumps(meta),
            "records": json.dumps(recs), "T_template": json.dumps(template_of(T.state_dict())),
            "enc_template": json.dumps(template_of(enc.state_dict())),
            "dec_template": json.dumps(template_of(dec.state_dict()))}
    for k, v in T.state_dict().items():
        if v.is_floating_point() and k not in ("temporal_pos", "lw_pos", "Tlw_pos"):
            if sample:  # full-size model: a strided sample of <= ~sample elements per tensor
                flat = v.flatten()
                save["post:T:" + k] = flat[::max(1, flat.numel() // sample)].numpy()
            else:
                save["post:" + k] = v.numpy()
    if sample:
        save["sample"] = np.array(sample)
        for drop in ("T_template", "enc_template", "dec_template"):
            save.pop(drop, None)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def nar_gan_step_case(ref, name, cfg, feat, HW, N, seed, steps=2, lam_gan=0.001):
    """single_iter of train_NAR.py:49-107 WITH its optional adversarial branch (VPTR_Disc, optimizer_D, lam_gan; :66-79)."""
    enc = ref.VPTREnc(1, feat_dim=feat, n_downsampling=3, padding_type="reflect").eval()
    dec = ref.VPTRDec(1, feat_dim=feat, n_downsampling=3, out_layer="Tanh", padding_type="reflect").eval()
    disc = ref.VPTRDisc(1, ndf=64, n_layers=3, norm_layer=torch.nn.BatchNorm2d)
    T = build_nar(ref, cfg, seed + 20)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    fill.apply_fill(disc, seed + 30)
    opt = torch.optim.AdamW(T.parameters(), lr=1e-4)
    opt_D = torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.5, 0.999))
    mse, gdl = ref.MSELoss(), ref.GDL(alpha=1)
    nce = ref.BiPatchNCE(N, cfg["Tf"], cfg["H"], cfg["W"], 1.0)
    gan = ref.GANLoss("vanilla", target_real_label=1.0, target_fake_label=0.0)
    st = O.NARStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(T.state_dict()), cfg, P_disc=dict(disc.state_dict()),
                   lam_gan=lam_gan)
    recs = []
    for s in range(steps):
        past = (fill.rand_input((N, cfg["Tp"], 1, HW, HW), seed + 100 + s) - 0.6013795) / 2.7570653
        fut = (fill.rand_input((N, cfg["Tf"], 1, HW, HW), seed + 200 + s) - 0.6013795) / 2.7570653
        with torch.no_grad():
            pf, ff = enc(past), enc(fut)
        T.train()
        T.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        pred_f = T(pf)
        pred = dec(pred_f)
        disc.train()
        for p in disc.parameters():
            p.requires_grad_(True)
        disc.zero_grad(set_to_none=True)
        l_fake = gan(disc(pred.detach().flatten(0, 1)), False)
        l_real = gan(disc(fut.flatten(0, 1)), True)
        loss_D = (l_fake + l_real) * 0.5 * lam_gan
        loss_D.backward()
        opt_D.step()
        for p in disc.parameters():
            p.requires_grad_(False)
        a = T.NCE_projector(pred_f.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        b = T.NCE_projector(ff.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        l_mse, l_gdl = mse(pred, fut), gdl(fut, pred)
        l_pc = nce(F.normalize(b, p=2.0, dim=2), F.normalize(a, p=2.0, dim=2))
        t_gan = gan(disc(pred.flatten(0, 1)), True)
        loss = l_gdl + l_mse + 0.1 * l_pc + lam_gan * t_gan
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(T.parameters(), max_norm=1.0, norm_type=2)
        opt.step()
        r = st.step(past, fut)
        rec = {"T_total": loss.item(), "T_GDL": l_gdl.item(), "T_MSE": l_mse.item(), "T_bpc": l_pc.item(), "grad_norm": float(gn),
               "Dtotal": loss_D.item(), "Dfake": l_fake.item(), "Dreal": l_real.item(), "T_gan": t_gan.item()}
        for k in rec:
            assert abs(rec[k] - r[k]) <= 2e-4 * abs(rec[k]) + 1e-7, (k, rec[k], r[k])
        recs.append(rec)
    e = max(rel(st.P_T[k], v) for k, v in T.state_dict().items() if v.is_floating_point())
    ed = max(rel(st.P_disc[k], v) for k, v in disc.state_dict().items() if v.is_floating_point())
    print(f"[{name}] {steps} NAR+GAN train steps: losses {recs}; post-step params oracle-vs-ref T {e:.2e} disc {ed:.2e}")
    assert e < 1e-4 and ed < 1e-4
    save = {"cfg": json.dumps(cfg), "meta": json.dumps(dict(feat=feat, HW=HW, N=N, seed=seed, steps=steps, lam_gan=lam_gan)),
            "records": json.dumps(recs)}
    for tag, mod in (("T", T), ("disc", disc)):
        for k, v in mod.state_dict().items():
            if v.is_floating_point() and k not in ("temporal_pos", "lw_pos", "Tlw_pos"):
                flat = v.flatten()
                save[f"post:{tag}:{k}"] = flat[::max(1, flat.numel() // 4096)].numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def far_step_case(ref, name, cfg, feat, HW, N, seed, steps=2, cimg=1, padding_type="reflect", out_layer="Sigmoid", norm="raw", sample=0):
    """single_iter recipe of train_FAR.py:48-101 with the real reference modules (VPTR_Disc = None), dropout 0.  cimg=3,
    padding_type="zero", out_layer="Tanh", norm="bair" is the BAIR configuration (train_FAR_mp.py:289-300, utils/dataset.py:47-50)."""
    enc = ref.VPTREnc(cimg, feat_dim=feat, n_downsampling=3, padding_type=padding_type).eval()
    dec = ref.VPTRDec(cimg, feat_dim=feat, n_downsampling=3, out_layer=out_layer, padding_type=padding_type).eval()
    T = build_nar(ref, cfg, seed + 20, far=True)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    opt = torch.optim.AdamW(T.parameters(), lr=1e-4)
    mse, gdl = ref.MSELoss(), ref.GDL(alpha=1)
    st = O.FARStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(T.state_dict()), cfg, padding_type=padding_type,
                   out_layer=out_layer)
    recs = []
    for s in range(steps):
        past = clip_input((N, cfg["Tp"], cimg, HW, HW), seed + 100 + s, norm)
        fut = clip_input((N, cfg["Tf"], cimg, HW, HW), seed + 200 + s, norm)
        with torch.no_grad():
            gt_feats = enc(torch.cat([past, fut[:, 0:-1, ...]], dim=1))
        T.train()
        T.zero_grad(set_to_none=True)
        dec.zero_grad(set_to_none=True)
        pred = dec(T(gt_feats))
        real = torch.cat([past[:, 1:, ...], fut], dim=1)
        l_mse, l_gdl = mse(pred, real), gdl(real, pred)
        loss = l_gdl + l_mse
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(T.parameters(), max_norm=1.0, norm_type=2)
        opt.step()
        r = st.step(past, fut)
        rec = {"T_total": loss.item(), "T_GDL": l_gdl.item(), "T_MSE": l_mse.item(), "grad_norm": float(gn)}
        for k in rec:
            assert abs(rec[k] - r[k]) <= 2e-4 * abs(rec[k]) + 1e-7, (k, rec[k], r[k])
        recs.append(rec)
    e = max(rel(st.P_T[k], v) for k, v in T.state_dict().items() if v.is_floating_point())
    print(f"[{name}] {steps} FAR train steps: losses {recs}; post-step params oracle-vs-ref {e:.2e}")
    assert e < 1e-4
    meta = dict(feat=feat, HW=HW, N=N, seed=seed, steps=steps, out_layer=out_layer)
    if cimg != 1 or padding_type != "reflect" or norm != "raw":
        meta.update(cimg=cimg, padding_type=padding_type, norm=norm)
    save = {"cfg": json.dumps(cfg), "meta": json.dumps(meta), "records": json.dumps(recs)}
    if not sample:
        save["T_template"] = json.dumps(template_of(T.state_dict()))
    for k, v in T.state_dict().items():
        if v.is_floating_point() and k not in ("temporal_pos", "lw_pos", "Tlw_pos"):
            if sample:
                flat = v.flatten()
                save["post:T:" + k] = flat[::max(1, flat.numel() // sample)].numpy()
            else:
                save["post:" + k] = v.numpy()
    if sample:
        save["sample"] = np.array(sample)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def ae_step_case(ref, name, cimg, feat, HW, N, T, seed, steps=2, lam_gan=0.01, out_layer="Tanh", norm="kth"):
    """single_iter recipe of train_AutoEncoder.py:44-78 with the real reference modules (train-mode BN, PatchGAN, Adam).
    out_layer="Sigmoid" + norm="raw" = MovingMNIST (train_AutoEncoder.py:132 comment, utils/dataset.py:36-39)."""
    enc = ref.VPTREnc(cimg, feat_dim=feat, n_downsampling=3, padding_type="reflect")
    dec = ref.VPTRDec(cimg, feat_dim=feat, n_downsampling=3, out_layer=out_layer, padding_type="reflect")
    disc = ref.VPTRDisc(cimg, ndf=64, n_layers=3, norm_layer=torch.nn.BatchNorm2d)
    fill.apply_fill(enc, seed)
    fill.apply_fill(dec, seed + 10)
    fill.apply_fill(disc, seed + 20)
    st = O.AEStep(dict(enc.state_dict()), dict(dec.state_dict()), dict(disc.state_dict()), lam_gan=lam_gan, out_layer=out_layer)
    opt_G = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=2e-4, betas=(0.5, 0.999))
    opt_D = torch.optim.Adam(disc.parameters(), lr=2e-4, betas=(0.5, 0.999))
    gan, mse, gdl = ref.GANLoss("vanilla", target_real_label=1.0, target_fake_label=0.0), ref.MSELoss(), ref.GDL(alpha=1)
    recs = []
    for s in range(steps):
        past = clip_input((N, T, cimg, HW, HW), seed + 100 + s, norm)
        fut = clip_input((N, T, cimg, HW, HW), seed + 200 + s, norm)
        x = torch.cat([past, fut], dim=1)
        enc.train(); enc.zero_grad(); dec.train(); dec.zero_grad()
        rec = dec(enc(x))
        disc.train()
        for p in disc.parameters():
            p.requires_grad_(True)
        disc.zero_grad(set_to_none=True)
        l_fake = gan(disc(rec.detach().flatten(0, 1)), False)
        l_real = gan(disc(x.flatten(0, 1)), True)
        loss_D = (l_fake + l_real) * 0.5 * lam_gan
        loss_D.backward()
        opt_D.step()
        for p in disc.parameters():
            p.requires_grad_(False)
        l_gan = gan(disc(rec.flatten(0, 1)), True)
        l_mse, l_gdl = mse(rec, x), gdl(x, rec)
        loss_G = lam_gan * l_gan + l_mse + l_gdl
        loss_G.backward()
        opt_G.step()
        rec_ = {"AEgan": l_gan.item(), "AE_MSE": l_mse.item(), "AE_GDL": l_gdl.item(), "AE_total": loss_G.item(),
                "Dtotal": loss_D.item(), "Dfake": l_fake.item(), "Dreal": l_real.item()}
        r = st.step(past, fut)
        for k in rec_:
            assert abs(rec_[k] - r[k]) <= 2e-4 * abs(rec_[k]) + 1e-7, (k, rec_[k], r[k])
        recs.append(rec_)
    errs = [max(rel(P[k], v) for k, v in mod.state_dict().items() if v.is_floating_point())
            for P, mod in ((st.P_enc, enc), (st.P_dec, dec), (st.P_disc, disc))]
    print(f"[{name}] {steps} AE train steps: losses {recs}; post-step params oracle-vs-ref enc/dec/disc {errs}")
    assert max(errs) < 1e-4
    meta = dict(cimg=cimg, feat=feat, HW=HW, N=N, T=T, seed=seed, steps=steps, lam_gan=lam_gan)
    if out_layer != "Tanh" or norm != "kth":
        meta.update(out_layer=out_layer, norm=norm)
    save = {"meta": json.dumps(meta), "records": json.dumps(recs)}
    for tag, mod in (("enc", enc), ("dec", dec), ("disc", disc)):
        for k, v in mod.state_dict().items():
            if v.is_floating_point():  # strided sample of <= ~4096 elements per tensor keeps the fixture small (the disc has 2.8 M)
                flat = v.flatten()
                save[f"post:{tag}:{k}"] = flat[::max(1, flat.numel() // 4096)].numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def metrics_case(ref, name):
    """utils/metrics.py PSNR / MSEScore / SSIM of the real reference on seeded image batches"""
    import utils.metrics as RM
    save, out = {}, {}
    for tag, (n, c, h, w) in (("a", (3, 1, 32, 32)), ("b", (2, 3, 20, 28))):
        x, y = fill.rand_input((n, c, h, w), 301), fill.rand_input((n, c, h, w), 302)
        y = 0.8 * x + 0.2 * y
        save["x:" + tag], save["y:" + tag] = x.numpy(), y.numpy()
        out[tag] = {"psnr": RM.PSNR(x, y), "psnr255": RM.PSNR(x * 255, y * 255, 255), "mse": RM.MSEScore(x, y),
                    "ssim": float(RM.SSIM()(x, y)), "ssim_each": RM.SSIM(size_average=False)(x, y).tolist()}
    save["expected"] = json.dumps(out)
    print(f"[{name}] {out}")
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def pos_case(ref, name):
    from utils.position_encoding import PositionEmbeddding1D, PositionEmbeddding2D, PositionEmbeddding3D
    from utils.misc import NestedTensor
    save = {}
    for (T, E, ws) in [(6, 96, 4), (20, 528, 4), (50, 528, 8)]:
        t1 = PositionEmbeddding1D()(L=T, N=1, E=E)[:, 0, :]
        t2 = PositionEmbeddding2D()(N=1, E=E, H=ws, W=ws)[0].permute(1, 2, 0)
        t3 = PositionEmbeddding3D(E=E, T=T)(NestedTensor(torch.empty(T, E, ws, ws), None))[0].permute(1, 2, 3, 0)
        assert rel(O.pos1d(T, E), t1) < 1e-6 and rel(O.pos2d(E, ws, ws), t2) < 1e-6 and rel(O.pos3d(E, T, ws, ws), t3) < 1e-6
        tag = f"{T}_{E}_{ws}"
        save["p1:" + tag], save["p2:" + tag] = t1.numpy(), t2.numpy()
        if E == 96:
            save["p3:" + tag] = t3.numpy()
        else:
            n, s = fill.digest(t3)
            save["p3n:" + tag], save["p3s:" + tag] = np.array(n), s
    from model.MultiHeadAttentionRPE import MultiheadAttentionRPE
    for ws in (4, 8):
        idx = MultiheadAttentionRPE(16, 2, rpe=True, window_size=ws).relative_position_index
        assert torch.equal(idx, O.rpe_index(ws))
        save[f"rpe_index:{ws}"] = idx.numpy()
    print(f"[{name}] position tables + RPE index match")
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **save)


def ckpt_case(ref, name, seed):
    """a checkpoint file written by the reference's own save_ckpt (utils/train_summary.py:130-147): a small VPTRFormerNAR
    (d 24, 4 heads, 1 + 1 layers, filled with `seed`), an un-stepped AdamW, a one-entry loss history, epoch 2.  The writer's
    `read_code_files` is stubbed to {} for this one call, so the file carries no copy of the reference's source tree under
    'code' -- only tensors, the loss history and the pickle globals the reference's load_ckpt resolves.
    -> tests/golden/<name>.tar (tests/test_cpu.py::test_checkpoint_interop_with_reference)"""
    import shutil
    import tempfile
    import utils.train_summary as RS
    Tr = ref.VPTRFormerNAR(2, 2, 8, 8, 24, 4, 1, 1, 0.0, 4, 4, False, True)
    fill.apply_fill(Tr, seed)
    opt = torch.optim.AdamW(Tr.parameters(), lr=1e-4)
    ld = RS.init_loss_dict(["T_MSE"])
    ld["T_MSE"].val.append(0.25)
    code, RS.read_code_files = RS.read_code_files, lambda: {}
    tmp = tempfile.mkdtemp()
    try:
        RS.save_ckpt({"VPTR_Transformer": Tr}, {"optimizer_T": opt}, 2, ld, tmp)
        shutil.copyfile(os.path.join(tmp, "epoch_2.tar"), os.path.join(GOLD, name + ".tar"))
    finally:
        RS.read_code_files = code
        shutil.rmtree(tmp, ignore_errors=True)
    print(f"[{name}] reference checkpoint written ({os.path.getsize(os.path.join(GOLD, name + '.tar'))} bytes)")


def main():
    """python oracle/make_golden.py [fixture names ...]   (no names: regenerate every fixture)"""
    os.makedirs(GOLD, exist_ok=True)
    ref = import_reference()
    torch.set_num_threads(8)
    tiny = dict(Tp=3, Tf=3, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=1, num_decoder_layers=1, rpe=True)
    k64 = dict(Tp=10, Tf=10, H=8, W=8, C=528, nhead=8, window_size=4, num_encoder_layers=4, num_decoder_layers=8, rpe=True)
    far = dict(Tp=2, Tf=10, Tin=11, H=8, W=8, C=528, nhead=8, window_size=4, num_encoder_layers=12, rpe=True)
    far_tiny = dict(Tp=3, Tf=2, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=2, rpe=False)
    cases = [
        ("pos_tables", lambda n: pos_case(ref, n)),
        ("nar_tiny", lambda n: transformer_case(ref, n, tiny, False, 2, 11)),
        ("nar_tiny_norpe", lambda n: transformer_case(ref, n, dict(tiny, rpe=False), False, 2, 12)),
        ("far_tiny", lambda n: transformer_case(ref, n, dict(tiny, Tin=5, num_encoder_layers=2), True, 2, 13)),
        ("nar_tiny_pad", lambda n: transformer_case(ref, n, dict(tiny, H=6, W=6, Tp=2, Tf=2), False, 1, 14)),
        ("nar_tiny_T", lambda n: transformer_case(ref, n, dict(tiny, Tp=2, Tf=4, num_decoder_layers=2), False, 1, 15)),
        ("nar_tiny_tslma", lambda n: transformer_case(ref, n, dict(tiny, Tp=2, TSLMA=True, num_decoder_layers=2), False, 2, 16)),
        ("nar_tiny_tslma_pad", lambda n: transformer_case(ref, n, dict(tiny, H=6, W=6, Tp=2, Tf=2, TSLMA=True), False, 1, 17)),
        ("ae_tiny_reflect", lambda n: ae_case(ref, n, 1, 48, 32, 1, 2, "reflect", "Tanh", 21)),
        ("ae_tiny_zero", lambda n: ae_case(ref, n, 3, 48, 32, 1, 2, "zero", "Sigmoid", 22)),
        ("losses_tiny", lambda n: losses_case(ref, n, 31)),
        ("step_tiny", lambda n: step_case(ref, n, dict(tiny, Tp=2, Tf=2), 48, 64, 2, 41)),
        ("step_k64_digest", lambda n: step_case(ref, n, k64, 528, 64, 1, 101, steps=2, sample=1024)),
        ("step_nar_gan_tiny", lambda n: nar_gan_step_case(ref, n, dict(tiny, Tp=2, Tf=2), 48, 64, 2, 91)),
        ("step_far_tiny", lambda n: far_step_case(ref, n, far_tiny, 48, 64, 2, 61)),
        ("step_ae_tiny", lambda n: ae_step_case(ref, n, 1, 48, 32, 2, 2, 81)),
        ("metrics_tiny", lambda n: metrics_case(ref, n)),
        ("nar_k64_digest", lambda n: transformer_case(ref, n, k64, False, 1, 51, full=False, check64=False)),
        # batch 4 = 2560 tokens: > 256-tile GEMM grids (the two-stage nt instantiations the batch-16 bench step runs), 4-sample BatchNorm statistics
        ("nar_k64_digest_n4", lambda n: transformer_case(ref, n, k64, False, 4, 55, full=False, check64=False)),
        ("step_k64_n4_digest", lambda n: step_case(ref, n, k64, 528, 64, 4, 102, steps=2, sample=1024)),
        ("nar_kth128_digest", lambda n: transformer_case(ref, n, dict(k64, Tf=40, H=16, W=16, window_size=8), False, 1, 53, full=False,
                                                          check64=False)),
        ("far_bair_digest", lambda n: transformer_case(ref, n, far, True, 1, 52, full=False, check64=False)),
        # BASELINE config 4 at its literal size: VPTRFormerFAR(2, 28, ...), T_in = 29 (train_FAR_mp.py:293-300)
        ("far_bair29_digest", lambda n: transformer_case(ref, n, dict(far, Tf=28, Tin=29), True, 1, 54, full=False, check64=False)),
        # full-size auto-encoders: BAIR (3 channels, zero padding, 64x64) and KTH 128x128 (1 channel, reflect)
        ("ae_bair528_digest", lambda n: ae_digest_case(ref, n, 3, 528, 64, 1, 2, "zero", "Tanh", 23)),
        ("ae_kth128_digest", lambda n: ae_digest_case(ref, n, 1, 528, 128, 1, 2, "reflect", "Tanh", 24)),
        ("rollouts_tiny", lambda n: rollout_case(ref, n, 111)),
        # the bench workload at the bench's per-GPU batch: 16 clips = 10 240 tokens (the 240-tile and 960-tile GEMM grids, 160-frame statistics)
        ("step_k64_n16_digest", lambda n: step_case(ref, n, k64, 528, 64, 16, 106, steps=2, sample=1024)),
        # ---- round 4: reference-recorded 2-step TRAIN-STEP records at the literal size of every BASELINE.json config -------------
        # config 1: stage-1 auto-encoder + PatchGAN on MovingMNIST, feat 528, batch 4 x (10 + 10) frames, Sigmoid output, raw inputs
        ("step_ae528_mnist_digest", lambda n: ae_step_case(ref, n, 1, 528, 64, 4, 10, 83, out_layer="Sigmoid", norm="raw")),
        # config 2: MovingMNIST NAR 10 -> 10 (4 + 8 layers), Sigmoid decoder on un-normalised [0, 1) frames
        ("step_mnist_digest", lambda n: step_case(ref, n, k64, 528, 64, 2, 103, steps=2, sample=1024, out_layer="Sigmoid", norm="raw")),
        # config 4: BAIR FAR 2 -> 28 (T_in = 29, 12 layers, RPE), 3-channel frames, zero padding, Tanh, BAIR normalisation
        ("step_bair29_digest", lambda n: far_step_case(ref, n, dict(far, Tf=28, Tin=29), 528, 64, 1, 104, steps=2, cimg=3,
                                                        padding_type="zero", out_layer="Tanh", norm="bair", sample=1024)),
        # config 5: KTH 128 x 128 10 -> 40, 16 x 16 feature maps, 8 x 8 windows (152.6 M parameters)
        ("step_kth128_digest", lambda n: step_case(ref, n, dict(k64, Tf=40, H=16, W=16, window_size=8), 528, 128, 1, 105, steps=2,
                                                    sample=1024)),
        # ---- round 5: configs 4 and 5 at batch sizes that run the MULTI-ROUND GEMM grids the bench times (> 256 tiles on a 528-wide
        # output needs > 10 880 tokens): BAIR T = 29 at N = 6 (11 136 tokens), KTH128 at the bench's own per-GPU batch 2 (20 480 tokens)
        ("far_bair29_digest_n6", lambda n: transformer_case(ref, n, dict(far, Tf=28, Tin=29), True, 6, 56, full=False, check64=False)),
        ("nar_kth128_digest_n2", lambda n: transformer_case(ref, n, dict(k64, Tf=40, H=16, W=16, window_size=8), False, 2, 57, full=False,
                                                             check64=False)),
        ("step_bair29_n6_digest", lambda n: far_step_case(ref, n, dict(far, Tf=28, Tin=29), 528, 64, 6, 107, steps=2, cimg=3,
                                                           padding_type="zero", out_layer="Tanh", norm="bair", sample=1024)),
        ("step_kth128_n2_digest", lambda n: step_case(ref, n, dict(k64, Tf=40, H=16, W=16, window_size=8), 528, 128, 2, 108, steps=2,
                                                       sample=1024)),
        # a checkpoint the reference itself wrote (the checkpoint-interchange test reads it instead of importing the reference)
        ("ckpt_ref_nar24", lambda n: ckpt_case(ref, n, 5)),
    ]
    only = sys.argv[1:]
    for name, fn in cases:
        if not only or name in only:
            fn(name)
    print("golden fixtures written to", GOLD, "(" + (", ".join(only) if only else "all") + ")")


if __name__ == "__main__":
    main()
