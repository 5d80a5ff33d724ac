"""The trainers with `gan_loss="fused"` (ops.gan_loss_pair / ops.gan_loss, csrc/gan_loss.hip) on the tiny configurations of
tests/validation_cases.py:
  * AETrainer against the reference's records of step_ae_tiny and NARTrainer(disc=) against those of step_nar_gan_tiny, both at the bar
    of tests/test_02_model_gpu.py's stage-1 test, 2 * TOL * |v| + 1e-6;
  * FARTrainer(disc=), whose fixture has no adversarial branch and so no records, against a `gan_loss="torch"` twin at the same bar;
  * `eval_step` of all three against a `gan_loss="torch"` twin (see `_eval_bounds`);
  * a captured NAR + GAN step: strictly fewer kernel nodes with the fused setting; both censuses are printed (profiles/gan_loss.md)."""
import pytest
import torch

import validation_cases as V
from helpers import jload, load

pytestmark = pytest.mark.gpu

TOL = 1e-3          # the north-star tolerance of tests/test_02_model_gpu.py
GAN_KEYS = ("Dfake", "Dreal", "AEgan", "T_gan")


@pytest.fixture(scope="module")
def pkg():
    import vptr_amd.model as pkg
    return pkg


def _trainer(pkg, c, dev, gan_loss):
    """V.trainer with the gan_loss argument"""
    from vptr_amd.train import AETrainer, FARTrainer, NARTrainer
    enc, dec, T, disc = V.modules(pkg, c)
    kind, meta = c["kind"], c["meta"]
    if kind == "ae":
        return AETrainer(enc.to(dev), dec.to(dev), disc.to(dev), lr=2e-4, lam_gan=c["lam_gan"], gan_loss=gan_loss)
    if kind.startswith("nar"):
        return NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=meta["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, disc=disc.to(dev),
                          lam_gan=c["lam_gan"], gan_loss=gan_loss)
    return FARTrainer(enc.to(dev), dec.to(dev), T.to(dev), lr=1e-4, max_grad_norm=1.0, disc=disc.to(dev), lam_gan=c["lam_gan"], gan_loss=gan_loss)


def _batch(c, s, dev):
    past, fut = V.batch(c, s)
    return past.to(dev), fut.to(dev)


def _steps(pkg, c, dev, gan_loss, n):
    from vptr_amd import ops
    ops.unregister_flat_slabs()
    tr = _trainer(pkg, c, dev, gan_loss)
    assert tr.gan_fused == (gan_loss == "fused")
    return [{k: float(v) for k, v in tr.step(*_batch(c, s, dev)).items()} for s in range(n)]


@pytest.mark.parametrize("kind,fixture", [("ae", "step_ae_tiny"), ("nar_gan", "step_nar_gan_tiny")])
def test_fused_steps_match_the_reference_records(pkg, dev, kind, fixture):
    c = V.case(kind)
    records = jload(load(fixture), "records")
    outs = _steps(pkg, c, dev, "fused", len(records))
    for s, (out, ref) in enumerate(zip(outs, records)):
        for k, v in ref.items():
            print("%s step %d %-9s got % .9e  reference % .9e  |diff| / bound %.4f" % (kind, s, k, out[k], v, abs(out[k] - v) / (2 * TOL * abs(v) + 1e-6)))
            assert abs(out[k] - v) < 2 * TOL * abs(v) + 1e-6, (kind, s, k, out[k], v)


def test_fused_far_gan_steps_match_the_torch_twin(pkg, dev):
    c = V.case("far_gan")
    torch_outs = _steps(pkg, c, dev, "torch", 2)
    fused_outs = _steps(pkg, c, dev, "fused", 2)
    for s, (a, b) in enumerate(zip(fused_outs, torch_outs)):
        assert set(a) == set(b) and {"T_gan", "Dtotal", "Dfake", "Dreal"} <= set(a)
        for k, v in b.items():
            print("far_gan step %d %-9s fused % .9e  torch % .9e  |diff| / bound %.4f" % (s, k, a[k], v, abs(a[k] - v) / (2 * TOL * abs(v) + 1e-6)))
            assert abs(a[k] - v) < 2 * TOL * abs(v) + 1e-6, (s, k, a[k], v)


def _eval_bounds(terms, lam, max_logit):
    """|fused - torch| per term of one eval pass of twins that hold the same state, in deterministic mode.  The two passes issue the same
    forward launches on the same bits, so the logits are the same and every term the adversarial loss does not enter is EQUAL.  A GAN
    term is the mean of a vanilla loss over the same logits, evaluated twice in fp32: each evaluation is within the forward bar of
    tests/gan_loss_cases.py, 1e-6 * mean(|x| (1 + |t|) + 1) <= B = 1e-6 * (2 max|x| + 1), of the exact mean, so the two differ by at most
    2 B.  Dtotal = 0.5 lam (Dfake + Dreal): lam * 2 B and two roundings of the result; the total adds lam * T_gan to the other terms:
    lam * 2 B and three roundings."""
    B = 1e-6 * (2.0 * max_logit + 1.0)
    out = {}
    for k, v in terms.items():
        if k in GAN_KEYS:
            out[k] = 2.0 * B
        elif k == "Dtotal":
            out[k] = lam * 2.0 * B + 2.0 ** -23 * abs(v)
        elif k in ("AE_total", "T_total"):
            out[k] = lam * 2.0 * B + 1.5 * 2.0 ** -23 * abs(v)
        else:
            out[k] = 0.0
    return out


@pytest.mark.parametrize("kind", ["ae", "nar_gan", "far_gan"])
def test_fused_eval_step_matches_the_torch_twin(pkg, dev, kind):
    from vptr_amd import ops
    c = V.case(kind)
    past, fut = _batch(c, 0, dev)
    ops.set_deterministic(True)
    try:
        runs, logit = {}, [0.0]
        for gan_loss in ("torch", "fused"):
            ops.unregister_flat_slabs()
            tr = _trainer(pkg, c, dev, gan_loss)
            hook = tr.disc.register_forward_hook(lambda m, i, o: logit.__setitem__(0, max(logit[0], float(o.detach().abs().max()))))
            out = tr.eval_step(past, fut)
            hook.remove()
            assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and not v.requires_grad for v in out.values())
            runs[gan_loss] = {k: float(v) for k, v in out.items()}
            del tr
    finally:
        ops.set_deterministic(False)
    assert set(runs["torch"]) == set(runs["fused"]) and logit[0] > 0.0
    bounds = _eval_bounds(runs["torch"], c["lam_gan"], logit[0])
    for k, v in runs["torch"].items():
        d = abs(runs["fused"][k] - v)
        print("eval[%s] %-9s fused % .9e  torch % .9e  |diff| %.3e  bound %.3e" % (kind, k, runs["fused"][k], v, d, bounds[k]))
        assert d <= bounds[k], (kind, k, runs["fused"][k], v, bounds[k])


def test_captured_nar_gan_step_has_fewer_kernel_nodes_when_fused(pkg, dev):
    from vptr_amd import ops
    c = V.case("nar_gan")
    past, fut = _batch(c, 0, dev)
    census = {}
    for gan_loss in ("torch", "fused"):
        ops.unregister_flat_slabs()
        tr = _trainer(pkg, c, dev, gan_loss)
        tr.capture(past, fut, warmup=2)
        census[gan_loss] = dict(tr.graph_nodes)
        out = tr.step(past, fut)
        assert all(torch.isfinite(v).all() for v in out.values())
        del tr
    print("captured NAR + GAN step, node census: torch %s  fused %s" % (census["torch"], census["fused"]))
    assert set(census["fused"]) <= {"kernel", "memcpy", "empty"}
    assert census["fused"]["kernel"] < census["torch"]["kernel"], census
