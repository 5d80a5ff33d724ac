"""What KV-cached FAR decoding rests on, checked without a GPU: the prefix property of the causal model on the oracle in fp64, and the
declaration of the step kernel's entry point."""
import os
import re

import torch

from helpers import build_transformer
from oracle import fill
from oracle import vptr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_far_prefix_property_fp64():
    """In eval mode every sub-layer of a FAR block but the causal temporal attention is frame-local, so the outputs of frames < t do
    not depend on later frames: far_forward(x[:, :t]) == far_forward(x)[:, :t].  `forward_cached` reproduces the full pass because of
    exactly this."""
    import vptr_amd.model as pkg
    cfg = dict(Tp=3, Tf=3, H=8, W=8, C=48, nhead=8, window_size=4, num_encoder_layers=2, rpe=True)
    m = build_transformer(pkg, cfg, True)
    fill.apply_fill(m, 730)
    P = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in m.state_dict().items()}
    x = fill.rand_normal((2, 6, 48, 8, 8), 731).abs().double()
    full = O.far_forward(P, x, cfg)
    assert full.dtype == torch.float64
    for t in range(1, 7):
        part = O.far_forward(P, x[:, :t], cfg)
        d = float((part - full[:, :t]).norm() / full[:, :t].norm())
        assert d <= 1e-12, (t, d)
    # and the property is not vacuous: a later frame does change with an earlier one
    y = x.clone()
    y[:, 0] = x[:, 1]
    assert float((O.far_forward(P, y, cfg)[:, -1] - full[:, -1]).norm() / full[:, -1].norm()) > 1e-6


def test_tattn_step_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vptr_hip.h")).read()
    assert re.search(r"\bint\s+vptr_tattn_step\s*\(", hdr)
    assert "TIME-MAJOR" in hdr[hdr.index("vptr_tattn_step") - 1500:hdr.index("vptr_tattn_step")]      # the layout comment
    from vptr_amd import _lib
    assert "vptr_tattn_step" in _lib.SIGNATURES and len(_lib.SIGNATURES["vptr_tattn_step"]) == 11
    assert "vptr_tattn_step" in _lib.EXPORTS


def test_cached_rollout_keyword_default_is_off():
    import inspect
    from vptr_amd.inference import far_rollout
    assert inspect.signature(far_rollout).parameters["kv_cache"].default is False
