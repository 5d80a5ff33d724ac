"""CPU side of the parameter groups of the device-resident optimizer controls: the ABI table of include/vptr_hip_groups.h, the host-side
rejects of its two entry points, every case of tests/param_groups_cases.py against the fp32 CPU emulation of the entry points -- and
against six named mutations of it, each of which must fail the cases listed for it --, the fp64 builder of the cases pinned to
torch.optim.AdamW with param_groups + LambdaLR + clip_grad_norm_, and the host rules: validation of `param_groups=`, `no_decay_groups` on
the tiny NAR and FAR transformers, and `state_dict` into a grouped torch.optim.AdamW and back."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import param_groups_cases as G
import validation_cases as V
from helpers import f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vptr_optim_group_scalars", "vptr_adamw_groups"}


# ---- the ABI table ------------------------------------------------------------------------------------------------------------------
def test_group_signatures_match_header_and_library():
    from vptr_amd import _lib, optim
    text = open(os.path.join(ROOT, "include", "vptr_hip_groups.h")).read()
    assert '#include "vptr_hip_accum.h"' in text
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\bint (vptr_\w+)\s*\(([^;]*)\);", text)}
    assert set(decls) == set(_lib.GROUP_SIGNATURES) == NAMES
    for name, args in decls.items():
        assert len(args.split(",")) == len(_lib.GROUP_SIGNATURES[name]), name             # the stream included
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == _lib.GROUP_SIGNATURES[name] and fn.restype is _lib.c_int
    others = [set(_lib.EXPORTS), set(_lib.EXT_SIGNATURES), set(_lib.OPTIM_SIGNATURES), set(_lib.CONVFFN_SIGNATURES), set(_lib.ACCUM_SIGNATURES),
              set(_lib.LOSS_SIGNATURES), set(_lib.GAN_SIGNATURES)]
    assert all(not NAMES & o for o in others)
    assert len(_lib.EXPORTS) == 77 and _lib.lib.vptr_abi_version() == 10
    from vptr_amd.build import SOURCES
    assert "optim.hip" in SOURCES
    # the table layout: header, host layer and the cases agree
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VPTR_GRP_(\w+) (\d+)", text)}
    assert defs["MAX"] == optim.MAX_GROUPS == G.MAX_GROUPS == 16 and defs["WORDS"] == optim.G_WORDS == G.G_WORDS == 4
    assert {k: defs["H_" + k] for k in G.GH} == G.GH and {k: defs["S_" + k] for k in G.GS} == G.GS
    assert (optim.G_LR_SCALE, optim.G_WEIGHT_DECAY) == (G.GH["LR_SCALE"], G.GH["WEIGHT_DECAY"])
    assert (optim.GS_STEP_SIZE, optim.GS_DECAY, optim.GS_LR) == (G.GS["STEP_SIZE"], G.GS["DECAY"], G.GS["LR"])


def test_entry_points_reject_on_the_host():
    """the argument checks run before any launch, so they can be exercised without a device (the pointers are never dereferenced)"""
    from vptr_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_float * 400)()
    base = (ctypes.addressof(buf) + 63) & ~63
    state, window, ghyper, gstate, slab, ema, gid = base, base + 64, base + 128, base + 384, base + 640, base + 768, base + 896

    def bad(fn, prefix, *args):
        assert fn(*args, None) != 0, (prefix, args)
        assert L.vptr_last_error().decode().startswith(prefix), L.vptr_last_error()

    good = (state, ghyper, gstate, 3)
    for i in range(3):
        bad(L.vptr_optim_group_scalars, "optim_group_scalars", *[None if j == i else a for j, a in enumerate(good)])
        bad(L.vptr_optim_group_scalars, "optim_group_scalars", *[a + 16 if j == i else a for j, a in enumerate(good)])
    for ng in (0, -1, 17):
        bad(L.vptr_optim_group_scalars, "optim_group_scalars", state, ghyper, gstate, ng)
    good = (slab, slab, slab, slab, ema, gid, 4, state, window, gstate, 3)
    for i in (0, 1, 2, 3, 4, 5, 7, 8, 9):                                                 # 4 / 8: ema without window and the reverse
        bad(L.vptr_adamw_groups, "adamw_groups", *[None if j == i else a for j, a in enumerate(good)])
    plain = (slab, slab, slab, slab, None, gid, 4, state, None, gstate, 3)
    for i in (0, 5, 7, 9):
        bad(L.vptr_adamw_groups, "adamw_groups", *[None if j == i else a for j, a in enumerate(plain)])
    for form in (good, plain):
        for n in (0, -5):
            bad(L.vptr_adamw_groups, "adamw_groups", *(form[:6] + (n,) + form[7:]))
        for ng in (0, 17):
            bad(L.vptr_adamw_groups, "adamw_groups", *(form[:10] + (ng,)))
        for i in (7, 8, 9):
            if form[i] is not None:
                bad(L.vptr_adamw_groups, "adamw_groups", *[a + 4 if j == i else a for j, a in enumerate(form)])
    assert all(x == 0.0 for x in buf)


# ---- the cases against the emulation and its mutations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    return G.GroupEmu()


@pytest.mark.parametrize("case", G.all_cases(), ids=G.case_id)
def test_case_passes_on_the_emulation(be, case):
    getattr(G, case[0])(be, *case[1])


def test_mutation_lists_name_real_cases():
    known = set(G.all_cases())
    assert len(G.MUTATIONS) == 6
    for name, cases in G.MUTATIONS.items():
        assert cases and set(cases) <= known, name


@pytest.mark.parametrize("mutation,case", [(m, c) for m in sorted(G.MUTATIONS) for c in G.MUTATIONS[m]], ids=lambda x: x if isinstance(x, str) else G.case_id(x))
def test_case_fails_on_the_mutated_emulation(mutation, case):
    with pytest.raises(AssertionError):
        getattr(G, case[0])(G.GroupEmu(mutation), *case[1])


# ---- the fp64 builder is torch.optim.AdamW ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.REF_STEPS)
def test_fp64_builder_is_torch_adamw_with_param_groups(k):
    """groups_ref64 against torch.optim.AdamW on fp64 parameters, one param_groups entry per group (lr = base * lr_scale, its own
    weight_decay), LambdaLR with the schedule's factor, clip_grad_norm_ over all parameters, resumed from the state k - 1 steps leave"""
    state4, sumsq, max_norm, gid, sched, want, _, _ = G.ref_case(k)
    p, g, m, v = state4
    base = f32(G.BASE_LR)
    pars, groups = [], []
    for grp, (scale, wd) in enumerate(G.REF_SPECS):
        sel = gid == grp
        par = torch.nn.Parameter(p[sel].double().clone())
        par.grad = g[sel].double().clone()
        pars.append((par, sel))
        groups.append({"params": [par], "lr": base * f32(scale), "weight_decay": f32(wd)})
    opt = torch.optim.AdamW(groups, lr=base, betas=(f32(G.HYPER["b1"]), f32(G.HYPER["b2"])), eps=f32(G.HYPER["eps"]))
    for par, sel in pars:
        opt.state[par] = {"step": torch.tensor(float(k - 1)), "exp_avg": m[sel].double().clone(), "exp_avg_sq": v[sel].double().clone()}
    lam = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: sched.factor(e + k - 1))      # epoch 0 is the update after k - 1 applied ones
    total = torch.nn.utils.clip_grad_norm_([par for par, _ in pars], f32(max_norm))
    assert abs(float(total) - sumsq ** 0.5) <= 1e-6 * sumsq ** 0.5                       # fp32(sumsq) against the fp64 norm
    # clip_grad_norm_ used the fp64 norm; the builder the fp32 word of the sum of squares, as the device does: put its coefficient in
    coef64 = min(1.0, f32(max_norm) / (float(total) + 1e-6))
    coefab = min(1.0, f32(max_norm) / (float(sumsq) ** 0.5 + 1e-6))
    for par, _ in pars:
        par.grad.mul_(coefab / coef64)
    opt.step()
    lam.step()
    for name, i in (("p", 0), ("m", 1), ("v", 2)):
        got = torch.zeros(G.REF_N, dtype=torch.float64)
        for par, sel in pars:
            st = opt.state[par]
            got[sel] = (par.detach(), st["exp_avg"], st["exp_avg_sq"])[i]
        err = float((got - want[i]).norm() / want[i].norm())
        assert err <= 1e-12, (k, name, err)


# ---- host rules --------------------------------------------------------------------------------------------------------------------------
def _params():
    return [torch.nn.Parameter(torch.randn(s)) for s in ((5,), (3, 2, 2), (7,), (2, 3, 1))]


def test_resolve_param_groups_rules():
    from vptr_amd.optim import resolve_param_groups as R
    ps = _params()
    assert R(ps, []) == ([0, 0, 0, 0], [(1.0, None)])
    assert R(ps, [{"params": [ps[2]], "lr_scale": 0.5}]) == ([0, 0, 1, 0], [(1.0, None), (0.5, None)])          # the unlisted ones: group 0
    assert R(ps, [{"params": [ps[1], ps[3]], "weight_decay": 0.0}, {"params": [ps[0], ps[2]], "lr_scale": 0}]) == ([1, 0, 1, 0], [(1.0, 0.0), (0.0, None)])
    stranger = torch.nn.Parameter(torch.zeros(5))
    for bad in ([{"params": [ps[0]]}, {"params": [ps[0]]}], [{"params": [ps[0], ps[0]]}], [{"params": [stranger]}],
                [{"params": [ps[0]], "lr_scale": -0.1}], [{"params": [ps[0]], "lr_scale": float("nan")}], [{"params": [ps[0]], "lr_scale": float("inf")}],
                [{"params": [ps[0]], "weight_decay": -1.0}], [{"params": [ps[0]], "weight_decay": float("inf")}], [{"params": [ps[0]], "lr": 1e-3}],
                [{"lr_scale": 1.0}], "groups", [[ps[0]]], [{"params": [ps[0]], "lr_scale": "1"}]):
        with pytest.raises(ValueError):
            R(ps, bad)
    many = [torch.nn.Parameter(torch.zeros(1)) for _ in range(17)]
    assert len(R(many, [{"params": [p]} for p in many[:15]])[1]) == 16                      # 15 listed + group 0
    with pytest.raises(ValueError, match="at most 16"):
        R(many, [{"params": [p]} for p in many[:16]])                                       # 16 listed + the unlisted one's group
    assert len(R(many[:16], [{"params": [p]} for p in many[:16]])[1]) == 16                 # all listed: no group 0 in front
    with pytest.raises(ValueError, match="at most 16"):
        R(many, [{"params": [p]} for p in many])


def test_group_map_pads_with_group_0():
    from vptr_amd.optim import group_map
    assert group_map([(0, 5, None), (5, 6, None)], [1, 2], 12).tolist() == [1] * 5 + [2] * 6 + [0]
    assert G.GroupEmu().group_map([(0, 5, None), (5, 6, None)], [1, 2], 12).tolist() == group_map([(0, 5, None), (5, 6, None)], [1, 2], 12).tolist()


@pytest.mark.parametrize("kind", ["nar", "far"])
def test_no_decay_groups_on_the_tiny_models(kind):
    """every trainable parameter lands in exactly one group; norms (the (C, H, W) affines included), biases and the relative-position bias
    tables are the exempt ones, matrices, convolution kernels and the frame queries are decayed"""
    import vptr_amd.model as pkg
    from vptr_amd.optim import no_decay_groups, no_decay_names, resolve_param_groups
    _, _, T, _ = V.modules(pkg, V.case(kind))
    groups = no_decay_groups(T)
    assert len(groups) == 1 and groups[0]["weight_decay"] == 0.0 and "lr_scale" not in groups[0]
    params = [p for p in T.parameters() if p.requires_grad]
    group_of, specs = resolve_param_groups(params, groups)
    assert specs == [(1.0, None), (1.0, 0.0)] and len(group_of) == len(params) and set(group_of) == {0, 1}
    assert len({id(p) for p in groups[0]["params"]}) == len(groups[0]["params"])
    exempt = set(no_decay_names(T))
    by_id = {id(p): n for n, p in T.named_parameters()}
    assert {by_id[id(p)] for p in groups[0]["params"]} == exempt
    norm_params = {id(p) for m in T.modules() if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm2d)) for p in m.parameters(recurse=False)}
    assert norm_params and any(p.dim() == 3 and id(p) in norm_params for p in T.parameters())            # the (C, H, W) affines are among them
    for n, p in T.named_parameters():
        want = id(p) in norm_params or n.endswith("bias") or n.endswith("relative_position_bias_table")
        assert (n in exempt) == want, n
        if p.dim() >= 2 and id(p) not in norm_params and not n.endswith("bias_table"):
            assert n not in exempt, n                                                        # matrices and kernels are decayed
    assert any(n.endswith("weight") and n not in exempt for n in by_id.values())
    if kind == "nar":
        assert "frame_queries" in "".join(by_id.values()) and not any("frame_queries" in n for n in exempt)      # learned queries are decayed


def test_no_decay_groups_exempts_bias_and_position_tables():
    """the tiny fixtures run without relative-position tables: the attention module that owns one, and a module with made-up tables"""
    from vptr_amd.model.vidhrformer import MultiheadAttentionRPE
    from vptr_amd.optim import no_decay_names

    class Odd(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_embed = torch.nn.Parameter(torch.zeros(4, 8))
            self.query_pos = torch.nn.Parameter(torch.zeros(4, 8))
            self.gate_bias = torch.nn.Parameter(torch.zeros(8))
            self.queries = torch.nn.Parameter(torch.zeros(4, 8))
            self.frozen_bias = torch.nn.Parameter(torch.zeros(8), requires_grad=False)
            self.gn = torch.nn.GroupNorm(2, 8)
            self.conv = torch.nn.Conv2d(8, 8, 3)

    assert set(no_decay_names(Odd())) == {"pos_embed", "query_pos", "gate_bias", "gn.weight", "gn.bias", "conv.bias"}
    attn = MultiheadAttentionRPE(16, 2, rpe=True, window_size=4)
    names = set(no_decay_names(attn))
    assert "relative_position_bias_table" in names and not any(n.endswith("weight") for n in names), names


def test_public_arguments():
    from vptr_amd import train
    for cls in (train.FlatAdamW, train.NARTrainer, train.FARTrainer, train.AETrainer):
        assert inspect.signature(cls.__init__).parameters["param_groups"].default is None, cls
    for name in ("set_group", "group_lr"):
        assert callable(getattr(train.FlatAdamW, name))


class _CpuAdamW:
    """FlatAdamW on CPU tensors with parameters that have no GEMM operand form: the host rules of its state_dict need no launch"""

    def __new__(cls, params, **kw):
        from vptr_amd import ops
        from vptr_amd.train import FlatAdamW
        ops.unregister_flat_slabs()
        return FlatAdamW(params, **kw)


def test_state_dict_into_a_grouped_torch_adamw_and_back():
    from vptr_amd.optim import SCALE_KEY, STATE_KEY
    ps = _params()
    mine = [{"params": [ps[2]], "lr_scale": 0.1}, {"params": [ps[3], ps[1]], "weight_decay": 0.0}]
    opt = _CpuAdamW(ps, lr=1e-3, weight_decay=0.01, param_groups=mine)
    assert opt.ctl is not None and opt.groups.ngroups == 3 and opt._order() == [0, 2, 1, 3]
    for slab, seed in ((opt.m, 1), (opt.v, 2)):
        slab.copy_(torch.rand(slab.numel(), generator=torch.Generator().manual_seed(seed)))
    opt.step_dev.fill_(3.0)
    sd = opt.state_dict()
    gs = sd["param_groups"]
    assert [g["params"] for g in gs] == [[0], [1], [2, 3]]                                   # torch's numbering: group after group
    assert [g["lr"] for g in gs] == [1e-3, 1e-3 * 0.1, 1e-3] and [g["weight_decay"] for g in gs] == [0.01, 0.01, 0.0]
    assert [g[SCALE_KEY] for g in gs] == [1.0, 0.1, 1.0] and STATE_KEY in gs[0] and all(STATE_KEY not in g for g in gs[1:])
    assert torch.equal(sd["state"][1]["exp_avg"], opt._logical(opt.m, 2)) and torch.equal(sd["state"][2]["exp_avg"], opt._logical(opt.m, 1))
    # into torch.optim.AdamW built with the same grouping
    tp = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    stock = torch.optim.AdamW([{"params": [tp[0]]}, {"params": [tp[2]], "lr": 1e-4}, {"params": [tp[1], tp[3]], "weight_decay": 0.0}], lr=1e-3, weight_decay=0.01)
    stock.load_state_dict(sd)
    assert torch.equal(stock.state[tp[2]]["exp_avg"], opt._logical(opt.m, 2)) and torch.equal(stock.state[tp[3]]["exp_avg_sq"], opt._logical(opt.v, 3))
    assert [g["lr"] for g in stock.param_groups] == [1e-3, 1e-3 * 0.1, 1e-3]
    # and back, from a torch dict without this project's keys, with other values in it
    back = stock.state_dict()
    for g, lr, wd in zip(back["param_groups"], (2e-3, 5e-4, 0.0), (0.02, 0.02, 0.3)):
        g.pop(SCALE_KEY), g.pop(STATE_KEY, None)
        g["lr"], g["weight_decay"] = lr, wd
    ps2 = _params()
    opt2 = _CpuAdamW(ps2, lr=1e-3, weight_decay=0.01, param_groups=[{"params": [ps2[2]], "lr_scale": 0.1}, {"params": [ps2[3], ps2[1]], "weight_decay": 0.0}])
    opt2.load_state_dict(back)
    assert opt2.lr == 2e-3 and opt2.weight_decay == 0.02 and opt2.groups.lr_scale == [1.0, 0.25, 0.0]
    assert opt2.groups.weight_decay == [None, None, 0.3] and [opt2.groups.decay_of(g) for g in range(3)] == [0.02, 0.02, 0.3]
    n = opt.total                                                                            # the pad elements are no parameter's
    assert torch.equal(opt2.m[:n], opt.m[:n]) and torch.equal(opt2.v[:n], opt.v[:n]) and float(opt2.step_dev) == 3.0
    assert opt2.groups.ghyper[:12].tolist() == [1.0, f32(0.02), 0.0, 0.0, 0.25, f32(0.02), 0.0, 0.0, 0.0, f32(0.3), 0.0, 0.0]
    opt2.set_weight_decay(0.05)                                                              # the inheriting groups follow, the explicit one stays
    assert [opt2.groups.decay_of(g) for g in range(3)] == [0.05, 0.05, 0.3]
    # a multi-group dict into an ungrouped optimizer: equal groups load, different ones raise
    opt3 = _CpuAdamW(_params(), lr=1.0, weight_decay=0.5)
    assert opt3.groups is None and opt3.ctl is None
    with pytest.raises(ValueError, match="param_groups"):
        opt3.load_state_dict(sd)
    # (ids are matched by position, as ever: the dict of an optimizer whose group order is the slab order)
    ps5 = _params()
    opt5 = _CpuAdamW(ps5, param_groups=[{"params": [ps5[0], ps5[1]]}, {"params": [ps5[2], ps5[3]], "lr_scale": 2.0, "weight_decay": 0.3}])
    opt5.step_dev.fill_(3.0)
    same = opt5.state_dict()
    assert len(same["param_groups"]) == 2
    for g in same["param_groups"]:
        g["lr"], g["weight_decay"] = 1e-3, 0.01
    opt3.load_state_dict(same)
    assert opt3.lr == 1e-3 and opt3.weight_decay == 0.01 and float(opt3.step_dev) == 3.0
    # group sizes that do not match
    ps4 = _params()
    opt4 = _CpuAdamW(ps4, param_groups=[{"params": [ps4[0], ps4[1]], "lr_scale": 0.1}, {"params": [ps4[2]], "weight_decay": 0.0}])
    with pytest.raises(ValueError, match="sizes"):
        opt4.load_state_dict(sd)
    # set_group validation
    for bad in (dict(g=3), dict(g=-1), dict(g=True), dict(g=0, lr_scale=-1.0), dict(g=0, weight_decay=float("nan"))):
        with pytest.raises(ValueError):
            opt.set_group(**bad)
    opt.set_group(1, lr_scale=0.0, weight_decay=0.2)
    assert opt.groups.lr_scale[1] == 0.0 and opt.groups.decay_of(1) == 0.2
    with pytest.raises(RuntimeError, match="param_groups"):
        opt3.set_group(0, lr_scale=1.0)
