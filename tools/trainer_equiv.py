#!/usr/bin/env python
"""Do two revisions of vptr_amd/train.py compute the same thing?  Record the trainers' steps at one revision, compare two records.

    VPTR_DETERMINISTIC=1 python tools/trainer_equiv.py --save FILE       (run from the tree under test; needs a GPU)
    python tools/trainer_equiv.py --compare A B                          (host only)

Only the trainers' interface is used (constructors, `step`, `eval_step`, `capture`, `capture_front`, `capture_eval`, `_snapshot`,
`_restore`, `graph_nodes`, `eval_graph_nodes`, `opt`, `opt_D`) and tests/validation_cases.py for the tiny configurations, so one copy
of this file runs against any revision that has them.

--save, per kind (nar, far, nar_gan, far_gan; fixed seeds, the fixtures' models and batches), each sequence twice in the process:
  eager        3 x step, 1 x eval_step, 3 x step
  graph        (nar, far) from the start state: capture(warmup=2), back to the start state, 3 replays
  capture_state  the optimizer state capture's warm-up steps left (their number depends on whether the process has tuned the grouped
               weight-gradient launches before, so the second run of the process need not repeat the first)
  eval_graph   (nar, far) capture_eval, one replay
  front        (nar, in a one-rank gloo group) capture_front(warmup=1), back to the start state, 3 steps
Recorded after every call: each returned term, opt.flat / m / v, opt_D.flat with the adversarial branch; the node censuses; and
whether the two runs of a sequence were bit-identical.

--compare A B: equal censuses; torch.equal on everything of a sequence that was bit-reproducible within A's own run; a sequence that
was not is compared at `verify_graph`'s bounds (terms 5e-3 relative, parameters 3e-4 relative L2) and named as such.  Exit status 1
on any difference."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = ("nar", "far", "nar_gan", "far_gan")
TERM_RTOL, PARAM_RTOL = 5e-3, 3e-4


def _state(tr):
    s = {"flat": tr.opt.flat, "m": tr.opt.m, "v": tr.opt.v}
    if getattr(tr, "disc", None) is not None:
        s["D.flat"] = tr.opt_D.flat
    return {k: v.detach().cpu().clone() for k, v in s.items()}


def _call(rec, name, tr, out=None):
    """append what a call returned and the optimizer state it left"""
    for k, v in (out or {}).items():
        rec["%s/term/%s" % (name, k)] = v.detach().cpu().clone()
    for k, v in _state(tr).items():
        rec["%s/state/%s" % (name, k)] = v


def _run_kind(kind, dev, group):
    """-> ({sequence: {record name: CPU tensor}}, {census name: {node type: count}})"""
    import validation_cases as V
    import vptr_amd.model as pkg
    from vptr_amd import ops
    from vptr_amd.train import NARTrainer

    c = V.case(kind)
    batches = [tuple(t.to(dev) for t in V.batch(c, s)) for s in range(7)]

    def fresh(pg=None):
        ops.unregister_flat_slabs()
        ops.manual_seed(dev, 1234)
        torch.manual_seed(7)
        if pg is None:
            return V.trainer(pkg, c, dev)
        enc, dec, T, _ = V.modules(pkg, c)
        return NARTrainer(enc.to(dev), dec.to(dev), T.to(dev), batch_size=c["meta"]["N"], lr=1e-4, max_grad_norm=1.0, lam_pc=0.1, process_group=pg)

    seqs, census = {}, {}
    tr = fresh()
    start = tr._snapshot()
    rec = seqs["eager"] = {}
    for i in range(7):
        fn = tr.eval_step if i == 3 else tr.step
        _call(rec, "%d_%s" % (i, "eval" if i == 3 else "step"), tr, fn(*batches[i]))
    if kind in ("nar", "far"):
        rec = seqs["graph"] = {}
        tr._restore(start)
        tr.capture(*batches[0], warmup=2)
        census["graph_nodes"] = dict(tr.graph_nodes)
        _call(seqs.setdefault("capture_state", {}), "after_capture", tr)
        tr._restore(start)
        for i in range(3):
            _call(rec, "%d_replay" % i, tr, tr.step(*batches[i]))
        rec = seqs["eval_graph"] = {}
        tr.capture_eval(*batches[3])
        census["eval_graph_nodes"] = dict(tr.eval_graph_nodes)
        _call(rec, "0_replay", tr, tr.eval_step(*batches[3]))
    del tr
    if kind == "nar":
        rec = seqs["front"] = {}
        tr = fresh(group)
        start = tr._snapshot()
        tr.capture_front(*batches[0], warmup=1)
        census["front_nodes"] = dict(tr.graph_nodes)
        tr._restore(start)
        for i in range(3):
            _call(rec, "%d_step" % i, tr, tr.step(*batches[i]))
        del tr
    ops.unregister_flat_slabs()
    torch.cuda.synchronize()
    return seqs, census


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)     # the same records in the same order (a step's terms keep theirs)


def save(path):
    import torch.distributed as dist
    from vptr_amd import ops
    if not ops.config.deterministic:
        raise SystemExit("run with VPTR_DETERMINISTIC=1")
    dev = torch.device("cuda:0")
    import vptr_amd.train
    print("trainers under test: %s" % vptr_amd.train.__file__, flush=True)
    store = tempfile.NamedTemporaryFile(prefix="trainer_equiv_store_", delete=False)
    store.close()
    os.unlink(store.name)     # the file store creates it
    dist.init_process_group("gloo", init_method="file://" + store.name, rank=0, world_size=1)
    out = {}
    try:
        for kind in KINDS:
            first, census = _run_kind(kind, dev, dist.group.WORLD)
            second, census2 = _run_kind(kind, dev, dist.group.WORLD)
            repro = {s: _same(first[s], second[s]) for s in first}
            out[kind] = {"seqs": first, "census": census, "census_repeat_equal": census == census2, "repro": repro}
            print("%-8s census %s  bit-identical when repeated: %s" % (kind, census, repro), flush=True)
    finally:
        dist.destroy_process_group()
        if os.path.exists(store.name):
            os.unlink(store.name)
    torch.save(out, path)
    print("saved", path)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def compare(path_a, path_b):
    A, B = torch.load(path_a), torch.load(path_b)
    bad = 0
    print("A = %s\nB = %s\n" % (path_a, path_b))
    print("| kind | sequence | repeatable within A | records | comparison | result |")
    print("|---|---|---|---|---|---|")
    for kind in KINDS:
        a, b = A[kind], B[kind]
        ok = a["census"] == b["census"]
        bad += not ok
        print("| %s | node censuses | %s | %d | equal dicts: %s | %s |"
              % (kind, a["census_repeat_equal"], len(a["census"]), a["census"], "ok" if ok else "DIFFER: B has %s" % b["census"]))
        for seq, ra in a["seqs"].items():
            rb = b["seqs"].get(seq, {})
            if list(ra) != list(rb):
                bad += 1
                print("| %s | %s | %s | %d | same record names in the same order | DIFFER: %s |"
                      % (kind, seq, a["repro"][seq], len(ra), sorted(set(ra) ^ set(rb)) or "order"))
                continue
            if a["repro"][seq]:
                diff = [k for k in ra if not torch.equal(ra[k], rb[k])]
                bad += bool(diff)
                print("| %s | %s | yes | %d | torch.equal on every record | %s |" % (kind, seq, len(ra), "ok" if not diff else "DIFFER: %s" % diff[:6]))
            else:   # A does not repeat itself bit for bit: the bounds of verify_graph instead
                worst_t = max([_rel(rb[k], ra[k]) for k in ra if "/term/" in k] or [0.0])
                worst_p = max([_rel(rb[k], ra[k]) for k in ra if k.endswith("flat")] or [0.0])
                worst_mv = max([_rel(rb[k], ra[k]) for k in ra if k.endswith("/m") or k.endswith("/v")] or [0.0])
                ok = worst_t <= TERM_RTOL and worst_p <= PARAM_RTOL
                bad += not ok
                print("| %s | %s | NO | %d | bounds: terms %.1e <= %g, parameters %.1e <= %g (moments %.1e, not bounded) | %s%s |"
                      % (kind, seq, len(ra), worst_t, TERM_RTOL, worst_p, PARAM_RTOL, worst_mv, "ok" if ok else "OUT OF BOUNDS",
                         " (and bit-identical)" if _same(ra, rb) else ""))
    print("\n%s" % ("EQUIVALENT" if not bad else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.save:
        save(args.save)
    elif args.compare:
        sys.exit(compare(*args.compare))
    else:
        ap.error("--save FILE or --compare A B")
