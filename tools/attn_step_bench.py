"""Micro-benchmark of vptr_tattn_step (one KV-cached decoding step of the causal temporal attention) at the FAR models' geometries
(GPU box).  The kernel streams the cache: 2 * Tk * rows * C * 4 bytes per call.  Twelve caches are visited in turn, as the 12 layers of
the model do, so that a call never finds its slabs in the last-level cache from the call before."""
import os, sys
import torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from vptr_amd._lib import lib, ptr, stream, check

dev = torch.device("cuda:0")
C, nh, L = 528, 8, 12


def timed(fn, n):
    for i in range(L):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for name, N, Tcap, Tks in (("BAIR 2->28 batch 16", 16, 30, (2, 10, 20, 29)), ("10->10 batch 8", 8, 20, (10, 19))):
    rows = N * 64
    q = torch.randn(rows, C, device=dev)
    o = torch.empty(rows, C, device=dev)
    ks = [torch.randn(Tcap, rows, C, device=dev) for _ in range(L)]
    vs = [torch.randn(Tcap, rows, C, device=dev) for _ in range(L)]
    for Tk in Tks:
        us = timed(lambda i: check(lib.vptr_tattn_step(ptr(q), ptr(ks[i % L]), ptr(vs[i % L]), ptr(o), rows, Tk, Tcap, C, nh, 1, stream()),
                                   "vptr_tattn_step"), 10 * L)
        mb = 2.0 * Tk * rows * C * 4 / 1e6
        print("%-20s rows %5d Tk %2d: %7.1f us  %7.1f MB  %6.2f TB/s" % (name, rows, Tk, us, mb, mb / us))
    del ks, vs
