"""Test-time rollouts of VPTR on the MI355X path.

The reference defines them in Test_VPTR.ipynb cell 5 and train_FAR.py:103-125; these are the loops behind the "10 -> 40" and
"2 -> 28" settings of BASELINE.json configs 4 / 5:

`nar_rollout(chain="feats")` -- NAR_test_single_iter: round r+1 takes the PREDICTED FEATURES of round r as its past (no
                                Dec -> Enc round trip); needs Tf == Tp from the second round on.
`nar_rollout(chain="frames")`-- every round re-encodes the last Tp predicted frames (the scheme of the BAIR function below for an
                                arbitrary number of rounds).
`nar_bair_2_to_28`           -- NAR_BAIR_2_to_28_test_single_iter: three re-encoded rounds from 2 frames, the third round
                                trimmed by two frames (10 + 10 + 8 = 28 with the released Tf = 10 model).
`far_rollout(mode="RIP")`    -- FAR_RIP_test_single_iter: recurrent inference over PIXELS -- the newest predicted feature is decoded
                                and re-encoded before it joins the input window; once `num_future_frames` predictions have been
                                appended the window slides (its oldest feature is dropped).
`far_rollout(mode="RIL")`    -- FAR_RIL_test_single_iter: the same over the LATENT space (predicted features are appended as-is).
`far_rollout(mode="train")`  -- FAR_show_sample's test phase (train_FAR.py:103-125): growing window, Dec -> Enc from the second
                                prediction on, ONE decoder pass at the end; also returns the re-predicted past frames.

Everything runs under no_grad through the same HIP kernels as training (eval mode: dropout / DropPath off).
`far_rollout(kv_cache=True)` feeds the transformer one new frame per step against cached temporal-attention keys / values
(`VPTRFormerFAR.forward_cached`, the `vptr_tattn_step` kernel) instead of re-running it over the whole window.
`far_rollout(kv_cache=True, graph=True)` / `CachedDecoder` replay ONE captured hipGraph per cached step: the frame index lives in a
device record (include/vptr_hip_decode.h), so the same graph serves every frame of every rollout at a batch size.
"""
import torch

from . import ops


@torch.no_grad()
def nar_rollout(enc, dec, T, past, rounds=1, chain="feats"):
    """past (N,Tp,C,H,W) -> predicted frames (N, rounds*Tf, C, H, W)."""
    if chain not in ("feats", "frames"):
        raise ValueError("nar_rollout: chain must be 'feats' or 'frames'")
    T.eval()
    Tp = past.shape[1]
    out = []
    feats = enc(past)
    for r in range(rounds):
        pred_feats = T(feats)
        pred = dec(pred_feats)
        out.append(pred)
        if r + 1 == rounds:
            break
        if chain == "feats":
            if pred_feats.shape[1] != Tp:
                raise ValueError("nar_rollout(chain='feats'): chained rounds need num_future_frames == num_past_frames "
                                 "(got %d -> %d)" % (Tp, pred_feats.shape[1]))
            feats = pred_feats                      # past_gt_feats = pred_future_feats
        else:
            if pred.shape[1] < Tp:
                raise ValueError("nar_rollout(chain='frames'): a round predicts fewer frames than the model's past length")
            feats = enc(pred[:, -Tp:])
    return torch.cat(out, dim=1)


@torch.no_grad()
def nar_bair_2_to_28(enc, dec, T, past):
    """past (N,2,C,H,W) -> (N, 3*Tf - 2, C, H, W): rounds 2 and 3 start from the last two predicted frames, and the last two
    frames of round 3 are dropped (28 = 10 + 10 + 8 for Tf = 10)."""
    if past.shape[1] != 2:
        raise ValueError("nar_bair_2_to_28: expects two past frames")
    T.eval()
    out = []
    cur = past
    for r in range(3):
        pred = dec(T(enc(cur)))
        out.append(pred if r < 2 else pred[:, :-2])
        cur = pred[:, -2:]
    return torch.cat(out, dim=1)


@torch.no_grad()
def far_rollout(enc, dec, T, past, num_pred, mode="train", kv_cache=False, graph=False):
    """mode 'RIP' / 'RIL': past (N,Tp,C,H,W) -> predicted future frames (N,num_pred,C,H,W).
    mode 'train': -> (pred_past_frames (N,Tp-1,...), pred_future_frames (N,num_pred,...)) exactly as FAR_show_sample's test phase.

    kv_cache=True runs the transformer through `VPTRFormerFAR.forward_cached`: the past features are one prefill pass, every later
    feature is ONE frame against the cached temporal-attention keys / values instead of a pass over the whole window (in eval mode a
    frame's activations depend on earlier frames only, through the causal temporal attention, so the outputs are those of the full
    passes; the two paths run different attention kernels and agree to rounding, not bitwise).  'train': the per-frame outputs are
    collected and decoded once -- the tensor the last full pass returns.  'RIP' / 'RIL': cached while the window only grows; from
    the first step at which the window slides, every position (hence every frame's activations) changes and nothing in the cache is
    reusable, so the rest of the rollout recomputes the slid window as kv_cache=False does.

    graph=True (with kv_cache=True only, else ValueError): the cached steps are replays of one captured hipGraph (`CachedDecoder`, built
    and captured by this call); graph=<a CachedDecoder> reuses one that was built for these modules, this batch size and this mode."""
    if graph is not False and graph is not None:
        if not kv_cache:
            raise ValueError("far_rollout: graph=True replays the KV-cached step; it needs kv_cache=True")
        T.eval()
        d = graph if isinstance(graph, CachedDecoder) else CachedDecoder(enc, dec, T, past.shape[0], mode)
        if (d.enc, d.dec, d.T, d.mode) != (enc, dec, T, mode):
            raise ValueError("far_rollout: the CachedDecoder was built for other modules or another mode")
        return d.rollout(past, num_pred)
    T.eval()
    past_feats = enc(past)
    if kv_cache:
        return _far_rollout_cached(enc, dec, T, past_feats, num_pred, mode)
    pred_feats = T(past_feats)
    if mode == "train":
        input_feats = past_feats
        for i in range(num_pred - 1):
            if i == 0:
                input_feats = torch.cat([past_feats, pred_feats[:, -1:]], dim=1)
            else:
                input_feats = torch.cat([input_feats, enc(dec(pred_feats[:, -1:]))], dim=1)
            pred_feats = T(input_feats)
        frames = dec(pred_feats)
        return frames[:, :-num_pred], frames[:, -num_pred:]
    if mode not in ("RIP", "RIL"):
        raise ValueError("far_rollout: mode must be 'train', 'RIP' or 'RIL'")
    horizon = T.num_future_frames
    frames = [dec(pred_feats[:, -1:])]
    window = past_feats
    newest = pred_feats[:, -1:]                    # the first appended feature is the raw prediction in both modes
    for i in range(1, num_pred):
        window = torch.cat([window, newest], dim=1)
        if i > 1 and i >= horizon:
            window = window[:, 1:]                 # slide: drop the oldest feature once `horizon` predictions were appended
        pred_feats = T(window)
        frame = dec(pred_feats[:, -1:])
        frames.append(frame)
        newest = enc(frame) if mode == "RIP" else pred_feats[:, -1:]
    return torch.cat(frames, dim=1)


def _far_rollout_cached(enc, dec, T, past_feats, num_pred, mode):
    """far_rollout(kv_cache=True) after the encoder pass"""
    if mode not in ("train", "RIP", "RIL"):
        raise ValueError("far_rollout: mode must be 'train', 'RIP' or 'RIL'")
    cache = T.init_cache(past_feats.shape[0], past_feats.device)
    out = T.forward_cached(past_feats, cache)      # prefill: the outputs of all Tp past frames
    newest = out[:, -1:]
    if mode == "train":
        outs = [out]
        for i in range(num_pred - 1):
            newest = T.forward_cached(newest if i == 0 else enc(dec(newest)), cache)
            outs.append(newest)
        frames = dec(torch.cat(outs, dim=1))
        return frames[:, :-num_pred], frames[:, -num_pred:]
    horizon = T.num_future_frames
    frames = [dec(newest)]
    window = past_feats
    slid = False
    for i in range(1, num_pred):
        window = torch.cat([window, newest], dim=1)
        if i > 1 and i >= horizon:
            window = window[:, 1:]
            slid = True                            # the cache is dead from here on: positions shifted under every cached frame
        last = T(window)[:, -1:] if slid else T.forward_cached(newest, cache)
        frame = dec(last)
        frames.append(frame)
        newest = enc(frame) if mode == "RIP" else last
    return torch.cat(frames, dim=1)


def _graph_degrees(g):
    """(nodes, nodes with more than one successor or predecessor) of a torch.cuda.CUDAGraph captured with keep_graph=True"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    graph = ctypes.c_void_p(int(g.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    e = ctypes.c_size_t(0)
    if hip.hipGraphGetEdges(graph, None, None, ctypes.byref(e)) != 0:
        raise RuntimeError("hipGraphGetEdges failed")
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    if e.value and hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(e)) != 0:
        raise RuntimeError("hipGraphGetEdges failed")
    out, inn = {}, {}
    for i in range(e.value):
        out[src[i]] = out.get(src[i], 0) + 1
        inn[dst[i]] = inn.get(dst[i], 0) + 1
    return n.value, sum(1 for v in out.values() if v > 1) + sum(1 for v in inn.values() if v > 1)


class CachedDecoder:
    """KV-cached FAR rollouts at batch size N whose cached steps are replays of ONE captured hipGraph.

    Owns a `FARCache(device_pos=True)` (the frame index is a device record the kernels read by address, so nothing in the step depends
    on a host value), the static feature buffer `x` the step reads and overwrites, and for 'RIP' the static frame buffer.  The graph:
      'RIL'   x <- T.forward_cached(x)                 the features are collected with one eager copy per step, decoded once at the end
      'RIP'   last = T.forward_cached(x); frame <- dec(last); x <- enc(frame)
      'train' x <- T.forward_cached(enc(dec(x)))       from the second step on; the first step takes the raw prediction and runs eagerly
    It is captured on one stream at the first `rollout` (the procedure of the trainers' `_capture`: eager warm-up passes on a side
    stream, reserved staging, the node census -- kernel, memcpy and empty nodes only, a memset node raises) and replayed ever after:
    `captures` counts the captures.  The graph reads the weights by address (the trainers' parameter slab and its P16 images, which the
    eager prefill of every rollout refreshes), so it follows optimizer steps and EMA swaps; the auto-encoder must stay as it was at
    the capture (it is frozen in stage 2).  `rollout` is `far_rollout(kv_cache=True)`'s loop: eager prefill, replays while the window
    grows, today's un-cached recomputation once it slides."""

    MODES = ("train", "RIP", "RIL")

    def __init__(self, enc, dec, T, N, mode, warmup=2):
        if mode not in self.MODES:
            raise ValueError("far_rollout: mode must be 'train', 'RIP' or 'RIL'")
        if T.training or enc.training or dec.training:
            raise ValueError("CachedDecoder: the captured step is eval-only (call .eval() on the encoder, the decoder and the transformer)")
        if isinstance(N, bool) or int(N) < 1:
            raise ValueError("CachedDecoder: N must be a batch size >= 1")
        self.enc, self.dec, self.T, self.N, self.mode, self.warmup = enc, dec, T, int(N), mode, max(int(warmup), 1)
        self.cache = T.init_cache(self.N, device_pos=True)
        tr = T.transformer
        self.x = torch.zeros((self.N, 1, tr.in_C, tr.H, tr.W), device=self.cache.pos.device, dtype=torch.float32)
        self.frame = None
        self.graph, self.graph_nodes, self.graph_branches, self.captures, self.capture_seconds = None, None, None, 0, None
        self._scratch = None

    # -- the step -------------------------------------------------------------------------------------------------------------------
    def _body(self):
        T, x = self.T, self.x
        if self.mode == "RIL":
            x.copy_(T.forward_cached(x, self.cache))
        elif self.mode == "RIP":
            frame = self.dec(T.forward_cached(x, self.cache))
            if self.frame is None:
                self.frame = torch.empty_like(frame)
            self.frame.copy_(frame)
            x.copy_(self.enc(frame))
        else:
            x.copy_(T.forward_cached(self.enc(self.dec(x)), self.cache))

    def _capture(self):
        import time
        from .train import graph_node_census
        t0 = time.perf_counter()
        cache = self.cache
        keep = self.x.clone()

        def warm():
            cache.reset()
            self._body()

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(self.warmup - 1):
                warm()
            ops._upload_stats.update(count=0, max_bytes=0)
            warm()
        torch.cuda.current_stream().wait_stream(s)
        ops.reserve_graph_staging(count=ops._upload_stats["count"] + 4, nbytes=max(1 << 16, 2 * ops._upload_stats["max_bytes"]))
        cache.reset()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            self._body()
        cache.reset()
        self.x.copy_(keep)
        nodes = graph_node_census(g)
        self.graph_nodes = nodes
        bad = {k: v for k, v in nodes.items() if k not in ("kernel", "memcpy", "empty")}
        if bad:
            g.reset()
            raise RuntimeError("captured decoding step holds node types that are not replay-safe on this HIP runtime: %s (all nodes: %s)" % (bad, nodes))
        self.graph_branches = _graph_degrees(g)[1]
        if self.graph_branches:
            g.reset()
            raise RuntimeError("captured decoding step has %d nodes with parallel branches; it must be one chain" % self.graph_branches)
        g.instantiate()
        # shape-keyed scratch of the frozen auto-encoder that the graph reads and writes by address (NARTrainer._module_scratch)
        self._scratch = [getattr(m, a) for mod in (self.enc, self.dec) for m in mod.modules() for a in ("_plane_bufs", "_head_bufs", "_wino_bufs")
                         if getattr(m, a, None) is not None]
        self.graph = g
        self.captures += 1
        torch.cuda.synchronize()
        self.capture_seconds = time.perf_counter() - t0

    def step(self):
        """one cached step on `x` (and `frame`): a replay.  ValueError on the host, before the replay, if it would pass the capacity."""
        cache = self.cache
        if cache.len + 1 > cache.Tcap:
            raise ValueError("forward_cached: %d cached + 1 new frames exceed the cache's %d" % (cache.len, cache.Tcap))
        self.graph.replay()
        cache.len += 1

    # -- the rollout ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def rollout(self, past, num_pred):
        """far_rollout(enc, dec, T, past, num_pred, mode, kv_cache=True) with replayed steps"""
        enc, dec, T, cache, x, mode = self.enc, self.dec, self.T, self.cache, self.x, self.mode
        if past.dim() != 5 or past.shape[0] != self.N:
            raise ValueError("CachedDecoder: built for batches of %d samples, got a past of shape %s" % (self.N, tuple(past.shape)))
        if T.training or enc.training or dec.training:
            raise ValueError("CachedDecoder: the captured step is eval-only")
        if self.graph is None:
            self._capture()
        past_feats = enc(past)
        cache.reset()
        out = T.forward_cached(past_feats, cache)      # prefill (eager); ends with POS = Tp
        x.copy_(out[:, -1:])
        if mode == "train":
            outs = [out]
            for i in range(num_pred - 1):
                if i == 0:
                    x.copy_(T.forward_cached(x, cache))   # the raw prediction: no Dec -> Enc round trip
                else:
                    self.step()
                outs.append(x.clone())
            frames = dec(torch.cat(outs, dim=1))
            return frames[:, :-num_pred], frames[:, -num_pred:]
        horizon = T.num_future_frames
        frames = [dec(x)]
        window = past_feats
        newest = x.clone()
        lasts = []
        slid = False
        for i in range(1, num_pred):
            window = torch.cat([window, newest], dim=1)
            if i > 1 and i >= horizon:
                window = window[:, 1:]
                slid = True
            if slid:
                last = T(window)[:, -1:]
                frame = dec(last)
                frames.append(frame)
                newest = enc(frame) if mode == "RIP" else last
                continue
            self.step()
            newest = x.clone()
            if mode == "RIP":
                frames.append(self.frame.clone())
            else:
                lasts.append(newest)
        if mode == "RIL" and lasts:                    # ONE decoder pass over the replayed steps' features
            n = len(lasts)
            dl = dec(torch.cat(lasts, dim=1))
            frames[1:1] = [dl[:, j:j + 1] for j in range(n)]
        return torch.cat(frames, dim=1)
