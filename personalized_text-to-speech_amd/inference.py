"""Graph-captured inference: `Synthesizer(net_g)` serves SynthesizerTrn.infer() from captured hipGraphs.

A call is two graphs with one small readback between them (the predicted lengths size the frame axis, which a graph cannot do):

    P  text encoder, speaker embedding, duration predictor (reverse), durations and lengths     key (b, padded t_x, forced)
       -> the host reads y_lengths (b int32 values: the call's only device-to-host copy) and picks the frame capacity t_cap
    S  prior expansion (csrc/expand.hip), reverse flow, decoder at t_cap frames                  key (P key, t_cap, decoder frames)

Every key runs eagerly the first time it is seen (its warm-up: the workspaces reach their size), is captured the second time and
replayed from then on.  All graphs share one memory pool and one non-default capture stream, and record one stream (no side
branches).  The scalars live in a device buffer read by the kernels, so one graph serves every noise_scale / length_scale /
noise_scale_w; the noise is drawn inside the graphs from torch's graph-safe generator, with the shapes and dtypes infer() draws
at the same shapes.  Weight preparation (weight_arena) is part of every graph: in-place parameter updates reach replays.
"""
import collections

import torch

from . import kernels as K


def padded_tokens(t_x, steps):
    """Token axis of a call: the first of `steps` that holds t_x, beyond the largest a multiple of it."""
    for s in steps:
        if s >= t_x:
            return s
    top = steps[-1]
    return -(-t_x // top) * top


def frame_capacity(y_max, frame_step, max_len=None):
    """(flow frames, decoder frames) for a call whose longest predicted utterance has y_max frames.  The flow runs at the next
    multiple of frame_step, cut back towards max_len but never below y_max (frames past max_len still feed the flow's
    convolutions in infer()); the decoder sees at most max_len frames, as infer()'s `[:, :, :max_len]` does."""
    t_cap = -(-y_max // frame_step) * frame_step
    if max_len is not None and max_len < t_cap:
        t_cap = max(y_max, max_len)
    t_dec = t_cap if max_len is None else min(t_cap, max_len)
    return t_cap, t_dec


class GraphCache:
    """Keys -> entries with least-recently-used eviction and the session's counters (host logic only).  An entry is seen once
    (eager warm-up) before it is captured; `children` of a key are evicted with it (an S graph reads its P graph's outputs)."""

    def __init__(self, max_graphs):
        if max_graphs < 2:
            raise ValueError("max_graphs must be at least 2 (one P and one S graph)")
        self.max_graphs = max_graphs
        self.entries = collections.OrderedDict()
        self.stats = dict(calls=0, graphs=0, hits=0, captures=0, warmups=0, evictions=0, fallbacks=0)

    def lookup(self, key, parent=None):
        """-> (entry, action), action 'eager' (first sight), 'capture' (second) or 'replay'."""
        ent = self.entries.get(key)
        if ent is None:
            ent = self.entries[key] = dict(key=key, parent=parent, graph=None)
            self.stats["warmups"] += 1
            return ent, "eager"
        self.entries.move_to_end(key)
        if parent is not None:
            self.entries.move_to_end(parent)
        if ent["graph"] is None:
            return ent, "capture"
        self.stats["hits"] += 1
        return ent, "replay"

    def captured(self, ent, graph):
        ent["graph"] = graph
        self.stats["captures"] += 1
        self.stats["graphs"] += 1
        self._evict(keep=(ent["key"], ent["parent"]))

    def _drop(self, key):
        ent = self.entries.pop(key, None)
        if ent is None:
            return
        if ent["graph"] is not None:
            self.stats["graphs"] -= 1
            self.stats["evictions"] += 1
        for k in [k for k, e in self.entries.items() if e["parent"] == key]:
            self._drop(k)

    def _evict(self, keep):
        while self.stats["graphs"] > self.max_graphs:
            victim = next((k for k, e in self.entries.items() if e["graph"] is not None and k not in keep), None)
            if victim is None:
                return
            self._drop(victim)


class Synthesizer:
    """Captured-graph inference session over an eval-mode SynthesizerTrn.

        synth = Synthesizer(net_g, amp=True)
        audio, sample_lengths, durations = synth(x, x_lengths, sid, noise_scale=.667, length_scale=1.0, noise_scale_w=.8)

    audio [b, 1, t_dec * hop] (device; item i is valid up to sample_lengths[i]), sample_lengths [b] int64 (host: the lengths
    were read anyway), durations [b, t_x] int32 frames per token (device).  Calls whose longest utterance exceeds max_frames run
    eagerly through infer() (counted in stats["fallbacks"]) and return the same triple."""

    def __init__(self, net_g, amp=True, t_x_steps=(32, 64, 128, 256, 512), frame_step=64, max_frames=4096, max_graphs=32):
        if net_g.training:
            raise RuntimeError("Synthesizer needs the generator in eval mode (net_g.eval()): dropout would be captured")
        self.net, self.amp = net_g, amp
        self.t_x_steps, self.frame_step, self.max_frames = sorted(t_x_steps), int(frame_step), int(max_frames)
        self.device = next(net_g.parameters()).device
        self.hop = 1
        for r in net_g.upsample_rates:
            self.hop *= r
        self.cache = GraphCache(max_graphs)
        self.stats = self.cache.stats
        self._pool = None
        self._stream = torch.cuda.Stream(self.device)

    # -- the two stages, on the capture stream --------------------------------------------------------------------------------

    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.amp)

    def _run(self, ent, action, fn):
        """Run fn() eagerly, or capture it into ent's graph and replay it; returns fn's outputs (static ones once captured)."""
        cs, cur = self._stream, torch.cuda.current_stream(self.device)
        if action == "replay":
            cs.wait_stream(cur)
            with torch.cuda.stream(cs):
                ent["graph"].replay()
            cur.wait_stream(cs)
            return ent["out"]
        if action == "eager":
            cs.wait_stream(cur)
            with torch.cuda.stream(cs):
                out = fn()
            cur.wait_stream(cs)
            return out
        from . import _lib
        timer_was, _lib.timer.enabled = _lib.timer.enabled, False
        K.note_graph_captured()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g, pool=self._pool, stream=cs):
            ent["out"] = fn()
        _lib.timer.enabled = timer_was
        if self._pool is None:
            self._pool = g.pool()
        ent["arenas"] = dict(self.net.__dict__.get("_weight_arenas", {}))     # what the graph's weight preparation writes
        self.cache.captured(ent, g)
        return self._run(ent, "replay", fn)

    def _inputs(self, key, x, x_lengths, sid, durations):
        """Static input buffers of a P key (kept in its cache entry)."""
        b, t_x = key[1], key[2]
        ent = self.cache.entries[key]
        if "in" not in ent:
            dev = self.device
            ent["in"] = dict(x=torch.zeros(b, t_x, dtype=torch.long, device=dev),
                             x_lengths=torch.zeros(b, dtype=torch.long, device=dev),
                             sid=torch.zeros(b, dtype=torch.long, device=dev) if sid is not None else None,
                             scalars=torch.zeros(3, dtype=torch.float32, device=dev),
                             durations=torch.zeros(b, 1, t_x, dtype=torch.float32, device=dev) if durations is not None else None)
        st = ent["in"]
        n = x.size(1)
        st["x"][:, :n].copy_(x, non_blocking=True)
        if n < t_x:
            st["x"][:, n:].zero_()
        st["x_lengths"].copy_(x_lengths, non_blocking=True)
        if sid is not None:
            st["sid"].copy_(sid, non_blocking=True)
        if durations is not None:
            st["durations"][..., :n].copy_(durations.reshape(b, 1, n), non_blocking=True)
            if n < t_x:
                st["durations"][..., n:].zero_()
        return st

    def __call__(self, x, x_lengths, sid=None, noise_scale=.667, length_scale=1.0, noise_scale_w=.8, durations=None, max_len=None):
        net = self.net
        if net.training:
            raise RuntimeError("Synthesizer: the generator was switched to train mode after the session was created")
        self.stats["calls"] += 1
        b, n = x.size(0), x.size(1)
        x, x_lengths = x.to(self.device), x_lengths.to(self.device)
        sid = sid.to(self.device) if sid is not None else None
        durations = durations.to(self.device) if durations is not None else None
        pkey = ("P", b, padded_tokens(n, self.t_x_steps), durations is not None, sid is not None)
        pent, paction = self.cache.lookup(pkey)
        st = self._inputs(pkey, x, x_lengths, sid, durations)
        sc = st["scalars"]
        for i, v in enumerate((length_scale, noise_scale, noise_scale_w)):
            sc[i].fill_(float(v))

        def stage_p():
            with torch.no_grad(), self._autocast(), net._scope():
                return net._infer_prior(st["x"], st["x_lengths"], st["sid"], sc, st["durations"])

        with torch.no_grad():
            m_p, logs_p, d, g, y_lengths, w_ceil = self._run(pent, paction, stage_p)
            y_host = y_lengths.to("cpu")                         # the one readback of a call
            y_max = int(y_host.max())
            if self.needs_fallback(y_max, self.max_frames):
                self.stats["fallbacks"] += 1
                return self._eager(x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, durations, max_len)
            t_cap, t_dec = frame_capacity(y_max, self.frame_step, max_len)
            skey = ("S", pkey, t_cap, t_dec)
            sent, saction = self.cache.lookup(skey, parent=pkey)
            if paction == "eager" and saction == "capture":
                saction = "eager"                                # P's outputs are not yet the static ones S must be captured on
            forced = durations is not None

            def stage_s():
                with self._autocast(), net._scope():
                    o, _ = net._infer_synth(m_p, logs_p, d, st["x_lengths"], g, sc, t_cap, max_len=t_dec, forced=forced)
                    return o

            o = self._run(sent, saction, stage_s)
            audio = o.clone()
            dur = w_ceil[:, :n].clone()
        lengths = torch.clamp(y_host.long(), max=t_dec) * self.hop
        return audio, lengths, dur

    @staticmethod
    def needs_fallback(y_max, max_frames):
        return y_max > max_frames

    def _eager(self, x, x_lengths, sid, noise_scale, length_scale, noise_scale_w, durations, max_len):
        """infer() itself (the fallback for utterances longer than max_frames)."""
        net = self.net
        with torch.no_grad(), self._autocast():
            o, attn, y_mask, _ = net.infer(x, x_lengths, sid, noise_scale=noise_scale, length_scale=length_scale,
                                           noise_scale_w=noise_scale_w, max_len=max_len, durations=durations)
        w_ceil = attn.sum(2)[:, 0].round().to(torch.int32)
        lengths = y_mask[:, 0].sum(-1).long().cpu()
        if max_len is not None:
            lengths = torch.clamp(lengths, max=max_len)
        return o, lengths * self.hop, w_ceil
