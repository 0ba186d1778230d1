"""GPU: graph-captured inference (inference.Synthesizer) and its prior-expansion kernel (kernels.expand_prior, csrc/expand.hip).

The kernel against the eager composition it replaces (generate_path + the two one-hot GEMMs + the noise arithmetic), bitwise in
fp32 and under bf16 autocast; the session against SynthesizerTrn.infer() on the tiny fixture model: bitwise where its shapes equal
eager's, to a tolerance where it pads; scalars, shape changes, parameter updates and host syncs across replays."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------------------
# expand_prior == the eager composition

def _eager_expand(pkg, logw, x_lengths, m_p, logs_p, eps, ls, ns, t_cap, durations=None):
    """models.py _infer's expansion at t_y = t_cap (eps [b, c, t_cap])."""
    C = pkg.commons
    t_x = m_p.size(2)
    x_mask = torch.unsqueeze(C.sequence_mask(x_lengths, t_x), 1).to(torch.float32)
    w_ceil = torch.ceil(torch.exp(logw) * x_mask * ls) if durations is None else durations.to(torch.float32) * x_mask
    y_lengths = torch.clamp_min(C.sum12(w_ceil), 1).long()
    y_mask = torch.unsqueeze(C.sequence_mask(y_lengths, t_cap), 1).to(x_mask.dtype)
    attn_mask = torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1)
    attn = C.generate_path(w_ceil, attn_mask)
    m = torch.matmul(attn.squeeze(1), m_p.transpose(1, 2)).transpose(1, 2)
    logs = torch.matmul(attn.squeeze(1), logs_p.transpose(1, 2)).transpose(1, 2)
    z_p = m + eps * torch.exp(logs) * ns
    return z_p, y_mask, y_lengths, w_ceil


def _stats(b, t_x, c, dtype, gen):
    """m_p, logs_p as the text encoder returns them: [b, c, t_x] views of one channels-last [b, t_x, 2c] tensor."""
    st = (torch.randn(b, t_x, 2 * c, generator=gen) * 0.7).to(DEV, dtype)
    stats = st.transpose(1, 2)
    return stats[:, :c], stats[:, c:]


CASES = [  # (t_x, c, x_lengths, logw mode, length_scale, extra frames past the longest item)
    (1, 192, [1, 1], "normal", 1.0, 0),
    (3, 192, [3, 2], "normal", 1.7, 5),
    (50, 192, [50, 31], "zeros", 0.5, 17),        # some durations zero
    (513, 192, [513, 400], "normal", 1.0, 64),
    (1500, 16, [1500, 1499], "normal", 1.0, 3),    # multi-chunk scan, tokens past x_length
    (7, 192, [7, 7], "allzero", 1.0, 4),           # every duration zero: y_len = 1, a frame no token covers
]


@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_expand_prior_equals_eager_composition(pkg, case, amp):
    t_x, c, xl, mode, ls, extra = CASES[case]
    gen = torch.Generator().manual_seed(100 + case)
    b = len(xl)
    x_lengths = torch.tensor(xl, device=DEV)
    logw = (torch.randn(b, 1, t_x, generator=gen) * 0.8 + 0.3)
    if mode == "zeros":
        logw[:, :, ::3] = -200.0                  # exp() underflows to 0: zero frames for these tokens
    if mode == "allzero":
        logw[:] = -200.0
    logw = logw.to(DEV)
    ns = 0.667
    scalars = torch.tensor([ls, ns], dtype=torch.float32, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        m_p, logs_p = _stats(b, t_x, c, torch.bfloat16 if amp else torch.float32, gen)
        _, _, y_len, _ = pkg.kernels.expand_prior(logw, x_lengths, None, None, None, scalars, 0)
        t_cap = int(y_len.max()) + extra
        edt = torch.bfloat16 if amp else torch.float32
        eps = torch.randn(b, t_cap, c, generator=gen).to(DEV, edt).transpose(1, 2)       # [b, c, t_cap], channels-last storage
        ref_z, ref_mask, ref_len, ref_w = _eager_expand(pkg, logw, x_lengths, m_p, logs_p, eps, ls, ns, t_cap)
        z_p, y_mask, y_lengths, w_ceil = pkg.kernels.expand_prior(logw, x_lengths, m_p, logs_p, eps.transpose(1, 2), scalars, t_cap)
    torch.cuda.synchronize()
    assert z_p.dtype == ref_z.dtype and z_p.shape == (b, t_cap, c)
    assert torch.equal(y_lengths.long(), ref_len)
    assert torch.equal(w_ceil, ref_w[:, 0].to(torch.int32))
    assert torch.equal(y_mask, ref_mask)
    ref_z = ref_z.transpose(1, 2)                                        # [b, t_cap, c]
    for i in range(b):
        n = int(ref_len[i])
        assert torch.equal(z_p[i, :n].view(torch.int32), ref_z[i, :n].view(torch.int32)), \
            (i, float((z_p[i, :n].float() - ref_z[i, :n].float()).abs().max()))
        assert not z_p[i, n:].any()
    if mode == "allzero":
        assert ref_len.tolist() == [1] * b


def test_expand_prior_forced_durations(pkg):
    gen = torch.Generator().manual_seed(7)
    b, t_x, c = 3, 40, 192
    x_lengths = torch.tensor([40, 25, 1], device=DEV)
    dur = torch.randint(0, 6, (b, 1, t_x), generator=gen).float().to(DEV)
    scalars = torch.tensor([1.0, 0.5], device=DEV)
    with torch.no_grad():
        m_p, logs_p = _stats(b, t_x, c, torch.float32, gen)
        _, _, y_len, _ = pkg.kernels.expand_prior(None, x_lengths, None, None, None, scalars, 0, durations=dur)
        t_cap = int(y_len.max()) + 9
        eps = torch.randn(b, t_cap, c, generator=gen).to(DEV).transpose(1, 2)
        ref_z, ref_mask, ref_len, ref_w = _eager_expand(pkg, None, x_lengths, m_p, logs_p, eps, 1.0, 0.5, t_cap, durations=dur)
        z_p, y_mask, y_lengths, w_ceil = pkg.kernels.expand_prior(None, x_lengths, m_p, logs_p, eps.transpose(1, 2), scalars, t_cap,
                                                                 durations=dur)
    assert torch.equal(y_lengths.long(), ref_len) and torch.equal(w_ceil, ref_w[:, 0].int()) and torch.equal(y_mask, ref_mask)
    for i in range(b):
        n = int(ref_len[i])
        assert torch.equal(z_p[i, :n], ref_z.transpose(1, 2)[i, :n]) and not z_p[i, n:].any()


# ----------------------------------------------------------------------------------------------------------------------------
# Synthesizer == infer()

def _net(pkg):
    from model_util import build_tiny, load_tiny
    g, cfg = load_tiny()
    net = build_tiny(pkg, g, cfg, DEV)
    t = lambda k: torch.from_numpy(g["in/" + k]).to(DEV)
    return net, t("x"), t("x_lengths"), t("sid"), cfg


def _eager(net, x, xl, sid, amp, seed, **kw):
    torch.manual_seed(seed)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        o, attn, y_mask, _ = net.infer(x, xl, sid, **kw)
    torch.cuda.synchronize()
    return o, attn, y_mask


def _session(pkg, net, x, xl, sid, amp, seed, synth, **kw):
    torch.manual_seed(seed)
    out = synth(x, xl, sid, **kw)
    torch.cuda.synchronize()
    return out


KW = dict(noise_scale=0.667, length_scale=1.0, noise_scale_w=0.8)


@pytest.mark.parametrize("amp", [False, True])
def test_session_equals_infer_at_equal_shapes(pkg, amp):
    net, x, xl, sid, _ = _net(pkg)
    synth = pkg.inference.Synthesizer(net, amp=amp, t_x_steps=(x.size(1),), frame_step=1)
    for i, seed in enumerate((11, 11, 11, 11)):                     # eager warm-up, capture + replay, replays
        o, attn, y_mask = _eager(net, x, xl, sid, amp, seed, **KW)
        audio, lengths, dur = _session(pkg, net, x, xl, sid, amp, seed, synth, **KW)
        assert audio.shape == o.shape, (i, audio.shape, o.shape)
        assert torch.equal(audio, o), (i, float((audio.float() - o.float()).abs().max()))
        assert torch.equal(lengths, y_mask[:, 0].sum(-1).long().cpu() * 16)
        assert torch.equal(dur, attn.sum(2)[:, 0].int())
    assert synth.stats["captures"] == 2 and synth.stats["graphs"] == 2 and synth.stats["hits"] >= 4


DEC_REACH = 16          # frames of the tiny decoder's receptive field on each side (conv_pre 3, upsampling 2, resblocks 7.5, conv_post 1)


@pytest.mark.parametrize("amp", [False, True])
def test_session_padded_shapes(pkg, amp):
    """Token axis padded 11 -> 16, frames up to the next multiple of 64.  The same noise values reach the same (item, position)
    in both runs (test_shape_policy_gpu.py's `serve`).  Padding is masked everywhere before the decoder.  The decoder has no
    length mask (as in the reference): past an item's last frame it sees zero frames, and its first convolution turns them into
    its bias.  In an eager batch that already holds for every item but the longest; the longest one ends at the edge of the
    tensor instead (zero padding after that convolution), so its last DEC_REACH frames differ by design and are left out.
    Measured: fp32 1.05e-5 of max|audio| (rounding of the padded token axis carried through the flows), bf16 0."""
    net, x, xl, sid, _ = _net(pkg)
    b, c = x.size(0), net.inter_channels
    gen = torch.Generator().manual_seed(5)
    n_w = torch.randn(b, 2, 64, generator=gen).to(DEV)
    n_e = torch.randn(b, c, 4096, generator=gen).to(DEV)
    orig = (pkg.rng.noise.randn_like, pkg.rng.noise.randn)

    def serve(shape, device, dtype):
        shape = tuple(shape)
        src = n_w if shape[1] == 2 else n_e
        return src[:, :, :shape[2]].to(dtype=dtype).contiguous()

    pkg.rng.noise.randn_like = lambda t: serve(t.shape, t.device, t.dtype)
    pkg.rng.noise.randn = lambda *shape, device=None, dtype=None: serve(shape, device, dtype)
    try:
        synth = pkg.inference.Synthesizer(net, amp=amp, t_x_steps=(16,), frame_step=64)
        errs = []
        for i in range(3):
            o, attn, y_mask = _eager(net, x, xl, sid, amp, 0, **KW)
            audio, lengths, dur = _session(pkg, net, x, xl, sid, amp, 0, synth, **KW)
            assert audio.size(2) % (64 * 16) == 0 and audio.size(2) >= o.size(2)
            assert torch.equal(lengths, y_mask[:, 0].sum(-1).long().cpu() * 16)
            assert torch.equal(dur, attn.sum(2)[:, 0].int())
            for j in range(b):
                n = int(lengths[j])
                if n == o.size(2):                                  # the longest item: eager ended at the tensor's edge
                    n -= DEC_REACH * 16
                ref = o[j, :, :n].float()
                errs.append(float((audio[j, :, :n].float() - ref).abs().max() / ref.abs().max()))
    finally:
        pkg.rng.noise.randn_like, pkg.rng.noise.randn = orig
    print(f"padded session vs infer (amp={amp}): max rel err over valid samples {max(errs):.3e}")
    assert max(errs) <= (2e-5 if not amp else 1e-2), errs


def test_session_forced_durations(pkg):
    net, x, xl, sid, _ = _net(pkg)
    gen = torch.Generator().manual_seed(3)
    durs = torch.randint(1, 5, (x.size(0), 1, x.size(1)), generator=gen).float().to(DEV)
    synth = pkg.inference.Synthesizer(net, amp=True, t_x_steps=(x.size(1),), frame_step=1)
    for seed in (1, 2, 3):
        o, attn, y_mask = _eager(net, x, xl, sid, True, seed, durations=durs, **KW)
        audio, lengths, dur = _session(pkg, net, x, xl, sid, True, seed, synth, durations=durs, **KW)
        assert torch.equal(audio, o) and torch.equal(dur, attn.sum(2)[:, 0].int())
    assert synth.stats["captures"] == 2


def test_scalars_reach_replays(pkg):
    net, x, xl, sid, _ = _net(pkg)
    synth = pkg.inference.Synthesizer(net, amp=False, t_x_steps=(x.size(1),), frame_step=1)
    for seed in (1, 2):                                             # P captured
        _session(pkg, net, x, xl, sid, False, seed, synth, **KW)
    p_graphs = [k for k, e in synth.cache.entries.items() if k[0] == "P" and e["graph"] is not None]
    assert len(p_graphs) == 1
    seen = set()
    for ls, nsw in ((1.0, 0.8), (1.5, 0.8), (1.5, 0.3), (1.0, 1.2)):
        kw = dict(noise_scale=0.667, length_scale=ls, noise_scale_w=nsw)
        o, attn, y_mask = _eager(net, x, xl, sid, False, 9, **kw)
        audio, lengths, dur = _session(pkg, net, x, xl, sid, False, 9, synth, **kw)
        assert torch.equal(lengths, y_mask[:, 0].sum(-1).long().cpu() * 16) and torch.equal(dur, attn.sum(2)[:, 0].int())
        seen.add(tuple(lengths.tolist()))
    assert len(seen) > 1, "the scalars did not change the lengths"
    assert [k for k, e in synth.cache.entries.items() if k[0] == "P" and e["graph"] is not None] == p_graphs


def test_shape_interleave_keeps_earlier_graphs_valid(pkg):
    net, x, xl, sid, _ = _net(pkg)
    gen = torch.Generator().manual_seed(21)
    xa, xla, sa = x[:1, :7], torch.tensor([7], device=DEV), sid[:1]
    xb = torch.randint(1, 20, (4, 96), generator=gen).to(DEV)
    xlb, sb = torch.tensor([96, 90, 80, 50], device=DEV), torch.tensor([0, 1, 2, 1], device=DEV)
    synth = pkg.inference.Synthesizer(net, amp=True, t_x_steps=(7, 96), frame_step=1)
    kw = dict(KW, length_scale=3.0)                                 # B: long utterances, larger workspaces
    for name, (xx, ll, ss) in [("A", (xa, xla, sa))] * 3 + [("B", (xb, xlb, sb))] * 3 + [("A", (xa, xla, sa))] * 2:
        o, _, _ = _eager(net, xx, ll, ss, True, 33, **kw)
        audio, _, _ = _session(pkg, net, xx, ll, ss, True, 33, synth, **kw)
        assert torch.equal(audio, o), name
    graphs = [e["graph"] for e in synth.cache.entries.values() if e["graph"] is not None]
    assert len(graphs) == synth.stats["graphs"] == 4
    assert all(g.pool() == synth._pool for g in graphs)


def test_parameter_update_reaches_replays(pkg):
    net, x, xl, sid, _ = _net(pkg)
    synth = pkg.inference.Synthesizer(net, amp=False, t_x_steps=(x.size(1),), frame_step=1)
    for seed in (1, 2, 3):
        _session(pkg, net, x, xl, sid, False, seed, synth, **KW)
    gen = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p * (1 + 0.05 * torch.randn(p.shape, generator=gen).to(DEV)))
    o, _, _ = _eager(net, x, xl, sid, False, 4, **KW)
    # the lengths are those of the new weights: a new frame capacity may be needed, so compare only once both graphs replay
    for _ in range(3):
        audio, _, _ = _session(pkg, net, x, xl, sid, False, 4, synth, **KW)
    assert torch.equal(audio, o)


def test_replayed_call_makes_one_host_sync(pkg):
    net, x, xl, sid, _ = _net(pkg)
    synth = pkg.inference.Synthesizer(net, amp=True, t_x_steps=(x.size(1),), frame_step=1)
    for seed in (1, 1, 1):
        _session(pkg, net, x, xl, sid, True, seed, synth, **KW)
    run, replays = synth._run, []

    def strict_run(ent, action, fn):
        assert action == "replay"
        replays.append(ent["key"][0])
        torch.cuda.set_sync_debug_mode("error")
        try:
            return run(ent, action, fn)
        finally:
            torch.cuda.set_sync_debug_mode(0)

    synth._run = strict_run
    torch.cuda.set_sync_debug_mode("error")
    try:
        pkey = next(k for k in synth.cache.entries if k[0] == "P")
        synth._inputs(pkey, x, xl, sid, None)                        # the input copies of a call
    finally:
        torch.cuda.set_sync_debug_mode(0)
    hits = synth.stats["hits"]
    torch.manual_seed(1)                                            # the lengths of the calls above: both graphs replay
    synth(x, xl, sid, **KW)
    assert replays == ["P", "S"] and synth.stats["hits"] == hits + 2
