#!/usr/bin/env python3
"""Inference benchmarks of the captured session (inference.Synthesizer).  Prints one JSON line.

    python tools/bench_infer.py --mode c4 --execution session [--steps K --warmup W --dump-outputs DIR]
    python tools/bench_infer.py --mode interactive [--prompts N]

--mode c4: workload C4 exactly as `bench.py --workload C4` runs it (same seed, model, inputs and call count), with --execution
eager (infer()) or session (Synthesizer at infer()'s shapes: the same noise draws, so --dump-outputs DIR writes the same waveform
as `bench.py --workload C4 --dump-outputs DIR`, as DIR/o.npy).

--mode interactive: the reference's use of inference (VC_inference.py:48, cmd_inference.py:113) — one sentence at batch 1,
stochastic durations, noise_scale .667, noise_scale_w .8, length_scale 1 — over seeded prompts of 31-201 tokens (blanks
interspersed): eager infer() and the session in the same run, p50 / p90 latency, real-time factor and the predicted lengths.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")   # before the HIP runtime initialises; see the package __init__

import torch  # noqa: E402


def build(P, cfgs):
    hps = cfgs.get(cfgs.C4["config"])
    torch.manual_seed(hps.train.seed)
    g = P.SynthesizerTrn(hps.n_symbols, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                         n_speakers=hps.data.n_speakers, **hps.model).to("cuda:0").eval()
    return g, hps


def bench_c4(args, P, cfgs):
    g, hps = build(P, cfgs)
    x, xl, sid, dur = cfgs.c4_inputs(hps, "cuda:0")
    kw = dict(noise_scale=cfgs.C4["noise_scale"], noise_scale_w=cfgs.C4["noise_scale_w"], durations=dur)
    synth = P.inference.Synthesizer(g, amp=not args.fp32, t_x_steps=(x.size(1),), frame_step=1) if args.execution == "session" else None
    ac = torch.autocast("cuda", dtype=torch.bfloat16, enabled=not args.fp32)

    def step():
        if synth is not None:
            return synth(x, xl, sid=sid, **kw)[0]
        with torch.no_grad(), ac:
            return g.infer(x, xl, sid=sid, **kw)[0]

    for _ in range(args.warmup):
        o = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        o = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "o.npy"), o.detach().float().cpu().numpy())
    assert bool(torch.isfinite(o).all())
    samples = o.size(0) * o.size(-1) * args.steps
    return dict(metric="22.05 kHz waveform samples/sec, VITS infer()", value=samples / elapsed, unit="samples/s", n_gpus=1,
                steps=args.steps, warmup=args.warmup, ms_per_step=elapsed / args.steps * 1e3, higher_is_better=True,
                dtype="fp32" if args.fp32 else "bf16", data="synthetic",
                session_stats=dict(synth.stats) if synth is not None else None,
                config=dict(workload=f"C4: batch {o.size(0)}, T_x = {x.size(1)} tokens, {o.size(-1)} samples per item (durations forced)",
                            execution="hipGraph replay (inference session)" if synth is not None else "eager launches"))


def bench_interactive(args, P, cfgs):
    g, hps = build(P, cfgs)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(4321)
    prompts = []
    for _ in range(args.prompts):
        n = int(torch.randint(15, 101, (1,), generator=gen))
        x = torch.zeros(1, 2 * n + 1, dtype=torch.long)
        x[0, 1::2] = torch.randint(1, hps.n_symbols, (n,), generator=gen)
        spk = int(torch.randint(0, 10, (1,), generator=gen))
        prompts.append((x.to(dev), torch.tensor([2 * n + 1], device=dev), torch.tensor([spk], device=dev)))
    kw = dict(noise_scale=0.667, noise_scale_w=0.8, length_scale=1.0)
    ac = torch.autocast("cuda", dtype=torch.bfloat16, enabled=not args.fp32)
    synth = P.inference.Synthesizer(g, amp=not args.fp32, max_graphs=256)

    def eager(x, xl, sid):
        with torch.no_grad(), ac:
            o, _, y_mask, _ = g.infer(x, xl, sid=sid, **kw)
        return o, y_mask

    warmup = max(args.warmup, 2)                  # every key seen twice: warm-up + capture (seeded: the timed calls predict the same lengths)
    for _ in range(warmup):
        for i, (x, xl, sid) in enumerate(prompts):
            torch.manual_seed(i)
            eager(x, xl, sid)
            torch.manual_seed(i)
            synth(x, xl, sid, **kw)
    torch.cuda.synchronize()
    captures = synth.stats["captures"]
    lat_e, lat_s, frames, frames_s = [], [], [], []
    for i, (x, xl, sid) in enumerate(prompts):
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o, y_mask = eager(x, xl, sid)
        torch.cuda.synchronize()
        lat_e.append(time.perf_counter() - t0)
        frames.append(int(y_mask.sum()))
        torch.manual_seed(i)
        t0 = time.perf_counter()
        audio, lengths, _ = synth(x, xl, sid, **kw)
        torch.cuda.synchronize()
        lat_s.append(time.perf_counter() - t0)
        frames_s.append(int(lengths[0]) // synth.hop)

    def pct(v, q):
        v = sorted(v)
        return v[min(len(v) - 1, int(round(q * (len(v) - 1))))] * 1e3

    secs = sum(f * synth.hop / hps.data.sampling_rate for f in frames)
    return dict(metric="batch-1 utterance latency p50, VITS inference session", value=pct(lat_s, 0.5), unit="ms", n_gpus=1,
                prompts=len(prompts), warmup=warmup, higher_is_better=False, dtype="fp32" if args.fp32 else "bf16", data="synthetic",
                latency_ms=dict(eager=dict(p50=pct(lat_e, 0.5), p90=pct(lat_e, 0.9)), session=dict(p50=pct(lat_s, 0.5), p90=pct(lat_s, 0.9))),
                real_time_factor=dict(eager=sum(lat_e) / secs, session=sum(lat_s) / secs),
                tokens=[int(p[1]) for p in prompts], predicted_frames=frames, session_frames=frames_s,
                session_stats=dict(synth.stats, captures_during_timing=synth.stats["captures"] - captures),
                config=dict(workload=f"interactive: batch 1, {len(prompts)} prompts of 31-201 tokens, stochastic durations",
                            execution="eager launches vs hipGraph replay (inference session)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("c4", "interactive"), required=True)
    ap.add_argument("--execution", choices=("eager", "session"), default="session", help="--mode c4 only")
    ap.add_argument("--steps", type=int, default=5, help="--mode c4: timed batches")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prompts", type=int, default=24, help="--mode interactive: number of prompts")
    ap.add_argument("--fp32", action="store_true", help="no bf16 autocast")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="--mode c4: write the last batch's waveform as DIR/o.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.prompts < 1:
        raise SystemExit("--steps and --prompts must be at least 1")
    from importlib import import_module
    P = import_module("personalized_text-to-speech_amd")
    cfgs = import_module("personalized_text-to-speech_amd.configs")
    P._lib.lib()
    line = bench_c4(args, P, cfgs) if args.mode == "c4" else bench_interactive(args, P, cfgs)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
