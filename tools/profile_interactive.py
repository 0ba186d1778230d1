"""One batch-1 utterance of bench.py's interactive set (prompt 0: stochastic durations, the reference's scalars), called
--calls times after two warm-up calls, eagerly or through inference.Synthesizer.  Meant to run under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/profile_interactive.py --mode session`
(profiles/r04_interactive_*_kernel_stats_all.csv: 12 calls per file)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("eager", "session"), required=True)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from importlib import import_module
    P = import_module("personalized_text-to-speech_amd")
    cfgs = import_module("personalized_text-to-speech_amd.configs")
    hps = cfgs.get(cfgs.C4["config"])
    torch.manual_seed(hps.train.seed)
    dev = torch.device("cuda:0")
    g = P.SynthesizerTrn(hps.n_symbols, hps.data.filter_length // 2 + 1, hps.train.segment_size // hps.data.hop_length,
                         n_speakers=hps.data.n_speakers, **hps.model).to(dev).eval()
    gen = torch.Generator().manual_seed(4321)
    n = int(torch.randint(15, 101, (1,), generator=gen))
    x = torch.zeros(1, 2 * n + 1, dtype=torch.long)
    x[0, 1::2] = torch.randint(1, hps.n_symbols, (n,), generator=gen)
    x, xl, sid = x.to(dev), torch.tensor([2 * n + 1], device=dev), torch.tensor([0], device=dev)
    kw = dict(noise_scale=0.667, noise_scale_w=0.8, length_scale=1.0)
    synth = P.inference.Synthesizer(g, amp=True)

    def call():
        torch.manual_seed(0)
        if args.mode == "session":
            return synth(x, xl, sid, **kw)[0]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return g.infer(x, xl, sid, **kw)[0]

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    for _ in range(args.calls):
        o = call()
    torch.cuda.synchronize()
    print(f"{args.mode}: t_x {x.size(1)}, {o.size(-1)} samples, {args.calls} timed calls after 2 warm-up calls, stats {synth.stats}")


if __name__ == "__main__":
    main()
