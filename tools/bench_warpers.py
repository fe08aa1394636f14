"""The sampled decode step with each of HF's four further warpers on against the same step with them off, in one process, alternating, on
the same random weights and inputs (Llama-3.2-3B shapes, bf16, 137-token prompts), and the selection kernel alone.

Measured at 1 024, 256 and 1 rows: ms per captured decode step and tok/s with sampling on (temperature 0.8, top_k 50, top_p 0.95: the
unfused lm_head -> fp32 logits -> sample_rows_kernel<false>) and, on top of that, min_p / typical_p / epsilon_cutoff / eta_cutoff one at a time and
all four (sample_rows_kernel<true>); then the two instantiations alone on Gaussian rows of the real vocabulary (us per launch).

    python tools/bench_warpers.py [--reps 5] [--out profiles/warpers.txt]

The report goes to stdout and, with --out, to that file as well.
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "llm-speech-summarization_amd"
BASE = dict(temperature=0.8, top_k=50, top_p=0.95, seed=1234)
MODES = {"off": {}, "min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "epsilon_cutoff": dict(epsilon_cutoff=3e-4),
         "eta_cutoff": dict(eta_cutoff=2e-3), "all four": dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)}


def mod(name):
    return importlib.import_module(PKG + "." + name)


def event_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 256, 1])
    ap.add_argument("--prompt", type=int, default=137)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file ")
    args = ap.parse_args()
    if args.out:
        out_f = open(args.out, "w")

        class Tee:
            def write(self, t):
                sys.__stdout__.write(t); out_f.write(t); out_f.flush()

            def flush(self):
                sys.__stdout__.flush()
        sys.stdout = Tee()
    L, ops, weights, llama_mod, utils = mod("_lib"), mod("ops"), mod("weights"), mod("audio_llama"), mod("utils")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    if args.layers:
        import dataclasses
        larch = dataclasses.replace(larch, num_hidden_layers=args.layers)
    S, new, dt = args.prompt, args.new_tokens, torch.bfloat16
    max_ctx = ((S + new + 8 + 63) // 64) * 64
    V, nl = larch.vocab_size, larch.num_hidden_layers
    print(f"# tools/bench_warpers.py --reps {args.reps}: medians of {args.reps} alternating runs after one warm-up round; {nl} layers, bf16, random init, "
          f"{S}-token prompts, {new} new tokens, max_ctx {max_ctx}; device {torch.cuda.get_device_name(0)}")
    print(f"# sampling = {BASE}")

    # ---- 1. the selection kernels alone (draw + commit launches), Gaussian rows (std 2.5) of the real vocabulary
    print(f"\n## selection alone, vocab {V} (us per call: the draw's launch of R blocks + the commit's)")
    print(f"{'rows':>6s} {'warpers':>16s} {'us':>10s} {'vs off':>8s} {'logits MB':>10s}")
    gen = torch.Generator().manual_seed(3)
    i32 = dict(dtype=torch.int32, device=dev)
    for R in args.rows:
        logits = (torch.randn(R, V, generator=gen) * 2.5).to(dev)
        st = [torch.ones(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros(R, **i32), torch.zeros((R, 4), **i32)]
        off = None
        for name, warp in MODES.items():
            def run():
                ops.sample_select_w(logits, BASE["temperature"], BASE["top_k"], BASE["top_p"], BASE["seed"], [], 0, False, *st, None, warp or None)
            us = statistics.median(event_us(run, args.launches) for _ in range(args.reps + 1))
            off = us if off is None else off
            print(f"{R:6d} {name:>16s} {us:10.1f} {us / off:8.3f} {R * V * 4 / 1e6:10.1f}", flush=True)
        del logits
    torch.cuda.empty_cache()

    # ---- 2. the captured step: each option off against on at the same row count (EOS off: every call runs every step)
    bench = importlib.import_module("bench")
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(bench.gpu_llama_state_dict(larch, 0, dev)), torch_dtype=dt, device=dev, max_ctx=max_ctx,
                                          max_batch=max(args.rows))
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, larch.hidden_size, generator=gen) * 0.05).to(dev, dt)
    print("\n## captured decode step, sampling (ms per step = decode_ms / decode launches; tok/s = rows / step)")
    print(f"{'rows':>6s} {'warpers':>16s} {'ms/step':>10s} {'tok/s':>12s} {'vs off':>8s}")
    llm.generation_config.eos_token_id = None
    for R in args.rows:
        times = {k: [] for k in MODES}
        for rep in range(args.reps + 1):
            for name, warp in MODES.items():
                llm.generate_packed(x_all[:R * S].clone(), [S] * R, new, use_eos=False, compact=False, sample=dict(BASE, **warp))
                torch.cuda.synchronize()
                if rep > 0:
                    times[name].append(llm.last_timings_ms[1] / max(1, llm.last_generate_stats["decode_launches"]))
        off = statistics.median(times["off"])
        for name in MODES:
            m = statistics.median(times[name])
            print(f"{R:6d} {name:>16s} {m:10.3f} {R / m * 1e3:12.0f} {m / off:8.3f}", flush=True)
        llm._kv = None
        llm._ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
