"""Beam search against the greedy step of the same build at the same row count, in one process, alternating, on the same random
weights and inputs (Llama-3.2-3B shapes, bf16, 137-token prompts, 64 new tokens).

Measured: ms per captured decode step of beam K in {2, 4} at nseq * K in {64, 256, 1 024} rows against the greedy step at that row
count (EOS off, so every call runs every step); the selection kernel alone (us per launch, bytes of logits read once) and the cache
re-ordering alone (us per gather + scatter pair when every row changes its slot, bytes moved) at the same row counts.

    python tools/bench_beam.py [--reps 5] [--out profiles/beam_vs_greedy.txt]

The report goes to stdout and, with --out, to that file as well (profiles/beam_vs_greedy.txt is the committed run).
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "llm-speech-summarization_amd"


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
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--beams", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--prompt", type=int, default=137)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/beam_vs_greedy.txt)")
    args = ap.parse_args()
    if args.out:
        out_f = open(args.out, "w")

        class Tee:
            def write(self, t):
                sys.__stdout__.write(t); out_f.write(t); out_f.flush()

            def flush(self):
                sys.__stdout__.flush()
        sys.stdout = Tee()
    L, weights, llama_mod, utils = mod("_lib"), mod("weights"), mod("audio_llama"), mod("utils")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.lib()
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    if args.layers:
        import dataclasses
        larch = dataclasses.replace(larch, num_hidden_layers=args.layers)
    S, new, dt = args.prompt, args.new_tokens, torch.bfloat16
    max_ctx = ((S + new + 8 + 63) // 64) * 64
    V, nkv, D, nl = larch.vocab_size, larch.num_key_value_heads, larch.head_dim, larch.num_hidden_layers
    print(f"# tools/bench_beam.py --reps {args.reps}: medians of {args.reps} alternating runs after one warm-up round; {nl} layers, bf16, random init, "
          f"{S}-token prompts, {new} new tokens, max_ctx {max_ctx}; device {torch.cuda.get_device_name(0)}")

    # ---- 1. the selection kernel alone
    print(f"\n## beam_topk_kernel, vocab {V} (us per launch of R blocks; logits bytes = R x V x 4)")
    print(f"{'rows':>6s} {'M':>4s} {'us':>10s} {'logits MB':>10s} {'GB/s if read once':>18s}")
    gen = torch.Generator().manual_seed(3)
    for R in args.rows:
        logits = torch.randn(R, V, generator=gen).to(dev)
        score = torch.zeros(R, device=dev)
        for K in args.beams:
            M = 2 * K
            val = torch.empty(R * M, device=dev)
            tok = torch.empty(R * M, dtype=torch.int32, device=dev)
            run = lambda: L.check(lib.sl_beam_topk(logits.data_ptr(), R, V, score.data_ptr(), M, val.data_ptr(), tok.data_ptr(), L.stream_ptr()), "sl_beam_topk")
            us = statistics.median(event_us(run, args.launches) for _ in range(args.reps + 1))
            print(f"{R:6d} {M:4d} {us:10.1f} {R * V * 4 / 1e6:10.1f} {R * V * 4 / us / 1e3:18.1f}", flush=True)
        del logits
    torch.cuda.empty_cache()

    # ---- 2. the model
    bench = importlib.import_module("bench")
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(bench.gpu_llama_state_dict(larch, 0, dev)), torch_dtype=dt, device=dev, max_ctx=max_ctx,
                                          max_batch=max(args.rows))
    llm.generation_config.eos_token_id = None
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, larch.hidden_size, generator=gen) * 0.05).to(dev, dt)

    # ---- 3. the cache re-ordering alone: every row takes its neighbour's slot, spans of new / 2 positions
    print(f"\n## kv_beam_gather + kv_beam_scatter, every row changes its slot, span {new // 2} positions (us per pair; bytes = 4 x R x layers x kv heads x span x row bytes)")
    print(f"{'rows':>6s} {'us':>10s} {'MB moved':>10s} {'TB/s':>8s}")
    for R in args.rows:
        kv = llm._kv_cache(R, 0)
        span = new // 2
        need = lib.sl_kv_beam_staging_bytes(C.byref(kv), C.byref(llm._dev().struct), R, span)
        staging = torch.empty(need, dtype=torch.uint8, device=dev)
        src = torch.tensor([r ^ 1 for r in range(R)], dtype=torch.int32).to(dev)
        p = torch.full((R,), S, dtype=torch.int32, device=dev)
        c = p + span
        run = lambda: L.check(lib.sl_kv_beam_reorder(C.byref(kv), C.byref(llm._dev().struct), src.data_ptr(), p.data_ptr(), c.data_ptr(), R, span,
                                                     staging.data_ptr(), need, L.stream_ptr()), "sl_kv_beam_reorder")
        us = statistics.median(event_us(run, args.launches) for _ in range(args.reps + 1))
        moved = 4.0 * R * nl * nkv * span * D * 2
        print(f"{R:6d} {us:10.1f} {moved / 1e6:10.1f} {moved / us / 1e6:8.2f}", flush=True)
        del staging
    torch.cuda.empty_cache()

    # ---- 4. the captured step: beam K against greedy at the same row count
    print("\n## captured decode step (ms per step = decode_ms / decode launches)")
    print(f"{'rows':>6s} {'mode':>10s} {'ms/step':>10s} {'vs greedy':>10s}")
    for R in args.rows:
        modes = {"greedy": (R, None)}
        for K in args.beams:
            modes[f"beam K={K}"] = (R // K, dict(num_beams=K))
        times = {k: [] for k in modes}
        for rep in range(args.reps + 1):
            for name, (nseq, beams) in modes.items():
                x = x_all[:nseq * S].clone()
                llm.generate_packed(x, [S] * nseq, new, use_eos=False, compact=False, beams=beams)
                torch.cuda.synchronize()
                if rep > 0:
                    times[name].append(llm.last_timings_ms[1] / max(1, llm.last_generate_stats["decode_launches"]))
        g = statistics.median(times["greedy"])
        for name in modes:
            m = statistics.median(times[name])
            print(f"{R:6d} {name:>10s} {m:10.3f} {m / g:10.3f}", flush=True)
        llm._kv = None
        llm._ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
