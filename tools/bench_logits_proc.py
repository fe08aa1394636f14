"""The decode step with HF's logits processors on against the same step with them off, in one process, alternating, on the same random
weights and inputs (Llama-3.2-3B shapes, bf16, 137-token prompts).

Measured at 1 024, 256 and 1 rows: ms per captured decode step and tok/s with the processors off (above 64 rows a greedy step then runs
the lm_head with the fused per-64-column top-1) and on (repetition_penalty 1.2 + no_repeat_ngram_size 3 + min_new_tokens 8: the unfused
lm_head -> fp32 logits -> sl_logits_process -> sl_greedy_select); the process kernel alone (us per launch, raw and log_softmax mode);
and how many of 1 024 random-init sequences run to max_new_tokens without emitting EOS, with and without no_repeat_ngram_size = 3.

    python tools/bench_logits_proc.py [--reps 5] [--out profiles/logits_proc.txt]

The report goes to stdout and, with --out, to that file as well (profiles/logits_proc.txt is the committed run).
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
ON = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8)


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
    ap.add_argument("--loop-tokens", type=int, default=128, help="max_new_tokens of the looping-rows count")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/logits_proc.txt)")
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
    max_new = max(new, args.loop_tokens)
    max_ctx = ((S + max_new + 8 + 63) // 64) * 64
    V, nl = larch.vocab_size, larch.num_hidden_layers
    print(f"# tools/bench_logits_proc.py --reps {args.reps}: medians of {args.reps} alternating runs after one warm-up round; {nl} layers, bf16, random init, "
          f"{S}-token prompts, {new} new tokens, max_ctx {max_ctx}; device {torch.cuda.get_device_name(0)}")
    print(f"# processors on = {ON}")

    # ---- 1. the process kernel alone: histories of new / 2 tokens over a 50-token alphabet (every n-gram repeats)
    print(f"\n## logits_process_kernel, vocab {V}, histories of {new // 2} tokens (us per launch of R blocks)")
    print(f"{'rows':>6s} {'mode':>12s} {'us':>10s} {'logits MB':>10s}")
    gen = torch.Generator().manual_seed(3)
    for R in args.rows:
        logits = torch.randn(R, V, generator=gen).to(dev)
        hist = torch.randint(0, 50, (R, new), generator=gen, dtype=torch.int32).to(dev)
        hist_len = torch.full((R,), new // 2, dtype=torch.int32, device=dev)
        scratch = torch.empty(R * new, device=dev)
        lp = L.LogitsOpts()
        lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = ON["repetition_penalty"], ON["no_repeat_ngram_size"], ON["min_new_tokens"]
        eos = (C.c_int32 * 8)(1, 2, 3, 0, 0, 0, 0, 0)
        for name, lsm in (("raw", 0), ("log_softmax", 1)):
            run = lambda: L.check(lib.sl_logits_process(logits.data_ptr(), R, V, hist.data_ptr(), new, hist_len.data_ptr(), None, C.byref(lp), eos, 3, lsm,
                                                        scratch.data_ptr(), L.stream_ptr()), "sl_logits_process")
            us = statistics.median(event_us(run, args.launches) for _ in range(args.reps + 1))
            print(f"{R:6d} {name:>12s} {us:10.1f} {R * V * 4 / 1e6:10.1f}", flush=True)
        del logits
    torch.cuda.empty_cache()

    # ---- 2. the model
    bench = importlib.import_module("bench")
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(bench.gpu_llama_state_dict(larch, 0, dev)), torch_dtype=dt, device=dev, max_ctx=max_ctx,
                                          max_batch=max(args.rows))
    eos_cfg = llm.generation_config.eos_token_id
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, larch.hidden_size, generator=gen) * 0.05).to(dev, dt)

    # ---- 3. the captured step: processors off against on at the same row count (EOS off: every call runs every step)
    print("\n## captured decode step, greedy (ms per step = decode_ms / decode launches; tok/s = rows / step)")
    print(f"{'rows':>6s} {'processors':>12s} {'ms/step':>10s} {'tok/s':>12s} {'vs off':>8s}")
    llm.generation_config.eos_token_id = None
    for R in args.rows:
        modes = {"off": None, "on": dict(ON, min_new_tokens=0), "on (n-gram)": dict(no_repeat_ngram_size=3)}
        times = {k: [] for k in modes}
        for rep in range(args.reps + 1):
            for name, logits in modes.items():
                llm.generate_packed(x_all[:R * S].clone(), [S] * R, new, use_eos=False, compact=False, logits=logits)
                torch.cuda.synchronize()
                if rep > 0:
                    times[name].append(llm.last_timings_ms[1] / max(1, llm.last_generate_stats["decode_launches"]))
        off = statistics.median(times["off"])
        for name in modes:
            m = statistics.median(times[name])
            print(f"{R:6d} {name:>12s} {m:10.3f} {R / m * 1e3:12.0f} {m / off:8.3f}", flush=True)
        llm._kv = None
        llm._ws = None
        torch.cuda.empty_cache()

    # ---- 4. looping rows: sequences that reach max_new_tokens without EOS, with and without no_repeat_ngram_size = 3
    R, n = max(args.rows), args.loop_tokens
    llm.generation_config.eos_token_id = eos_cfg
    print(f"\n## {R} random-init sequences, {n} new tokens, EOS ids {eos_cfg}: rows that reach max_new_tokens without EOS; decode launches x rows actually run")
    print(f"{'processors':>28s} {'rows without EOS':>18s} {'row steps':>12s} {'decode ms':>10s}")
    for name, logits in (("off", None), ("no_repeat_ngram_size=3", dict(no_repeat_ngram_size=3)), ("all three", ON)):
        ids, n_cols = llm.generate_packed(x_all[:R * S].clone(), [S] * R, n, use_eos=True, compact=True, logits=logits)
        torch.cuda.synchronize()
        eos_t = torch.tensor(list(eos_cfg) if isinstance(eos_cfg, (list, tuple)) else [eos_cfg])
        no_eos = int((~torch.isin(ids.long(), eos_t).any(dim=1)).sum())
        print(f"{name:>28s} {no_eos:18d} {llm.last_generate_stats['row_steps']:12d} {llm.last_timings_ms[1]:10.1f}", flush=True)


if __name__ == "__main__":
    main()
