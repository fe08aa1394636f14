#!/usr/bin/env python
"""What token log-probabilities cost: the decode step of a Llama-3.2-3B-shaped random-init bf16 model at 1 024, 256 and 1 rows

  off           generate_packed(scores=False): the step as it was (compare with the same tool run on the parent commit)
  on            scores=True: above 64 rows the lm_head's fused top-1 carries the third plane, sl_greedy_select_partial_sc finishes
  on unfused+p  scores=True through fp32 logits, forced by a logits processor that can never act (no_repeat_ngram_size above the budget):
             lm_head -> fp32 logits -> sl_logits_process (a no-op pass) -> sl_greedy_select_sc; an upper bound of the unfused form
  on unfused    derived: off - (fused lm_head + select, alone) + (fp32-logits lm_head + sl_greedy_select_sc, alone)
  direct        the unfused form itself, with no processor pass: sl_llama_decode_step (the decode step without the fused top-1: fp32 logits)
                + sl_greedy_select / sl_greedy_select_sc on the caches the calls above filled, one step captured as a graph and replayed,
                events around the replays.  Its own harness (no prefetch branch, three more small launches per step): compare its
                two lines with each other, and their difference with on - off.

and the lm_head + select pair alone, each form.  Steps are timed by the events sl_generate records around its graph replays
(last_timings_ms[1] / decode launches); the pairs alone by events around back-to-back launches.  One warm-up call per configuration
(captures the graphs), then --reps calls, the configurations alternating; median and spread are printed.

    python tools/bench_token_scores.py [--reps 5] [--rows 1024,256,1] [--out profiles/token_scores.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (gpu_llama_state_dict: the flagship's random-init weights, drawn on the GPU)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="1024,256,1")
    ap.add_argument("--prompt", type=int, default=128, help="prompt rows per sequence")
    ap.add_argument("--new", type=int, default=33, help="tokens per call (new - 1 decode steps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    dev = "cuda:0"
    L, ops, weights, llama_mod, utils = (bench.mod(n) for n in ("_lib", "ops", "weights", "audio_llama", "utils"))
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    rows = [int(r) for r in args.rows.split(",")]
    llm = llama_mod.AudioLlamaForCausalLM(larch, bench.gpu_llama_state_dict(larch, 0, dev), torch_dtype=torch.bfloat16, device=dev,
                                          max_ctx=((args.prompt + args.new + 63) // 64) * 64, max_batch=max(rows))
    llm.generation_config.eos_token_id = None
    lines = [f"token log-probabilities: decode step, Llama-3.2-3B shapes, bf16, prompt {args.prompt}, {args.new - 1} steps per call, {args.reps} reps (median [min, max]) "
             f"library {os.path.relpath(L.LIB_PATH, REPO)}"]
    has_sc = hasattr(llm, "last_token_logprobs")
    never = dict(repetition_penalty=1.0, no_repeat_ngram_size=args.new + 8, min_new_tokens=0)

    def fmt(v):
        return f"{statistics.median(v):8.3f} [{min(v):.3f}, {max(v):.3f}]"

    for B in rows:
        x = (torch.randn(B * args.prompt, larch.hidden_size, generator=torch.Generator().manual_seed(B)) * 0.05).to(torch.bfloat16).to(dev)
        lens = [args.prompt] * B
        cfgs = {"off": dict()}
        if has_sc:
            cfgs.update({"on": dict(scores=True), "on unfused+p": dict(scores=True, logits=never)})
        if has_sc:
            llm.generate_packed(x.clone(), lens, args.new, use_eos=False, scores=True, logits=dict(never, repetition_penalty=1.1))      # the largest workspace first
        times = {k: [] for k in cfgs}
        ids = {}
        for rep in range(args.reps + 1):
            for name, kw in cfgs.items():
                r = llm.generate_packed(x.clone(), lens, args.new, use_eos=False, **kw)
                ids[name] = r[0]
                if rep > 0:
                    times[name].append(llm.last_timings_ms[1] / llm.last_generate_stats["decode_launches"])
        for name in cfgs:
            assert torch.equal(ids[name], ids["off"]), name                    # the same tokens in every configuration
            lines.append(f"rows {B:5d}  step {name:13s} {fmt(times[name])} ms")
        # lm_head + select alone
        if B > 64:
            w = llm._dev()
            h = (torch.randn(B, larch.hidden_size, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
            st = lambda: dict(unfinished=torch.ones(B, dtype=torch.int32, device=dev), ctx=torch.zeros(B, dtype=torch.int32, device=dev),   # noqa: E731
                              gen=torch.zeros(B, dtype=torch.int32, device=dev), fin=torch.zeros(B, dtype=torch.int32, device=dev),
                              nxt=torch.zeros(B, dtype=torch.int32, device=dev), out=torch.zeros((B, 64), dtype=torch.int32, device=dev))
            lp = torch.zeros((B, 64), dtype=torch.float32, device=dev)
            logits = torch.empty((B, larch.vocab_size), dtype=torch.float32, device=dev)

            def run(kind, s):
                a = ([], 0, False, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"])
                if kind == "fused":
                    val, idx = ops.gemm_top1(h, w.lm_head)
                    ops.greedy_select_partial(val, idx, *a)
                elif kind == "fused+plane":
                    val, idx, ssum = ops.gemm_top1_lse(h, w.lm_head)
                    ops.greedy_select_partial_sc(val, idx, ssum, *a, lp)
                elif kind == "logits":
                    ops.gemm(h, w.lm_head, out_f32=True, out=logits)
                    ops.greedy_select(logits, *a)
                else:
                    ops.gemm(h, w.lm_head, out_f32=True, out=logits)
                    ops.greedy_select_sc(logits, *a, lp)

            kinds = ["fused", "logits"] + (["fused+plane", "logits+lse"] if has_sc else [])
            pair = {k: [] for k in kinds}
            for rep in range(args.reps + 1):
                for kind in kinds:
                    s = st()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(16):
                        run(kind, s)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep > 0:
                        pair[kind].append(e0.elapsed_time(e1) / 16)
            for kind in kinds:
                lines.append(f"rows {B:5d}  lm_head + select alone, {kind:12s} {fmt(pair[kind])} ms")
            # the unfused form itself: decode step -> fp32 logits -> row select, one captured step replayed
            lib = L.lib()
            struct, _ = llm._struct_for(B)
            kv = llm._kv_cache(B)
            ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(struct), B * args.prompt, B, args.new))
            s = st()

            def reset():
                s["ctx"].fill_(args.prompt)
                s["gen"].zero_()

            def step(sc):
                L.check(lib.sl_llama_decode_step(C.byref(struct), C.byref(kv), s["nxt"].data_ptr(), s["ctx"].data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
                a = ([], 0, False, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"])
                if sc:
                    ops.greedy_select_sc(logits, *a, lp)
                else:
                    ops.greedy_select(logits, *a)

            direct = {}
            for sc in ([False, True] if has_sc else [False]):
                reset()
                step(sc)
                torch.cuda.synchronize()
                reset()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step(sc)
                direct[sc] = (graph, [])
            for rep in range(args.reps + 1):
                for sc, (graph, acc) in direct.items():
                    reset()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.new - 1):
                        graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep > 0:
                        acc.append(e0.elapsed_time(e1) / (args.new - 1))
            for sc, (graph, acc) in direct.items():
                lines.append(f"rows {B:5d}  step direct unfused, scores {'on ' if sc else 'off'} {fmt(acc)} ms")
            if has_sc:
                derived = statistics.median(times["off"]) - statistics.median(pair["fused"]) + statistics.median(pair["logits+lse"])
                lines.append(f"rows {B:5d}  step unfused (derived: off - fused pair + logits+lse pair) {derived:8.3f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
