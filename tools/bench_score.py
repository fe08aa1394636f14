#!/usr/bin/env python
"""What teacher-forced scoring costs, on a Llama-3.2-3B-shaped random-init bf16 model:

  score()        llm.score() on --seqs sequences of --prompt prompt rows + --answer answer tokens (one sl_llama_score call per cache-full)
  forward loop   the per-sample loop Trainer.validate runs without its opt-in key: forward(inputs_embeds=[prompt | embed(resp[1:])],
                 labels=[resp]) — hidden_taps, all-position fp32 logits, sl_ce_loss — timed over the first --loop-samples samples and
                 quoted per sample (it is a batch-1 loop: its time is linear in the samples)
  lm_head alone  at --head-rows rows: sl_gemm_top1_lse_tgt + sl_score_finalize (planes) against fp32 logits + sl_score_rows

Times are host clocks around work that ends in a device synchronise; one warm-up per configuration, then --reps, the configurations
alternating; median [min, max].  No ratio is promised: the table is what was measured.

    python tools/bench_score.py [--reps 3] [--seqs 64,1024] [--out profiles/score.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (gpu_llama_state_dict: the flagship's random-init weights, drawn on the GPU)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seqs", default="64,1024")
    ap.add_argument("--prompt", type=int, default=137)
    ap.add_argument("--answer", type=int, default=60)
    ap.add_argument("--loop-samples", type=int, default=64)
    ap.add_argument("--head-rows", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    dev = "cuda:0"
    L, ops, weights, llama_mod, utils = (bench.mod(n) for n in ("_lib", "ops", "weights", "audio_llama", "utils"))
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    seqs = [int(v) for v in args.seqs.split(",")]
    H, V = larch.hidden_size, larch.vocab_size
    llm = llama_mod.AudioLlamaForCausalLM(larch, bench.gpu_llama_state_dict(larch, 0, dev), torch_dtype=torch.bfloat16, device=dev,
                                          max_ctx=((args.prompt + args.answer + 63) // 64) * 64, max_batch=max(seqs))
    emb = llm.model.embed_tokens
    lines = [f"teacher-forced scoring: Llama-3.2-3B shapes, bf16, {args.prompt} prompt rows + {args.answer} answer tokens per sequence, {args.reps} reps "
             f"(median [min, max]), library {os.path.relpath(L.LIB_PATH, REPO)}"]

    def fmt(v):
        return f"{statistics.median(v):10.2f} [{min(v):.2f}, {max(v):.2f}]"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for B in seqs:
        gen = torch.Generator().manual_seed(B)
        prompts = [(torch.randn(args.prompt, H, generator=gen) * 0.05).to(torch.bfloat16).to(dev) for _ in range(B)]
        resp = torch.randint(1, V, (B, args.answer + 1), generator=gen)          # [BOS-like first id | answer]: labels[1:] are the targets
        targets = [resp[b, 1:] for b in range(B)]
        n_loop = min(B, args.loop_samples)

        def run_score():
            run_score.out = llm.score(prompts, targets)

        def run_loop():
            losses = []
            for b in range(n_loop):
                r = resp[b].to(dev)
                seq = torch.cat([prompts[b], emb(r[1:])], 0)
                losses.append(llm(inputs_embeds=seq[None], labels=[r]).loss)
            run_loop.out = torch.stack(losses)

        t_score, t_loop = [], []
        for rep in range(args.reps + 1):
            a, b_ = timed(run_score), timed(run_loop)
            if rep > 0:
                t_score.append(a)
                t_loop.append(b_ / n_loop)
        d = float((run_score.out.nll[:n_loop].float().cpu() - run_loop.out.float().cpu()).abs().max())
        lines.append(f"seqs {B:5d}  score()                   {fmt(t_score)} ms per call = {statistics.median(t_score) / B:8.3f} ms per sequence   paths {sorted(run_score.out.paths)}")
        lines.append(f"seqs {B:5d}  forward(labels=) loop     {fmt(t_loop)} ms per sample (timed over {n_loop} samples)   worst |nll - loss| {d:.3e}")
    # the lm_head pass alone
    M = args.head_rows
    w = llm._dev()
    h = (torch.randn(M, H, generator=torch.Generator().manual_seed(1)) * 0.5).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    ng = (V + 63) // 64
    planes = (torch.empty((ng, M), device=dev, dtype=torch.float32), torch.empty((ng, M), device=dev, dtype=torch.int32), torch.empty((ng, M), device=dev, dtype=torch.float32))
    tv, lp, t1 = torch.zeros(M, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev, dtype=torch.int32)
    logits = torch.empty((M, V), dtype=torch.float32, device=dev)

    def fused():
        val, idx, ssum, _ = ops.gemm_top1_lse_tgt(h, w.lm_head, labels, out=planes, tgt_val=tv)
        ops.score_finalize(val, idx, ssum, tv, labels, V, logprob=lp, top1=t1)

    def unfused():
        ops.gemm(h, w.lm_head, out_f32=True, out=logits)
        ops.score_rows(logits, labels, logprob=lp, top1=t1)

    pair = {"fused (planes)": [], "fp32 logits + sl_score_rows": []}
    for rep in range(args.reps + 1):
        for name, fn in (("fused (planes)", fused), ("fp32 logits + sl_score_rows", unfused)):
            ms = timed(lambda: [fn() for _ in range(4)]) / 4
            if rep > 0:
                pair[name].append(ms)
    for name, v in pair.items():
        lines.append(f"lm_head pass alone, {M} rows, {name:28s} {fmt(v)} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
