"""fp16 against bf16, stage by stage, on the same random weights and inputs (HuBERT-large + Llama-3.2-3B shapes).

Each stage runs in bf16 and in fp16 alternately, `--reps` times each after a warm-up; the medians and their ratio are printed.
Stages: the encoder pass (256 utterances of 10 s), the configs[1] prefill (256 prompts of [prefix | audio | suffix]), one decode
step at 1 024 rows, per-token batch-1 decode, generate_audio_response of one utterance (encode + prefill + 64 greedy tokens).

    python tools/bench_fp16.py [--reps 5] > profiles/fp16_vs_bf16.txt
"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "llm-speech-summarization_amd"


def mod(name):
    return importlib.import_module(PKG + "." + name)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--enc-batch", type=int, default=256)
    ap.add_argument("--prefill-batch", type=int, default=256)
    ap.add_argument("--decode-rows", type=int, default=1024)
    ap.add_argument("--new-tokens", type=int, default=64)
    args = ap.parse_args()
    L, ri, cfgm, weights = mod("_lib"), mod("random_init"), mod("config"), mod("weights")
    enc_mod, llama_mod, utils = mod("audio_encoder"), mod("audio_llama"), mod("utils")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.lib()
    harch, larch = weights.KNOWN_HUBERT["facebook/hubert-large-ls960-ft"], weights.KNOWN_LLAMA[utils.LLAMA_ID]
    conf = cfgm.load_config(os.path.join(REPO, "config", "llama3_hubert.yaml"))
    enc_sd = ri.hubert_encoder_state_dict(harch, larch.hidden_size, seed=0)
    bench = importlib.import_module("bench")
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)           # bf16 values; fp16 holds them exactly (|w| << 65 504)
    prefix = ri.synthetic_ids(9, larch.vocab_size, seed=7, bos=larch.bos_token_id or 0)
    suffix = ri.synthetic_ids(6, larch.vocab_size, seed=8, bos=larch.bos_token_id or 0)
    n_samples = 160000
    waves = [ri.synthetic_waveform(n_samples, seed=100 + i) for i in range(args.enc_batch)]
    P = (harch.num_frames(n_samples) - 8) // 4 + 1
    S = prefix.shape[1] + P + suffix.shape[1] - 1
    max_ctx = ((S + args.new_tokens + 8 + 63) // 64) * 64
    gen = torch.Generator().manual_seed(5)
    x_pre = (torch.randn(args.prefill_batch * S, larch.hidden_size, generator=gen) * 0.05)
    x_dec = (torch.randn(args.decode_rows * S, larch.hidden_size, generator=gen) * 0.05)

    models = {}
    for dt in (torch.bfloat16, torch.float16):
        enc = enc_mod.AudioEncoder(conf, dev, dtype=dt, arch=harch)
        enc.load_state_dict(enc_sd).eval().to(dev)
        llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx,
                                              max_batch=max(args.decode_rows, args.prefill_batch))
        llm.generation_config.eos_token_id = None
        models[dt] = (enc, llm)
    del llm_sd

    def prefill(llm, x, B):
        w = llm._dev()
        cu = (C.c_int32 * (B + 1))(*[S * b for b in range(B + 1)])
        kv = llm._kv_cache(B, 0)
        ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), x.shape[0], B, 1))
        logits = torch.empty((B, larch.vocab_size), device=dev, dtype=torch.float32)
        ctx = torch.empty(B, device=dev, dtype=torch.int32)
        L.check(lib.sl_llama_prefill(C.byref(w.struct), C.byref(kv), x.data_ptr(), cu, B, logits.data_ptr(), ctx.data_ptr(), None,
                                     ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
        return kv, ws, logits, ctx

    def stage_encoder(dt):
        enc = models[dt][0]
        return lambda: enc.encode_packed(waves)

    def stage_prefill(dt):
        llm = models[dt][1]
        x = x_pre.to(dev, dt)
        return lambda: prefill(llm, x, args.prefill_batch)

    def stage_decode_step(dt):
        llm = models[dt][1]
        B = args.decode_rows
        kv, ws, logits, ctx = prefill(llm, x_dec.to(dev, dt), B)
        nid = torch.full((B,), 11, dtype=torch.int32, device=dev)
        ctx0 = ctx.clone()
        w = llm._dev()

        def step():
            ctx.copy_(ctx0)          # the same position every time: equal work per call
            L.check(lib.sl_llama_decode_step(C.byref(w.struct), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                             ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
        return step

    x1 = x_pre[:S][None]

    def stage_b1_token(dt):
        llm = models[dt][1]
        x = x1.to(dev, dt)

        def run():
            t_long = timed(lambda: llm.generate(inputs_embeds=x, max_new_tokens=args.new_tokens + 1))
            t_short = timed(lambda: llm.generate(inputs_embeds=x, max_new_tokens=1))
            run.per_token = (t_long - t_short) / args.new_tokens
        return run

    def stage_one_utterance(dt):
        enc, llm = models[dt]
        emb = llm.model.embed_tokens
        pe, se = emb(prefix.to(dev)), emb(suffix.to(dev))[:, 1:]

        def run():
            audio = enc(waves[0][None].to(dev))
            llm.generate(inputs_embeds=torch.cat([pe, audio, se], dim=1), max_new_tokens=args.new_tokens)
        return run

    stages = [("encoder pass, %d x 10 s" % args.enc_batch, stage_encoder), ("configs[1] prefill, %d x %d tokens" % (args.prefill_batch, S), stage_prefill),
              ("decode step, %d rows" % args.decode_rows, stage_decode_step), ("batch-1 decode, per token", stage_b1_token),
              ("generate_audio_response, one utterance, %d tokens" % args.new_tokens, stage_one_utterance)]
    print(f"# tools/bench_fp16.py --reps {args.reps}: medians of {args.reps} alternating runs per dtype, same random weights and inputs")
    print(f"{'stage':58s} {'bf16 ms':>10s} {'fp16 ms':>10s} {'fp16/bf16':>10s}")
    for name, make in stages:
        fns = {dt: make(dt) for dt in models}
        times = {dt: [] for dt in models}
        for rep in range(args.reps + 1):
            for dt in models:
                fn = fns[dt]
                if getattr(fn, "__name__", "") == "run" and name.startswith("batch-1"):
                    fn()
                    t = fn.per_token
                else:
                    t = timed(fn)
                if rep > 0:      # the first round is the warm-up (graph capture, workspace allocation)
                    times[dt].append(t)
        mb, mh = (statistics.median(times[dt]) * 1e3 for dt in (torch.bfloat16, torch.float16))
        print(f"{name:58s} {mb:10.3f} {mh:10.3f} {mh / mb:10.3f}", flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
