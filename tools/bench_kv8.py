"""fp8 (e4m3) K/V cache against the 16-bit cache, in one process, alternating, on the same random weights and inputs
(Llama-3.2-3B shapes, bf16, 137-token prompts, 256 new tokens: the shape bench.py runs).

Measured per format: the decode attention alone (us per launch at the cache geometry of the batched decode step), one decode
step at 1 024 and at 2 048 rows, a whole generate call (prefill + 255 decode steps; tokens per second), and the bytes of K/V
allocated.  Recorded, not asserted: the relative distance of the first decode step's logits (fp8 cache against 16-bit cache) and how
many of 16 greedy ids agree per sequence, on the full-depth random-init model (random weights have no margin between the top
logits, so this bounds nothing about a trained checkpoint).

    python tools/bench_kv8.py [--reps 5] [--out profiles/kv8_vs_16bit.txt]

The report goes to stdout and, with --out, to that file as well (profiles/kv8_vs_16bit.txt is the committed run).
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
FORMATS = ("16bit", "fp8")


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
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--prompt", type=int, default=137)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--attn-launches", type=int, default=200)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/kv8_vs_16bit.txt)")
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
    lib = L.lib()
    larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
    if args.layers:
        import dataclasses
        larch = dataclasses.replace(larch, num_hidden_layers=args.layers)
    S, new = args.prompt, args.new_tokens
    max_ctx = ((S + new + 8 + 63) // 64) * 64
    dt = torch.bfloat16
    nh, nkv, D = larch.num_attention_heads, larch.num_key_value_heads, larch.head_dim
    print(f"# tools/bench_kv8.py --reps {args.reps}: medians of {args.reps} alternating runs per K/V format after one warm-up round; {larch.num_hidden_layers} layers, "
          f"bf16, random init, {S}-token prompts, {new} new tokens, max_ctx {max_ctx}; device {torch.cuda.get_device_name(0)}")

    # ---- 1. the decode attention alone: (rows, n_kv) blocks over a cache of max_ctx positions, the geometry of one layer of the decode step
    print(f"\n## decode attention, one layer, {nh} heads / {nkv} kv heads, D = {D} (us per launch, {args.attn_launches} launches per timing)")
    print(f"{'rows':>6s} {'keys':>6s} {'16-bit us':>10s} {'fp8 us':>10s} {'fp8/16-bit':>11s} {'16-bit TB/s':>12s} {'fp8 TB/s':>10s}")
    gen = torch.Generator().manual_seed(3)
    for B in args.rows:
        q = (torch.randn(B, nh * D, generator=gen)).to(dev, dt)
        k16 = torch.randn(B, nkv, max_ctx, D, device=dev, dtype=dt)
        v16 = torch.randn(B, nkv, max_ctx, D, device=dev, dtype=dt)
        k8 = k16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        v8 = v16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        ws = torch.zeros(int(lib.sl_attn_decode_workspace_bytes(B, nh, nkv, max_ctx)), dtype=torch.uint8, device=dev)
        out = torch.empty(B, nh * D, device=dev, dtype=dt)
        for keys in (S + new // 2, S + new - 1):
            ctx = torch.full((B,), keys, dtype=torch.int32, device=dev)
            runs = {"16bit": lambda: ops.attn_decode_split_ex(q, q.stride(0), k16, v16, ctx, nh, nkv, D, max_ctx, D ** -0.5, L.KV_MODEL_DTYPE, 0, out=out, ws=ws),
                    "fp8": lambda: ops.attn_decode_split_ex(q, q.stride(0), k8, v8, ctx, nh, nkv, D, max_ctx, D ** -0.5, L.KV_FP8_E4M3, 0, out=out, ws=ws)}
            times = {f: [] for f in FORMATS}
            for rep in range(args.reps + 1):
                for f in FORMATS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.attn_launches):
                        runs[f]()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep > 0:
                        times[f].append(e0.elapsed_time(e1) * 1e3 / args.attn_launches)
            a, b = (statistics.median(times[f]) for f in FORMATS)
            byts = 2.0 * B * nkv * keys * D          # K and V elements read
            print(f"{B:6d} {keys:6d} {a:10.1f} {b:10.1f} {b / a:11.3f} {2 * byts / a / 1e6:12.2f} {byts / b / 1e6:10.2f}", flush=True)
        del q, k16, v16, k8, v8, ws, out
        torch.cuda.empty_cache()

    # ---- 2. the model: one instance per format on the same weights
    bench = importlib.import_module("bench")
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)
    models = {}
    for f in FORMATS:
        llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx, max_batch=max(args.rows),
                                              kv_cache_dtype="fp8" if f == "fp8" else None)
        llm.generation_config.eos_token_id = None
        models[f] = llm
    del llm_sd
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, larch.hidden_size, generator=gen) * 0.05).to(dev, dt)

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

    for B in args.rows:
        x = x_all[:B * S]
        print(f"\n## {B} rows")
        # decode step at the first new position (context S + 1), the same position every call
        steps, first_logits = {}, {}
        for f in FORMATS:
            llm = models[f]
            kv, ws, logits, ctx = prefill(llm, x.clone(), B)
            nid = logits.argmax(-1).to(torch.int32)          # the prefill's own greedy token (prefill logits are the same in both formats)
            ctx0 = ctx.clone()
            w = llm._dev()

            def step(llm=llm, kv=kv, ws=ws, logits=logits, ctx=ctx, ctx0=ctx0, nid=nid, w=w):
                ctx.copy_(ctx0)
                L.check(lib.sl_llama_decode_step(C.byref(w.struct), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), L.stream_ptr()), "sl_llama_decode_step")
            step()
            torch.cuda.synchronize()
            first_logits[f] = logits.clone()
            steps[f] = step
        times = {f: [] for f in FORMATS}
        for rep in range(args.reps + 1):
            for f in FORMATS:
                t = timed(steps[f])
                if rep > 0:
                    times[f].append(t)
        a, b = (statistics.median(times[f]) * 1e3 for f in FORMATS)
        print(f"decode step, context {S + 1} (un-captured launches): 16-bit {a:.3f} ms   fp8 {b:.3f} ms   fp8/16-bit {b / a:.3f}")
        d = (first_logits["fp8"] - first_logits["16bit"]).norm(dim=-1) / first_logits["16bit"].norm(dim=-1)
        same = (first_logits["fp8"].argmax(-1) == first_logits["16bit"].argmax(-1)).float().mean()
        print(f"first decode step's logits, fp8 cache against 16-bit cache: relative distance mean {float(d.mean()):.3e} max {float(d.max()):.3e}; "
              f"argmax equal in {float(same) * 100:.1f} % of rows")
        del steps, first_logits
        # the whole generate call (prefill + new - 1 captured decode steps)
        res = {f: [] for f in FORMATS}
        ids = {}
        for rep in range(args.reps + 1):
            for f in FORMATS:
                llm = models[f]
                out, _ = llm.generate_packed(x.clone(), [S] * B, new, use_eos=False)
                torch.cuda.synchronize()
                if rep > 0:
                    res[f].append(llm.last_timings_ms)
                ids[f] = out
        for f in FORMATS:
            pre = statistics.median(r[0] for r in res[f])
            dec = statistics.median(r[1] for r in res[f])
            k, v = models[f]._kv
            print(f"generate {f:>5s}: prefill {pre:8.1f} ms  decode {dec:8.1f} ms ({dec / (new - 1):.3f} ms per step)  "
                  f"{B * new / (pre + dec) * 1e3:9.0f} tok/s end to end, {B * (new - 1) / dec * 1e3:9.0f} tok/s decode  "
                  f"K+V allocated {(k.numel() * k.element_size() + v.numel() * v.element_size()) / 1e9:.2f} GB ({k.shape[1]} slots x {k.shape[3]} positions, {k.dtype})")
        a, b = (statistics.median(r[1] for r in res[f]) for f in FORMATS)
        print(f"decode ms fp8/16-bit {b / a:.3f}")
        agree = (ids["fp8"][:, :16] == ids["16bit"][:, :16]).float()
        lead = (agree.cumprod(dim=1)).sum(dim=1)
        print(f"greedy ids, first 16 of each sequence: {float(agree.sum(1).mean()):.2f} of 16 agree position-wise on average (min {int(agree.sum(1).min())}); "
              f"{float(lead.mean()):.2f} leading ids agree on average; {int((agree.sum(1) == 16).sum())} of {B} sequences agree on all 16")
        for f in FORMATS:
            models[f]._kv = None
            models[f]._ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
