"""fp8 (e4m3) decode weights against the 16-bit packed decode weights, in one process, alternating, on the same random weights and
inputs (Llama-3.2-3B shapes, bf16, random init), for the batches the e4m3 skinny kernels take: B = 1, 4, 16, 26.

Measured per batch and format: each of the five decode products alone (qkv + RoPE / append, o, gate/up + SiLU-mul, down, lm_head: us
per launch, bytes of weights read, fraction of 8 TB/s), and the decode step inside a whole generate call (captured graph: ms per
step, tokens per second).  Recorded, not asserted: the relative distance of one decode step's logits between the two formats on
the same cache, and the share of greedy ids that agree over 64 new tokens (random weights have no margin between the top logits,
so this bounds nothing about a trained checkpoint).

    python tools/bench_w8.py [--reps 5] [--out profiles/w8_vs_16bit.txt]

The report goes to stdout and, with --out, to that file as well (profiles/w8_vs_16bit.txt is the committed run).
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
FORMATS = ("16bit", "e4m3")
HBM = 8.0e12


def mod(name):
    return importlib.import_module(PKG + "." + name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 4, 16, 26])
    ap.add_argument("--prompt", type=int, default=137)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/w8_vs_16bit.txt)")
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
    H, D, nh, nkv, Fd, V = larch.hidden_size, larch.head_dim, larch.num_attention_heads, larch.num_key_value_heads, larch.intermediate_size, larch.vocab_size
    print(f"# tools/bench_w8.py --reps {args.reps}: medians of {args.reps} alternating runs per decode-weight format after one warm-up round; "
          f"{larch.num_hidden_layers} layers, bf16, random init, {S}-token prompts, {new} new tokens, max_ctx {max_ctx}; sl_w8_max_rows() = {lib.sl_w8_max_rows()}; "
          f"device {torch.cuda.get_device_name(0)}")

    # ---- 1. the five decode products alone, as the decode step calls them
    gen = torch.Generator().manual_seed(3)
    cos, sin = [t.to(dev) for t in weights.rope_tables(larch, max_ctx)]
    shapes = dict(qkv=((nh + 2 * nkv) * D, H), o=(H, nh * D), gu=(2 * Fd, H), down=(H, Fd), lm_head=(V, H))
    packed = {}
    for name, (N, K) in shapes.items():
        w = (torch.randn(N, K, generator=gen) * K ** -0.5).to(dev, dt)
        packed[name] = {"16bit": ops.pack_weight(w), "e4m3": ops.pack_weight_e4m3(w)}
        del w
    print(f"\n## decode products alone (us per launch, {args.launches} launches per timing; bytes = the weights read; fraction of {HBM / 1e12:.0f} TB/s)")
    print(f"{'B':>3s} {'product':>8s} {'N':>7s} {'K':>6s} {'16-bit us':>10s} {'16-bit MB':>10s} {'frac':>6s} {'e4m3 us':>9s} {'e4m3 MB':>9s} {'frac':>6s} {'e4m3/16-bit':>12s}")
    for B in args.rows:
        kc = torch.zeros(B, nkv, max_ctx, D, device=dev, dtype=dt)
        vc = torch.zeros_like(kc)
        rope = dict(cos=cos, sin=sin, pos=torch.full((B,), S, dtype=torch.int32, device=dev), seq=torch.arange(B, dtype=torch.int32, device=dev),
                    k_cache=kc, v_cache=vc, n_heads=nh, n_kv=nkv, max_ctx=max_ctx)
        for name, (N, K) in shapes.items():
            x = (torch.randn(B, K, generator=gen) * 0.5).to(dev, dt)
            res = torch.zeros(B, N, device=dev, dtype=dt) if name in ("o", "down") else None
            n_out = nh * D if name == "qkv" else (N // 2 if name == "gu" else N)
            out = torch.empty(B, n_out, device=dev, dtype=torch.float32 if name == "lm_head" else dt)
            kw = dict(qkv=dict(act=L.ACT_ROPE_KV, fuse_rms=True, rope=rope), o=dict(residual=res), gu=dict(act=L.ACT_SILU_MUL, fuse_rms=True),
                      down=dict(residual=res), lm_head=dict(out_f32=True, fuse_rms=True))[name]
            runs = {"16bit": lambda: ops.gemm_decode(x, packed[name]["16bit"], N, out=out, split_k=False, **kw),
                    "e4m3": lambda: ops.gemm_decode(x, packed[name]["e4m3"], N, out=out, split_k=False, w_layout=L.W_PACKED_E4M3, **kw)}
            times = {f: [] for f in FORMATS}
            for rep in range(args.reps + 1):
                for f in FORMATS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        runs[f]()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep > 0:
                        times[f].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            a, b = (statistics.median(times[f]) for f in FORMATS)
            by16, by8 = 2.0 * N * K, float(lib.sl_w8_image_bytes(N, K))
            print(f"{B:3d} {name:>8s} {N:7d} {K:6d} {a:10.1f} {by16 / 1e6:10.1f} {by16 / (a * 1e-6) / HBM:6.2f} {b:9.1f} {by8 / 1e6:9.1f} {by8 / (b * 1e-6) / HBM:6.2f} {b / a:12.3f}",
                  flush=True)
        del kc, vc
    del packed
    torch.cuda.empty_cache()

    # ---- 2. the model: one instance, both structs on the same weights
    bench = importlib.import_module("bench")
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx, max_batch=max(args.rows), weight_dtype="fp8")
    del llm_sd
    llm.generation_config.eos_token_id = None
    w = llm._dev()
    structs = {"16bit": w.struct, "e4m3": w.struct_e4m3}
    print(f"\n## the model: weights read per token {w.weight_bytes_per_token() / 1e9:.3f} GB (16-bit) / {w.weight_bytes_per_token('fp8') / 1e9:.3f} GB (e4m3 images, scales included)")
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, H, generator=gen) * 0.05).to(dev, dt)
    for B in args.rows:
        x = x_all[:B * S]
        # one decode step of either struct on the cache of the same prefill
        cu = (C.c_int32 * (B + 1))(*[S * b for b in range(B + 1)])
        kv = llm._kv_cache(B, 0)
        ws = llm._workspace(lib.sl_generate_workspace_bytes(C.byref(w.struct), x.shape[0], B, 1))
        logits = torch.empty((B, V), device=dev, dtype=torch.float32)
        ctx = torch.empty(B, device=dev, dtype=torch.int32)
        xin = x.clone()
        L.check(lib.sl_llama_prefill(C.byref(w.struct), C.byref(kv), xin.data_ptr(), cu, B, logits.data_ptr(), ctx.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                     L.stream_ptr()), "sl_llama_prefill")
        nid = logits.argmax(-1).to(torch.int32)
        ctx0 = ctx.clone()
        first = {}
        for f in FORMATS:
            ctx.copy_(ctx0)
            L.check(lib.sl_llama_decode_step(C.byref(structs[f]), C.byref(kv), nid.data_ptr(), ctx.data_ptr(), B, logits.data_ptr(), ws.data_ptr(), ws.numel(),
                                             L.stream_ptr()), "sl_llama_decode_step")
            torch.cuda.synchronize()
            first[f] = logits.clone()
        d = (first["e4m3"] - first["16bit"]).norm(dim=-1) / first["16bit"].norm(dim=-1)
        same = (first["e4m3"].argmax(-1) == first["16bit"].argmax(-1)).float().mean()
        # the whole generate call (prefill + new - 1 captured decode steps)
        res, ids = {f: [] for f in FORMATS}, {}
        for rep in range(args.reps + 1):
            for f in FORMATS:
                llm.set_weight_dtype("fp8" if f == "e4m3" else None)
                out, _ = llm.generate_packed(x.clone(), [S] * B, new, use_eos=False)
                torch.cuda.synchronize()
                assert llm.last_generate_stats["weight_format"] == ("e4m3" if f == "e4m3" else "16-bit")
                if rep > 0:
                    res[f].append(llm.last_timings_ms[1])
                ids[f] = out
        a, b = (statistics.median(res[f]) / (new - 1) for f in FORMATS)
        n_cmp = min(64, new)
        agree = (ids["e4m3"][:, :n_cmp] == ids["16bit"][:, :n_cmp]).float()
        print(f"B={B:3d}  decode step (captured graph): 16-bit {a:.3f} ms = {B / a * 1e3:8.0f} tok/s   e4m3 {b:.3f} ms = {B / b * 1e3:8.0f} tok/s   e4m3/16-bit {b / a:.3f}   "
              f"| step logits rel_err mean {float(d.mean()):.3e} max {float(d.max()):.3e}, argmax equal in {float(same) * 100:.0f} % of rows   "
              f"| greedy ids over {n_cmp} tokens: {float(agree.mean()) * 100:.1f} % agree position-wise", flush=True)


if __name__ == "__main__":
    main()
