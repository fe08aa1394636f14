"""MXFP4 decode weights against the e4m3 weight images and the 16-bit packed decode weights, in one process, alternating, on the same
random weights and inputs (Llama-3.2-3B shapes, bf16, random init), for the batches the skinny kernels take: B = 1, 4, 16, 26.  The
16-bit and e4m3 kernels are the yardstick: this work does not change them.

Measured per batch and format: each of the five decode products alone (qkv + RoPE / append, o, gate/up + SiLU-mul, down, lm_head: us
per launch, bytes of weights read, fraction of 8 TB/s), and the decode step inside a whole generate call (captured graph: ms per
step, tokens per second).  Every product is timed with events around many launches, and launch i reads copy i % n of its weight,
n copies holding at least 768 MB together, so that no launch finds its weights in the 256 MB last-level cache that the launch before
left there (an MXFP4 gate/up image is 27 MB: one copy would be timed out of the cache).  Reported per cell: the median of the
alternating repetitions after one warm-up round, and their spread (min .. max).  Recorded, not asserted: the relative distance of one
decode step's logits between each quantised format and the 16-bit weights on the same cache (random weights have no margin between
the top logits, so this bounds nothing about a trained checkpoint).

    python tools/bench_w4.py [--reps 5] [--out profiles/w4_vs_16bit.txt]

The report goes to stdout and, with --out, to that file as well (profiles/w4_vs_16bit.txt is the committed run).
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
FORMATS = ("16bit", "e4m3", "mxfp4")
HBM = 8.0e12
ROTATE_BYTES = 768e6          # three times the 256 MB last-level cache


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
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/w4_vs_16bit.txt)")
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
    print(f"# tools/bench_w4.py --reps {args.reps}: medians (min .. max) of {args.reps} alternating runs per decode-weight format after one warm-up round; "
          f"{larch.num_hidden_layers} layers, bf16, random init, {S}-token prompts, {new} new tokens, max_ctx {max_ctx}; sl_w4_max_rows() = {lib.sl_w4_max_rows()}; "
          f"device {torch.cuda.get_device_name(0)}")

    # ---- 1. the five decode products alone, as the decode step calls them
    gen = torch.Generator().manual_seed(3)
    cos, sin = [t.to(dev) for t in weights.rope_tables(larch, max_ctx)]
    shapes = dict(qkv=((nh + 2 * nkv) * D, H), o=(H, nh * D), gu=(2 * Fd, H), down=(H, Fd), lm_head=(V, H))
    layouts = {"16bit": L.W_PACKED, "e4m3": L.W_PACKED_E4M3, "mxfp4": L.W_PACKED_MXFP4}
    nbytes = {"16bit": lambda N, K: 2.0 * N * K, "e4m3": lambda N, K: float(lib.sl_w8_image_bytes(N, K)), "mxfp4": lambda N, K: float(lib.sl_w4_image_bytes(N, K))}
    print(f"\n## decode products alone (us per launch: median (min .. max); {args.launches} launches per timing over rotating copies of the weight; MB = the weights "
          f"one launch reads; frac = of {HBM / 1e12:.0f} TB/s at the median; "
          f"* = the host needed at least 0.9 of that time to enqueue the launches: the cell measures the launch rate, not the kernel)")
    print(f"{'B':>3s} {'product':>8s} {'N':>7s} {'K':>6s} " + " ".join(f"{f + ' us':>24s} {'MB':>7s} {'frac':>5s}" for f in FORMATS) + f" {'e4m3/16':>8s} {'fp4/16':>7s} {'fp4/e4m3':>9s}")
    for name, (N, K) in shapes.items():
        w = (torch.randn(N, K, generator=gen) * K ** -0.5).to(dev, dt)
        one = {"16bit": ops.pack_weight(w), "e4m3": ops.pack_weight_e4m3(w), "mxfp4": ops.pack_weight_mxfp4(w)}
        del w
        copies = {}
        for f in FORMATS:
            n = max(2, int(-(-ROTATE_BYTES // nbytes[f](N, K))))
            copies[f] = [one[f]] + [one[f].clone() for _ in range(n - 1)]
        del one
        for B in args.rows:
            kc = torch.zeros(B, nkv, max_ctx, D, device=dev, dtype=dt)
            vc = torch.zeros_like(kc)
            rope = dict(cos=cos, sin=sin, pos=torch.full((B,), S, dtype=torch.int32, device=dev), seq=torch.arange(B, dtype=torch.int32, device=dev),
                        k_cache=kc, v_cache=vc, n_heads=nh, n_kv=nkv, max_ctx=max_ctx)
            x = (torch.randn(B, K, generator=gen) * 0.5).to(dev, dt)
            res = torch.zeros(B, N, device=dev, dtype=dt) if name in ("o", "down") else None
            n_out = nh * D if name == "qkv" else (N // 2 if name == "gu" else N)
            out = torch.empty(B, n_out, device=dev, dtype=torch.float32 if name == "lm_head" else dt)
            kw = dict(qkv=dict(act=L.ACT_ROPE_KV, fuse_rms=True, rope=rope), o=dict(residual=res), gu=dict(act=L.ACT_SILU_MUL, fuse_rms=True),
                      down=dict(residual=res), lm_head=dict(out_f32=True, fuse_rms=True))[name]
            times, host = {f: [] for f in FORMATS}, {f: [] for f in FORMATS}
            for rep in range(args.reps + 1):
                for f in FORMATS:
                    cs = copies[f]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for i in range(args.launches):
                        ops.gemm_decode(x, cs[i % len(cs)], N, out=out, split_k=False, w_layout=layouts[f], **kw)
                    e1.record()
                    t1 = time.perf_counter()      # the host's time to enqueue the launches: a cell it nearly equals is bound by the launch rate
                    torch.cuda.synchronize()
                    if rep > 0:
                        times[f].append(e0.elapsed_time(e1) * 1e3 / args.launches)
                        host[f].append((t1 - t0) * 1e6 / args.launches)
            med = {f: statistics.median(times[f]) for f in FORMATS}
            mark = {f: "*" if statistics.median(host[f]) >= 0.9 * med[f] else " " for f in FORMATS}
            cells = " ".join(f"{med[f]:7.1f}{mark[f]} ({min(times[f]):6.1f} ..{max(times[f]):6.1f}) {nbytes[f](N, K) / 1e6:7.1f} {nbytes[f](N, K) / (med[f] * 1e-6) / HBM:5.2f}" for f in FORMATS)
            print(f"{B:3d} {name:>8s} {N:7d} {K:6d} {cells} {med['e4m3'] / med['16bit']:8.3f} {med['mxfp4'] / med['16bit']:7.3f} {med['mxfp4'] / med['e4m3']:9.3f}", flush=True)
            del kc, vc
        del copies
        torch.cuda.empty_cache()

    # ---- 2. the model: one instance, the three structs on the same weights
    bench = importlib.import_module("bench")
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx, max_batch=max(args.rows), weight_dtype="fp8")
    del llm_sd
    llm.set_weight_dtype("mxfp4")
    llm.generation_config.eos_token_id = None
    w = llm._dev()
    structs = {"16bit": w.struct, "e4m3": w.struct_e4m3, "mxfp4": w.struct_mxfp4}
    option = {"16bit": None, "e4m3": "fp8", "mxfp4": "mxfp4"}
    label = {"16bit": "16-bit", "e4m3": "e4m3", "mxfp4": "mxfp4"}
    print(f"\n## the model: weights read per token {w.weight_bytes_per_token() / 1e9:.3f} GB (16-bit) / {w.weight_bytes_per_token('fp8') / 1e9:.3f} GB (e4m3 images) / "
          f"{w.weight_bytes_per_token('mxfp4') / 1e9:.3f} GB (MXFP4 images), scales included")
    gen = torch.Generator().manual_seed(5)
    x_all = (torch.randn(max(args.rows) * S, H, generator=gen) * 0.05).to(dev, dt)
    for B in args.rows:
        x = x_all[:B * S]
        # one decode step of every struct on the cache of the same prefill
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
        dist = {f: (first[f] - first["16bit"]).norm(dim=-1) / first["16bit"].norm(dim=-1) for f in ("e4m3", "mxfp4")}
        # the whole generate call (prefill + new - 1 captured decode steps)
        res = {f: [] for f in FORMATS}
        for rep in range(args.reps + 1):
            for f in FORMATS:
                llm.set_weight_dtype(option[f])
                llm.generate_packed(x.clone(), [S] * B, new, use_eos=False)
                torch.cuda.synchronize()
                assert llm.last_generate_stats["weight_format"] == label[f]
                if rep > 0:
                    res[f].append(llm.last_timings_ms[1] / (new - 1))
        med = {f: statistics.median(res[f]) for f in FORMATS}
        cells = "   ".join(f"{label[f]} {med[f]:.3f} ms ({min(res[f]):.3f} .. {max(res[f]):.3f}) = {B / med[f] * 1e3:7.0f} tok/s" for f in FORMATS)
        print(f"B={B:3d}  decode step (captured graph): {cells}   e4m3/16-bit {med['e4m3'] / med['16bit']:.3f}  mxfp4/16-bit {med['mxfp4'] / med['16bit']:.3f}  "
              f"mxfp4/e4m3 {med['mxfp4'] / med['e4m3']:.3f}   | step logits rel_err to 16-bit, mean: e4m3 {float(dist['e4m3'].mean()):.3e}  mxfp4 {float(dist['mxfp4'].mean()):.3e}",
              flush=True)


if __name__ == "__main__":
    main()
