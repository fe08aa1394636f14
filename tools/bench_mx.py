"""The opt-in MX linears (linear_dtype="mx": MXFP8 activations x MXFP4 weights on the block-scaled MFMA) against the paths the
same process runs without the option, alternating, on the same random weights and inputs (Llama-3.2-3B shapes, bf16, random init).

Product legs: the four layer products at 8 192, 1 024, 256, 64 and 1 rows — the quantise launch + sl_gemm_mx (and the quantise launch
alone) against sl_gemm on the row-major weight (8 192 rows: prefill) or sl_gemm_fused_decode on the packed 16-bit copy with the K split
allowed (the decode rows), plain epilogues on both sides.  Launch i reads copy i % n of its weight, n copies holding at least 768 MB
together, so that no launch finds its weight in the 256 MB last-level cache that the launch before left there.  TF/s counts 2 M N K.
Model legs: prefill of 64 x 137 rows through sl_llama_prefill on both structs, and the captured decode step inside generate at 1 024 /
256 / 26 / 1 rows (at <= 26 rows also weight_dtype="mxfp4").  Reported per cell: the median of the alternating repetitions after one
warm-up round, and their spread.  NOT measured here: a bare loop of the scaled MFMA against the bf16 one.

    python tools/bench_mx.py [--reps 5] [--out profiles/mx_linear.txt]
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
ROTATE_BYTES = 768e6          # three times the 256 MB last-level cache
PEAK_E4M3 = 5.0e15


def mod(name):
    return importlib.import_module(PKG + "." + name)


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def cell(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):7.1f} ..{max(ts):7.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[8192, 1024, 256, 64, 1])
    ap.add_argument("--decode-rows", type=int, nargs="+", default=[1024, 256, 26, 1])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--new-tokens", type=int, default=48)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None, help="also write the report to this file (the committed run: profiles/mx_linear.txt)")
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
    dt = torch.bfloat16
    H, D, nh, nkv, Fd = larch.hidden_size, larch.head_dim, larch.num_attention_heads, larch.num_key_value_heads, larch.intermediate_size
    print(f"# tools/bench_mx.py --reps {args.reps}: medians (min .. max) of {args.reps} alternating runs after one warm-up round; {larch.num_hidden_layers} layers, bf16, "
          f"random init; device {torch.cuda.get_device_name(0)}")

    # ---- the four products alone
    gen = torch.Generator().manual_seed(3)
    shapes = dict(qkv=((nh + 2 * nkv) * D, H), o=(H, nh * D), gu=(2 * Fd, H), down=(H, Fd))
    print(f"\n## products alone (us per call; {args.launches} calls per timing over rotating weight copies; baseline: sl_gemm row-major at 8 192 rows, "
          f"sl_gemm_fused_decode on the packed 16-bit copy below; frac = MX TF/s of the {PEAK_E4M3 / 1e15:.0f} PF e4m3 peak)")
    print(f"{'rows':>5s} {'product':>7s} {'N':>6s} {'K':>5s} {'baseline us':>28s} {'quantise us':>28s} {'quantise + MX us':>28s} {'base TF/s':>9s} {'MX TF/s':>8s} {'frac':>6s} {'MX/base':>8s}")
    for name, (N, K) in shapes.items():
        wt = (torch.randn(N, K, generator=gen) * K ** -0.5).to(dev, dt)
        act = L.ACT_SILU_MUL if name == "gu" else L.ACT_NONE
        n16 = max(2, int(-(-ROTATE_BYTES // (2.0 * N * K))))
        nmx = max(2, int(-(-ROTATE_BYTES // float(lib.sl_mx_weight_image_bytes(N, K)))))
        rowmajor = [wt] + [wt.clone() for _ in range(n16 - 1)]
        packed = [ops.pack_weight(wt) for _ in range(n16)]
        imgs = [ops.pack_weight_mx(wt) for _ in range(nmx)]
        for M in args.rows:
            x = (torch.randn(M, K, generator=gen) * 0.5).to(dev, dt)
            res = torch.zeros(M, N, device=dev, dtype=dt) if name in ("o", "down") else None
            out = torch.empty(M, N // 2 if name == "gu" else N, device=dev, dtype=dt)
            q = torch.empty(M, K, device=dev, dtype=torch.uint8)
            s = torch.empty(M, K // 32, device=dev, dtype=torch.uint8)
            if M > 2048:
                base = lambda i: ops.gemm(x, rowmajor[i % n16], residual=res, act=act, out=out)
            else:
                base = lambda i: ops.gemm_decode(x, packed[i % n16], N, residual=res, act=act, out=out)

            def quant(i):
                ops.mxfp8_quantize_rows(x, out=(q, s))

            def mx(i):
                ops.mxfp8_quantize_rows(x, out=(q, s))
                ops.gemm_mx(q, s, imgs[i % nmx], N, dtype=dt, act=act, residual=res, out=out)
            tb, tq, tm = [], [], []
            for rep in range(args.reps + 1):
                for ts, fn in ((tb, base), (tq, quant), (tm, mx)):
                    t = timed(fn, args.launches)
                    if rep > 0:
                        ts.append(t)
            fl = 2.0 * M * N * K
            mb, mm = statistics.median(tb), statistics.median(tm)
            print(f"{M:5d} {name:>7s} {N:6d} {K:5d} {cell(tb)} {cell(tq)} {cell(tm)} {fl / mb / 1e6:9.1f} {fl / mm / 1e6:8.1f} {fl / (mm * 1e-6) / PEAK_E4M3:6.3f} {mm / mb:8.3f}",
                  flush=True)
        del rowmajor, packed, imgs, wt
        torch.cuda.empty_cache()

    # ---- the model: one instance, the structs on the same weights
    bench = importlib.import_module("bench")
    S, new = 137, args.new_tokens
    max_ctx = ((S + new + 8 + 63) // 64) * 64
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)
    llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx, max_batch=max(args.decode_rows), linear_dtype="mx")
    del llm_sd
    llm.generation_config.eos_token_id = None
    w = llm._dev()
    gen = torch.Generator().manual_seed(5)
    # (c) prefill of 64 x 137 rows
    B = 64
    x = (torch.randn(B * S, H, generator=gen) * 0.05).to(dev, dt)
    cu = (C.c_int32 * (B + 1))(*[S * b for b in range(B + 1)])
    logits = torch.empty((B, larch.vocab_size), device=dev, dtype=torch.float32)
    ctx = torch.empty(B, device=dev, dtype=torch.int32)
    res = {"16-bit": [], "mx": []}
    for rep in range(args.reps + 1):
        for name, struct, opt in (("16-bit", w.struct, None), ("mx", w.struct_mx, "mx")):
            llm.set_linear_dtype(opt)
            kv = llm._kv_cache(B, 0)
            ws = llm._workspace(lib.sl_llama_workspace_bytes(C.byref(struct), B * S, B))

            def run(i):
                xin = x.clone()
                L.check(lib.sl_llama_prefill(C.byref(struct), C.byref(kv), xin.data_ptr(), cu, B, logits.data_ptr(), ctx.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                             L.stream_ptr()), "sl_llama_prefill")
            t = timed(run, 3)
            if rep > 0:
                res[name].append(t / 1e3)
    m16, mmx = statistics.median(res["16-bit"]), statistics.median(res["mx"])
    print(f"\n## the model\nprefill 64 x 137 rows (ms, host set-up and the copy of x included): 16-bit {m16:.2f} ({min(res['16-bit']):.2f} .. {max(res['16-bit']):.2f})   "
          f"mx {mmx:.2f} ({min(res['mx']):.2f} .. {max(res['mx']):.2f})   mx/16-bit {mmx / m16:.3f}", flush=True)
    # (d) the captured decode step
    for B in args.decode_rows:
        x = (torch.randn(B * S, H, generator=gen) * 0.05).to(dev, dt)
        forms = [("16-bit", None, None), ("mx", "mx", None)] + ([("mxfp4", None, "mxfp4")] if B <= lib.sl_w4_max_rows() else [])
        res = {f[0]: [] for f in forms}
        for rep in range(args.reps + 1):
            for name, lin, wd in forms:
                llm.set_linear_dtype(None)
                llm.set_weight_dtype(wd)
                llm.set_linear_dtype(lin)
                llm.generate_packed(x.clone(), [S] * B, new, use_eos=False)
                torch.cuda.synchronize()
                assert llm.last_generate_stats["weight_format"] == name, llm.last_generate_stats["weight_format"]
                if rep > 0:
                    res[name].append(llm.last_timings_ms[1] / (new - 1))
        llm.set_linear_dtype(None)
        llm.set_weight_dtype(None)
        med = {k: statistics.median(v) for k, v in res.items()}
        cells = "   ".join(f"{k} {med[k]:.3f} ms ({min(v):.3f} .. {max(v):.3f}) = {B / med[k] * 1e3:8.0f} tok/s" for k, v in res.items())
        ratios = f"mx/16-bit {med['mx'] / med['16-bit']:.3f}" + (f"  mx/mxfp4 {med['mx'] / med['mxfp4']:.3f}" if "mxfp4" in med else "")
        print(f"B={B:4d}  decode step (captured graph): {cells}   {ratios}", flush=True)


if __name__ == "__main__":
    main()
