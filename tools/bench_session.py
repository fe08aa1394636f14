"""A follow-up question on a kept K/V cache against today's alternative, a re-prefill of everything (Llama-3.2-3B shapes, bf16, random weights).

Workload: 1 024 / 64 / 1 sequences hold 393 cache positions (a 137-row audio prompt and a 256-token answer) and are asked a 16-row follow-up,
on the 16-bit and on the e4m3 cache.
  (a) the continued call: sl_generate_cont, 16 new prompt rows on the 393-position past (generate_packed(session=));
  (b) the alternative without a session: sl_generate_sc over the concatenated 409-row prompt with compact = 0.
Both generate the same number of new tokens; prefill and decode are reported apart (the library's own events).  Also: the new attention
kernel alone (sl_attn_fwd_past, one layer, both formats) against sl_attn_fwd on a 16-bit cache of the same lengths.  The past holds random
K/V (timing only: random weights give no meaningful text either way).

    python tools/bench_session.py [--reps 5] [--out profiles/session.txt]

Medians of --reps alternating runs after one warm-up round, all in one process on one device."""
import argparse
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "llm-speech-summarization_amd"
PAST, ROWS = 393, 16


def mod(name):
    return importlib.import_module(PKG + "." + name)


def fill(t, fp8):
    """random K/V into a cache tensor, layer by layer (e4m3: finite bytes only)"""
    for l in range(t.shape[0]):
        r = torch.randn(t.shape[1:], device=t.device, dtype=torch.bfloat16)
        t[l] = r.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8) if fp8 else r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 64, 1])
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--attn-launches", type=int, default=50)
    ap.add_argument("--layers", type=int, default=0, help="override the depth (0 = the real 28 layers); for a quick dry run")
    ap.add_argument("--out", default=None)
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
    new = args.new_tokens
    max_ctx = ((PAST + ROWS + new + 63) // 64) * 64
    dt = torch.bfloat16
    nh, nkv, D = larch.num_attention_heads, larch.num_key_value_heads, larch.head_dim
    clocks = "left to the device's own management (not pinned, not read): the variants alternate inside every round, so they share its state"
    print(f"# tools/bench_session.py --reps {args.reps}: medians of {args.reps} alternating runs after one warm-up round; {larch.num_hidden_layers} layers, bf16, "
          f"random init, past {PAST}, {ROWS} new prompt rows, {new} new tokens, max_ctx {max_ctx}; device {torch.cuda.get_device_name(0)}; clocks: {clocks}")

    # ---- 1. the attention kernel alone, one layer
    print(f"\n## prefill attention of the continued rows, one layer, {nh} heads / {nkv} kv heads, D = {D}: past {PAST} + {ROWS} new keys (us per launch)")
    print(f"{'seqs':>6s} {'attn_fwd 16-bit':>16s} {'past 16-bit':>12s} {'past e4m3':>10s} {'e4m3/16-bit':>12s}")
    for B in args.rows:
        q = torch.randn(B * ROWS, (nh + 2 * nkv) * D, device=dev, dtype=dt)
        k16 = torch.randn(B, nkv, max_ctx, D, device=dev, dtype=dt)
        v16 = torch.randn(B, nkv, max_ctx, D, device=dev, dtype=dt)
        k8 = k16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        v8 = v16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        out = torch.empty(B * ROWS, nh * D, device=dev, dtype=dt)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * ROWS
        row0 = torch.arange(B, dtype=torch.int32, device=dev) * (nkv * max_ctx)
        past = torch.full((B,), PAST, dtype=torch.int32, device=dev)
        klen_new = torch.full((B,), ROWS, dtype=torch.int32, device=dev)
        klen_all = past + klen_new
        qw = (nh + 2 * nkv) * D
        kn, vn = q[:, nh * D:], q[:, (nh + nkv) * D:]
        common = dict(q_strides=(qw, D), o_strides=(nh * D, D), nseq=B, max_qlen=ROWS, n_heads=nh, n_kv_heads=nkv, head_dim=D, scale=D ** -0.5)
        runs = {
            "fwd16": lambda: ops.attn_fwd(q, k16, v16, out, cu, row0, klen_all, k_strides=(D, max_ctx * D), v_strides=(D, max_ctx * D), causal=True, **common),
            "past16": lambda: ops.attn_fwd_past(q, kn, vn, out, cu, cu, klen_new, k16, v16, past, row0, k_strides=(qw, D), v_strides=(qw, D), max_ctx=max_ctx,
                                                kv_format=L.KV_MODEL_DTYPE, **common),
            "past8": lambda: ops.attn_fwd_past(q, kn, vn, out, cu, cu, klen_new, k8, v8, past, row0, k_strides=(qw, D), v_strides=(qw, D), max_ctx=max_ctx,
                                               kv_format=L.KV_FP8_E4M3, **common)}
        times = {f: [] for f in runs}
        for rep in range(args.reps + 1):
            for f, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.attn_launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep > 0:
                    times[f].append(e0.elapsed_time(e1) * 1e3 / args.attn_launches)
        a, b, c = (statistics.median(times[f]) for f in ("fwd16", "past16", "past8"))
        print(f"{B:6d} {a:16.1f} {b:12.1f} {c:10.1f} {c / b:12.3f}", flush=True)
        del q, k16, v16, k8, v8, out
        torch.cuda.empty_cache()

    # ---- 2. the follow-up turn, per cache format
    bench = importlib.import_module("bench")
    llm_sd = bench.gpu_llama_state_dict(larch, 0, dev)
    gen = torch.Generator().manual_seed(5)
    Bmax = max(args.rows)
    x_all = (torch.randn(Bmax * (PAST + ROWS), larch.hidden_size, generator=gen) * 0.05).to(dev, dt)
    print(f"\n## the follow-up turn: (a) sl_generate_cont, {ROWS} rows on a {PAST}-position past; (b) sl_generate_sc over the {PAST + ROWS}-row prompt, compact = 0 (ms)")
    print(f"{'cache':>6s} {'seqs':>6s} {'(a) prefill':>12s} {'(a) decode':>11s} {'(a) total':>10s} {'(b) prefill':>12s} {'(b) decode':>11s} {'(b) total':>10s} {'(b)/(a) total':>14s} "
          f"{'(b)/(a) prefill':>16s}")
    for fmt in ("16bit", "e4m3"):
        llm = llama_mod.AudioLlamaForCausalLM(larch, dict(llm_sd), torch_dtype=dt, device=dev, max_ctx=max_ctx, max_batch=Bmax,
                                              kv_cache_dtype="fp8" if fmt == "e4m3" else None)
        llm.generation_config.eos_token_id = None
        for B in args.rows:
            sess = llm.new_session(B)
            fill(sess.k, fmt == "e4m3"); fill(sess.v, fmt == "e4m3")
            xa = x_all[:B * ROWS]
            xb = x_all[:B * (PAST + ROWS)]

            def run_a():
                sess.valid_len, sess.pending_id = [PAST] * B, [None] * B
                llm.generate_packed(xa.clone(), [ROWS] * B, new, use_eos=False, session=sess)
                return llm.last_timings_ms

            def run_b():
                llm.generate_packed(xb.clone(), [PAST + ROWS] * B, new, use_eos=False, compact=False)
                return llm.last_timings_ms
            res = {"a": [], "b": []}
            for rep in range(args.reps + 1):
                for name, fn in (("a", run_a), ("b", run_b)):
                    t = fn()
                    torch.cuda.synchronize()
                    if rep > 0:
                        res[name].append(t)
            pa, da = (statistics.median(r[i] for r in res["a"]) for i in (0, 1))
            pb, db = (statistics.median(r[i] for r in res["b"]) for i in (0, 1))
            print(f"{fmt:>6s} {B:6d} {pa:12.2f} {da:11.2f} {pa + da:10.2f} {pb:12.2f} {db:11.2f} {pb + db:10.2f} {(pb + db) / (pa + da):14.2f} {pb / pa:16.2f}", flush=True)
            del sess
            llm._kv = None
            torch.cuda.empty_cache()
        del llm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
