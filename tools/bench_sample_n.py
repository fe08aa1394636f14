"""Several sampled answers per prompt: the decode step with the prompt's K / V copied to every row slot
(SL_GEN_GROUP_ATTN=0, the parent's attention kernels) against the grouped attention (=1), alternating in one process, and the
attention launches on their own.  Llama-3.2-3B random-init, 137-row prompts, N = 4 answers, bf16, both K/V formats.
    python tools/bench_sample_n.py [rows ...]        (default 64 256 1024; writes profiles/sample_n_ab.txt)"""
import ctypes as C
import importlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

P = "llm-speech-summarization_amd."
L, ops, weights, llama_mod, utils = [importlib.import_module(P + m) for m in ("_lib", "ops", "weights", "audio_llama", "utils")]
dev = torch.device("cuda:0")
larch = weights.KNOWN_LLAMA[utils.LLAMA_ID]
ROWS = [int(a) for a in sys.argv[1:]] or [64, 256, 1024]
S, NEW, N, ROUNDS = 137, 128, 4, 3
MAX_CTX = ((S + NEW + 63) // 64) * 64
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def switch(v):
    os.environ["SL_GEN_GROUP_ATTN"] = v
    L.lib().sl_tuning_reload()


def med(v):
    return sorted(v)[len(v) // 2]


def step_ab(llm, rows):
    """decode ms per step, copy path and grouped path alternating"""
    nseq = rows // N
    x = (torch.randn(nseq * S, larch.hidden_size, device=dev) * 0.02).to(torch.bfloat16)
    smp = dict(temperature=1.0, top_k=0, top_p=1.0, seed=1)
    t = {"0": [], "1": []}
    for rnd in range(ROUNDS + 1):          # round 0 warms both paths up (graph capture, code objects)
        for sw in ("0", "1"):
            switch(sw)
            llm.generate_packed(x.clone(), [S] * nseq, NEW, use_eos=False, sample=smp, num_return=N)
            assert llm.last_generate_stats["attn_path"] == ("grouped" if sw == "1" else "copy")
            if rnd:
                t[sw].append(llm.last_timings_ms[1] / (NEW - 1))
    return med(t["0"]), med(t["1"]), max(t["0"]) - min(t["0"]), max(t["1"]) - min(t["1"])


def attn_ab(rows, kv_format):
    """us per launch set at mid-generation contexts (prompt + NEW / 2 keys), over enough layers' caches that no layer is re-read out of the
    Infinity Cache: the copy path's attention, both grouped passes, and each pass alone (the other given nothing to do)"""
    nseq, nh, nkv, D = rows // N, larch.num_attention_heads, larch.num_key_value_heads, larch.head_dim
    esz = 1 if kv_format == L.KV_FP8_E4M3 else 2
    slots = nseq + rows
    layer_bytes = 2 * slots * nkv * MAX_CTX * D * esz
    layers = max(2, min(28, (768 << 20) // layer_bytes + 1))
    mk = (lambda: torch.randint(0, 120, (slots, nkv, MAX_CTX, D), dtype=torch.uint8, device=dev)) if esz == 1 else \
         (lambda: (torch.randn(slots, nkv, MAX_CTX, D, device=dev) * 0.5).to(torch.bfloat16))
    kcs, vcs = [mk() for _ in range(layers)], [mk() for _ in range(layers)]
    q = (torch.randn(rows, nh * D, device=dev)).to(torch.bfloat16)
    out = torch.empty_like(q)
    ctx = torch.full((rows,), S + NEW // 2, dtype=torch.int32, device=dev)
    pslot, plen = [b // N for b in range(rows)], [S] * rows
    scale = D ** -0.5
    lib = L.lib()
    _, n_used, recs = ops.attn_group_plan(pslot, plen, nh // nkv)
    groups = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.int32).to(dev)
    no_groups = torch.zeros_like(groups)
    plen_d = torch.tensor(plen, dtype=torch.int32, device=dev)
    ctx_prefix_only = plen_d.clone()
    ws = torch.empty(int(lib.sl_attn_decode_grouped_workspace_bytes(rows, nh)), dtype=torch.uint8, device=dev)
    ws.zero_()
    ws_split = torch.empty(int(lib.sl_attn_decode_workspace_bytes(rows, nh, nkv, MAX_CTX)), dtype=torch.uint8, device=dev)
    slot_elems = nkv * MAX_CTX * D

    def grouped(l, g, c):
        L.check(lib.sl_attn_decode_grouped(q.data_ptr(), q.stride(0), kcs[l].data_ptr(), vcs[l].data_ptr(), out.data_ptr(), ws.data_ptr(), c.data_ptr(),
                                           plen_d.data_ptr(), g.data_ptr(), rows, nseq, nh, nkv, D, MAX_CTX, scale, L.SL_BF16, kv_format, L.stream_ptr()), "grouped")

    def copy(l):
        kc, vc = kcs[l].view(-1)[nseq * slot_elems:], vcs[l].view(-1)[nseq * slot_elems:]
        ops.attn_decode_split_ex(q, q.stride(0), kc, vc, ctx, nh, nkv, D, MAX_CTX, scale, kv_format=kv_format, out=out, ws=ws_split)

    forms = {"copy": copy, "grouped": lambda l: grouped(l, groups, ctx), "prefix pass": lambda l: grouped(l, groups, ctx_prefix_only),
             "tail pass": lambda l: grouped(l, no_groups, ctx)}
    t = {k: [] for k in forms}
    for rnd in range(ROUNDS + 1):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 4 * layers
            e0.record()
            for i in range(reps):
                fn(i % layers)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                t[name].append(e0.elapsed_time(e1) * 1000.0 / reps)
    return {k: med(v) for k, v in t.items()}, n_used, layers


def main():
    say(f"# tools/bench_sample_n.py: Llama-3.2-3B random-init, bf16, {S}-row prompts, N = {N}, {NEW} new tokens; median of {ROUNDS} alternating rounds")
    say("# step: decode ms per step inside generate_packed(num_return=4); attention: us per layer at prompt + 64 keys (each pass alone: the other pass given nothing to do)")
    for kv_name, kv in (("bf16 K/V", None), ("e4m3 K/V", "fp8")):
        llm = llama_mod.AudioLlamaForCausalLM(larch, bench.gpu_llama_state_dict(larch, 0, dev), torch_dtype=torch.bfloat16, device=dev, max_ctx=MAX_CTX,
                                              max_batch=max(ROWS), kv_cache_dtype=kv)
        for rows in ROWS:
            llm._kv = None
            c, g, sc, sg = step_ab(llm, rows)
            say(f"{kv_name} rows={rows:5d} ({rows // N:4d} prompts): step copy {c:8.4f} ms (spread {sc:.4f})  grouped {g:8.4f} ms (spread {sg:.4f})  grouped/copy {g / c:6.3f}")
        del llm
        torch.cuda.empty_cache()
        for rows in ROWS:
            a, n_used, layers = attn_ab(rows, L.kv_format_code(kv))
            say(f"{kv_name} rows={rows:5d}: attention copy {a['copy']:8.2f} us  grouped {a['grouped']:8.2f} us  (prefix pass {a['prefix pass']:7.2f} us over {n_used} records, "
                f"tail pass {a['tail pass']:7.2f} us; {layers} layers' caches in rotation)")
    switch("-1")
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "sample_n_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
