"""Encoder head forward + backward (final LayerNorm -> downsample -> projection and back) for the three downsample methods, on 16 x 10 s of
HuBERT-large frames (16 x 499 frames, H = 1024, llm_dim = 3072) in bf16 — training.EncoderTape._head_forward / _head_backward, i.e. exactly what a
KD window runs.  ctc_pool ranges come from the reference's preprocessing recipe (word chunks of 4 frames + one range per gap) over synthetic word
offsets, one utterance in four with a silence of a few hundred frames.  Writes profiles/downsample.txt.

The yardstick is the `pool` head at the same frame count (its code is the parent commit's, launch for launch): all three heads read the same
NT x H frames once.  Each figure is the median of REPS timings of ITERS back-to-back runs after a warm-up; the downsample launches are also timed alone."""
import importlib
import os
import statistics
import sys
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
training = importlib.import_module("llm-speech-summarization_amd.training")
ops = importlib.import_module("llm-speech-summarization_amd.ops")
L = importlib.import_module("llm-speech-summarization_amd._lib")

DEV, DT = "cuda:0", torch.bfloat16
B, T_UTT, H, LLM = 16, 499, 1024, 3072
WARMUP, ITERS, REPS = 5, 20, 7


def word_pool_ranges(words, chunk=4):
    """ranges of one utterance from its (start, end) word offsets, the way the reference's get_hubert_ctc_pool_ranges lays them out"""
    out = [(0, words[0][0])]
    for i, (start, end) in enumerate(words):
        out += [(s, s + chunk) for s in range(start, end, chunk)]
        out.append((end, words[i + 1][0]) if i + 1 < len(words) else (end, end + 2 * chunk))
    return out


def synthetic_words(T, gen, long_gap):
    """word offsets of a T-frame utterance: words of 5 .. 25 frames, gaps of 1 .. 30, optionally one silence of 200 .. 300 frames"""
    words, t = [], int(torch.randint(1, 20, (1,), generator=gen))
    gap_at = int(torch.randint(2, 6, (1,), generator=gen)) if long_gap else -1
    while True:
        n = int(torch.randint(5, 26, (1,), generator=gen))
        if t + n >= T - 8:
            break
        words.append((t, t + n))
        t += n + (int(torch.randint(200, 301, (1,), generator=gen)) if len(words) == gap_at else int(torch.randint(1, 31, (1,), generator=gen)))
    return words


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return statistics.median(us)


def head(method, T, x, ranges):
    f = 4
    K = H * f if method == "stack" else H
    gen = torch.Generator().manual_seed(7)
    t = dict(final_ln_g=torch.ones(H), final_ln_b=torch.zeros(H), proj_w=torch.randn(LLM, K, generator=gen) * 0.02, proj_b=torch.zeros(LLM))
    t = {k: v.to(DEV, DT) for k, v in t.items()}
    enc = SimpleNamespace(downsample_method=method, downsample_factor=f, pool_kernel=8, pool_stride=4, dtype=DT, device=torch.device(DEV),
                          arch=SimpleNamespace(hidden_size=H, layer_norm_eps=1e-5), weights=SimpleNamespace(t=t))
    tape_obj = training.EncoderTape(enc)
    toff = training._offsets(T)
    g = {k: torch.zeros(v.shape, device=DEV, dtype=torch.float32) for k, v in t.items()}
    out, hd = tape_obj._head_forward(x, T, toff, ranges)
    d_out = torch.randn(out.shape, device=DEV).to(DT)
    tape = dict(T=T, toff=toff, x_last=x, **hd)
    fwd = timed(lambda: tape_obj._head_forward(x, T, toff, ranges))
    bwd = timed(lambda: tape_obj._head_backward(tape, d_out, g, lambda names: None))
    return fwd, bwd, out.shape[0], hd


def main():
    gen = torch.Generator().manual_seed(1)
    T = [T_UTT] * B
    NT = sum(T)
    x = torch.randn(NT, H, generator=gen).to(DEV, DT)
    ranges = [word_pool_ranges(synthetic_words(T_UTT, gen, long_gap=(u % 4 == 0))) for u in range(B)]
    lens = [min(e, T_UTT) - s for r in ranges for s, e in r]
    lines = [f"encoder head, {B} x {T_UTT} frames = {NT} x {H} bf16, projection to {LLM}; median of {REPS} x {ITERS} runs, microseconds",
             f"ctc_pool table: {len(lens)} ranges, lengths min {min(lens)} / median {statistics.median(lens):.0f} / max {max(lens)} frames "
             f"(reference recipe over synthetic word offsets)", ""]
    res = {}
    for method in ("pool", "stack", "ctc_pool"):
        fwd, bwd, rows, hd = head(method, T, x, ranges if method == "ctc_pool" else None)
        res[method] = (fwd, bwd, rows, hd)
        lines.append(f"{method:9s} rows {rows:5d}   head forward {fwd:8.1f}   head backward {bwd:8.1f}   sum {fwd + bwd:8.1f}")
    base = res["pool"][0] + res["pool"][1]
    lines += ["", "relative to the pool head (forward + backward): " +
              ", ".join(f"{m} {(res[m][0] + res[m][1]) / base:.2f}x" for m in ("stack", "ctc_pool")), "", "the downsample launches alone:"]
    # the launches alone (tables already on the device)
    pooled_p, P = ops.avgpool_batch(x, T, 8, 4)
    poff, toff = training._offsets(P), training._offsets(T)
    lines.append(f"  pool      forward {timed(lambda: ops.avgpool_batch(x, T, 8, 4)):7.1f}   backward "
                 f"{timed(lambda: ops.avgpool_bwd_batch(pooled_p, torch.empty_like(x), P, T, poff[:-1], toff[:-1], 8, 4)):7.1f}   (with their descriptor uploads)")
    st, _ = ops.stack_rows_batch(x, T, 4)
    lines.append(f"  stack     forward {timed(lambda: ops.stack_rows_batch(x, T, 4)):7.1f}   backward {timed(lambda: ops.stack_rows_bwd_batch(st, T, 4)):7.1f}   "
                 f"(with their descriptor uploads)")
    seg = res["ctc_pool"][3]["seg"]
    pooled_c = res["ctc_pool"][3]["pooled"]
    lines.append(f"  ctc_pool  forward {timed(lambda: ops.segment_mean_batch(x, seg[0])):7.1f}   backward "
                 f"{timed(lambda: ops.segment_mean_bwd_batch(pooled_c, *seg, NT)):7.1f}   (tables resident)")
    lines.append(f"  ctc_pool  host tables (clamp + offset, CSR index, three uploads) "
                 f"{timed(lambda: [L.h2d(v, v.dtype, DEV) for v in (lambda p: (p,) + ops.segment_csr(p, NT))(ops.segment_ranges_pack(ranges, T)[0])]):7.1f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "downsample.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
