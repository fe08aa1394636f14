"""CTC segmentation on 256 x 10 s of HuBERT-large frames (256 x 499 frames, H = 1024, a 32-way CTC head) in bf16.  Writes profiles/ctc_segment.txt.

  * the head kernel (sl_ctc_greedy_batch: lm_head + argmax fused) next to its algorithmic bytes, n_rows x H x 2 (one read of the frames; the
    64 KB weight and the 4 B id per row are left out of the bound);
  * the same ids by the parent commit's means: sl_gemm to fp32 logits, then torch.argmax (the logits written and read back);
  * the segmentation (sl_ctc_pool_ranges_batch, its two launches) on ids with CTC-like statistics, with and without the word table;
  * for comparison only, where `transformers` is present: the host route of the reference's recipe per utterance (ids to the host,
    Wav2Vec2CTCTokenizer.decode(output_word_offsets=True), the Python loop of tests/ctc_segment_ref.py standing in for the reference's).

Each device figure is the median of REPS timings of ITERS back-to-back runs after a warm-up (device events); the ids of the two head routes are
compared before anything is timed.  The frames are 261 MB, more than the 256 MB Infinity Cache, so repeated runs do not read them from cache.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
ops = importlib.import_module("llm-speech-summarization_amd.ops")
L = importlib.import_module("llm-speech-summarization_amd._lib")
import ctc_segment_ref as ref  # noqa: E402

DEV, DT = "cuda:0", torch.bfloat16
B, T_UTT, H, V = 256, 499, 1024, 32
BLANK, DELIM = 0, 4
WARMUP, ITERS = 3, 10


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / ITERS * 1e3)
    return statistics.median(us), min(us), max(us)


def ctc_like_ids(gen):
    """per utterance: runs of blank (most frames), letters repeated 1 .. 3 frames, a delimiter run every 3 .. 9 letters"""
    out = []
    for _ in range(B):
        ids, since = [], 0
        while len(ids) < T_UTT:
            ids += [BLANK] * int(torch.randint(0, 9, (1,), generator=gen))
            if since >= int(torch.randint(3, 10, (1,), generator=gen)):
                ids += [DELIM] * int(torch.randint(1, 3, (1,), generator=gen))
                since = 0
            else:
                ids += [int(torch.randint(5, V, (1,), generator=gen))] * int(torch.randint(1, 4, (1,), generator=gen))
                since += 1
        out.append(ids[:T_UTT])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctc_segment.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ctc_segment.py measures on the MI355X; there is no CPU path"
    gen = torch.Generator().manual_seed(1)
    NT = B * T_UTT
    x = torch.randn(NT, H, generator=gen).to(DEV, DT)
    w = (torch.randn(V, H, generator=gen) * 0.5).to(DEV, DT)
    b = torch.randn(V, generator=gen).to(DEV, DT)

    def gemm_argmax():
        return torch.argmax(ops.gemm(x, w, bias=b, out_f32=True), dim=1)

    ids_k, ids_g = ops.ctc_greedy(x, w, b), gemm_argmax().to(torch.int32)
    differ = int((ids_k != ids_g).sum())          # both accumulate in fp32, in different orders: near-ties may differ
    logits = x.float() @ w.float().T + b.float()
    top = torch.topk(logits, 2, dim=1).values
    near = (top[:, 0] - top[:, 1]) < 1e-3 * top[:, 0].abs().clamp_min(1.0)
    assert not bool(((ids_k.long() != logits.argmax(dim=1)) & ~near).any()), "the fused kernel disagrees with fp32 logits away from near-ties"
    lines = [f"CTC segmentation, {B} x {T_UTT} frames = {NT} x {H} bf16, CTC head {V} x {H}; median (min .. max) of {args.reps} x {ITERS} runs, microseconds", ""]
    nbytes = NT * H * 2
    med, lo, hi = timed(lambda: ops.ctc_greedy(x, w, b), args.reps)
    lines.append(f"sl_ctc_greedy_batch (head + argmax fused)   {med:9.1f} ({lo:.1f} .. {hi:.1f})   algorithmic bytes {nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.2f} TB/s")
    med_g, lo, hi = timed(gemm_argmax, args.reps)
    lines.append(f"sl_gemm to fp32 logits + torch.argmax       {med_g:9.1f} ({lo:.1f} .. {hi:.1f})   {med_g / med:.2f}x the fused kernel; ids that differ: {differ} of {NT}")
    seqs = ctc_like_ids(gen)
    ids = torch.tensor([v for s in seqs for v in s], dtype=torch.int32).to(DEV)
    offs = L.h2d([T_UTT * u for u in range(B + 1)], torch.int64, DEV)
    ranges, counts = ops.ctc_pool_ranges(ids, offs, BLANK, DELIM, 4)
    counts = counts.cpu().tolist()
    want = [ref.packed_ranges(ref.words(s, BLANK, DELIM), T_UTT, 4, T_UTT * u) for u, s in enumerate(seqs)]
    assert [tuple(r) for r in ranges[:sum(counts)].cpu().tolist()] == [r for u in want for r in u] and counts == [len(u) for u in want]
    med, lo, hi = timed(lambda: ops.ctc_pool_ranges(ids, offs, BLANK, DELIM, 4), args.reps)
    lines.append(f"sl_ctc_pool_ranges_batch (count + emit)     {med:9.1f} ({lo:.1f} .. {hi:.1f})   {sum(counts)} ranges of {B} utterances (with its output allocations)")
    med, lo, hi = timed(lambda: ops.ctc_pool_ranges(ids, offs, BLANK, DELIM, 4, want_words=True), args.reps)
    lines.append(f"  ... with the word table                   {med:9.1f} ({lo:.1f} .. {hi:.1f})")
    try:
        from transformers import Wav2Vec2CTCTokenizer
        vocab = ["<pad>", "<s>", "</s>", "<unk>", "|"] + [chr(65 + i) for i in range(V - 5)]
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "vocab.json"), "w") as f:
                json.dump({t_: i for i, t_ in enumerate(vocab)}, f)
            tok = Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), unk_token="<unk>", pad_token="<pad>", bos_token="<s>", eos_token="</s>",
                                       word_delimiter_token="|")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u in range(B):
            row = ids[T_UTT * u:T_UTT * (u + 1)].cpu()
            wo = tok.decode(row, output_word_offsets=True).word_offsets
            ref.raw_ranges([(o["start_offset"], o["end_offset"]) for o in wo], T_UTT, 4)
        host = (time.perf_counter() - t0) * 1e6
        lines.append(f"host route (HF tokenizer + Python loop)     {host:9.1f} for the {B} utterances, {host / B:.1f} per utterance (one run, host clock; comparison only)")
    except ImportError:
        lines.append("host route: transformers is not installed, not measured")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
