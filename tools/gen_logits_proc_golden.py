#!/usr/bin/env python
"""Writes tests/golden/logits_proc_tiny.npz: what the reference class returns (CPU, fp32, HF `generate(inputs_embeds=...)`) with
repetition_penalty / no_repeat_ngram_size / min_new_tokens, and the same prompts with the processors off.

Cases, each on TINY_MHA and TINY_LLAMA: greedy with repetition_penalty = 1.3; greedy with no_repeat_ngram_size = 2; greedy with
min_new_tokens = 6 and EOS ids taken from the plain run so that it stops earlier; greedy with all three; beam search (K = 3) with
penalty 1.2 and n-gram 2.  Per case: the seeds that make the weights and the prompt embeddings, the options, the ids (beam: scores and
lengths too) of the processed and of the plain run, and the smallest top-1 / top-2 margin of the PROCESSED scores along each recorded
path (beam: tests/beam_ref.py's gap between consecutive live candidates).  `model.norm.weight` is multiplied by `norm_mul`, as in
tools/gen_beam_golden.py, because the random-init models are almost flat; the prompt seed is searched until the reference alone meets:
  - the processed run differs from the plain run in at least one token;
  - the plain run of an n-gram case (greedy n-gram 2, beam) contains a repeated 2-gram, the processed run of every n-gram case none;
  - every row of a min_new case's plain run is shorter than 6 tokens;
  - every margin is >= 1e-3 (the fp32 kernels differ from torch by about 1e-5).

    python tools/gen_logits_proc_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle.gen_golden import import_reference, build_ref_llama  # noqa: E402
from oracle.golden_cfgs import TINY_LLAMA, TINY_MHA  # noqa: E402
import beam_ref  # noqa: E402
import logits_proc_ref as lpr  # noqa: E402

MIN_MARGIN = 1e-3
MAX_NEW = 12
BATCH = 3
NORM_MUL = 32
MODELS = {"tiny_mha": (TINY_MHA, 32, 17), "tiny_gqa": (TINY_LLAMA, 31, 21)}      # config, weight seed, prompt length
SEEDS = range(2000, 2200)                                                        # prompt seeds tried, in order


def greedy(llm, x, eos, pad, **proc):
    """-> ids (B, MAX_NEW) pad-filled, n_cols, per-row lengths, smallest top-1 / top-2 margin of the processed scores over live rows"""
    g = llm.generation_config
    g.eos_token_id = list(eos) if len(eos) else None
    g.pad_token_id = pad
    with torch.no_grad():
        out = llm.generate(inputs_embeds=x, max_new_tokens=MAX_NEW, do_sample=False, num_beams=1, output_scores=True, return_dict_in_generate=True, **proc)
    seq = out.sequences
    B, n_cols = seq.shape
    live = torch.ones(B, dtype=torch.bool)
    lens = torch.full((B,), n_cols, dtype=torch.int64)
    margin = float("inf")
    for t, s in enumerate(out.scores):
        top = torch.topk(s.float(), 2, dim=-1).values
        for b in range(B):
            if not live[b]:
                continue
            assert int(s[b].argmax()) == int(seq[b, t])
            margin = min(margin, float(top[b, 0] - top[b, 1]))
            if int(seq[b, t]) in eos:
                live[b] = False
                lens[b] = t + 1
    ids = torch.full((B, MAX_NEW), pad, dtype=torch.int64)
    ids[:, :n_cols] = seq
    return ids, n_cols, lens, margin


def beam(llm, x, K, pad, **proc):
    g = llm.generation_config
    g.eos_token_id = None
    g.pad_token_id = pad
    with torch.no_grad():
        out = llm.generate(inputs_embeds=x, max_new_tokens=MAX_NEW, num_beams=K, num_return_sequences=1, length_penalty=1.0, early_stopping=False,
                           do_sample=False, output_scores=True, return_dict_in_generate=True, **proc)
    seqs = out.sequences
    lens = (out.beam_indices >= 0).sum(dim=1)
    ids = torch.full((seqs.shape[0], MAX_NEW), pad, dtype=torch.int64)
    ids[:, :seqs.shape[1]] = seqs
    for r in range(ids.shape[0]):
        ids[r, int(lens[r]):] = pad
    # replay of the processed log-probabilities (HF's `scores`: after the processors, before the running score is added)
    M = beam_ref.n_candidates(K, 0)
    ref = beam_ref.BeamRef(BATCH, K, MAX_NEW, (), 1.0, False, pad)
    for s in out.scores:
        top = torch.topk(s.float(), M + 4, dim=-1)
        assert bool(torch.isfinite(top.values).all())
        ref.step_logprobs(top.values.view(BATCH, K, -1), top.indices.view(BATCH, K, -1))
    r_ids, r_scores, r_lens = ref.result(1)
    assert torch.equal(r_ids.view(-1, MAX_NEW), ids) and torch.equal(r_lens.view(-1), lens) and torch.equal(r_scores.view(-1), out.sequences_scores.float())
    return ids, out.sequences_scores.float(), lens, ref.min_gap


def main():
    _, llama_mod, _ = import_reference()
    arrays, names = {}, []
    for model, (cfg, wseed, S) in MODELS.items():
        llm, _ = build_ref_llama(llama_mod, cfg, wseed)
        with torch.no_grad():
            llm.model.norm.weight.mul_(NORM_MUL)
        pad = cfg.pad_token_id

        def prompt(seed):
            return torch.randn(BATCH, S, cfg.hidden_size, generator=torch.Generator().manual_seed(seed)) * 0.05

        def record(name, seed, eos, K, proc, got, plain):
            full = f"{model}_{name}"
            names.append(full)
            arrays.update({f"{full}.model": model, f"{full}.weight_seed": wseed, f"{full}.input_seed": seed, f"{full}.S": S, f"{full}.norm_mul": NORM_MUL,
                           f"{full}.batch": BATCH, f"{full}.max_new": MAX_NEW, f"{full}.pad": pad, f"{full}.eos": np.asarray(sorted(eos), dtype=np.int64),
                           f"{full}.K": K, f"{full}.repetition_penalty": float(proc.get("repetition_penalty", 1.0)),
                           f"{full}.no_repeat_ngram_size": int(proc.get("no_repeat_ngram_size", 0)), f"{full}.min_new_tokens": int(proc.get("min_new_tokens", 0))})
            for tag, r in (("", got), ("plain_", plain)):
                arrays[f"{full}.{tag}ids"] = r["ids"].numpy().astype(np.int32)
                arrays[f"{full}.{tag}lens"] = r["lens"].numpy().astype(np.int32)
                arrays[f"{full}.{tag}min_margin"] = float(r["margin"])
                if K > 1:
                    arrays[f"{full}.{tag}scores"] = r["scores"].numpy()
                else:
                    arrays[f"{full}.{tag}n_cols"] = int(r["n_cols"])
            print(f"{full}: seed {seed} margins {got['margin']:.2e} / plain {plain['margin']:.2e} lens {got['lens'].tolist()} / plain {plain['lens'].tolist()}")

        def greedy_case(name, proc, with_eos):
            for seed in SEEDS:
                x = prompt(seed)
                eos = []
                if with_eos:       # the tokens the plain run without EOS emits at steps 2, 3 and 4 of rows 0, 1 and 2: every row then stops before 6
                    free, *_ = greedy(llm, x, [], pad)
                    eos = sorted({int(free[b, 2 + b]) for b in range(BATCH)})
                p_ids, p_cols, p_lens, p_margin = greedy(llm, x, eos, pad)
                ids, cols, lens, margin = greedy(llm, x, eos, pad, **proc)
                ok = not torch.equal(ids, p_ids) and margin >= MIN_MARGIN and p_margin >= MIN_MARGIN
                if proc.get("no_repeat_ngram_size", 0) > 0:
                    if proc.get("min_new_tokens", 0) == 0:       # (a plain run that stops before 6 tokens has no room for one)
                        ok = ok and any(lpr.has_repeated_ngram(p_ids[b, :int(p_lens[b])].tolist(), 2) for b in range(BATCH))
                    ok = ok and not any(lpr.has_repeated_ngram(ids[b, :int(lens[b])].tolist(), 2) for b in range(BATCH))
                if proc.get("min_new_tokens", 0) > 0:
                    ok = ok and int(p_lens.max()) < 6 and int(lens.min()) >= 6
                if ok:
                    record(name, seed, eos, 1, proc, dict(ids=ids, n_cols=cols, lens=lens, margin=margin), dict(ids=p_ids, n_cols=p_cols, lens=p_lens, margin=p_margin))
                    return
            raise SystemExit(f"{model}_{name}: no prompt seed in {SEEDS} meets the conditions")

        def beam_case(name, K, proc):
            for seed in SEEDS:
                x = prompt(seed)
                p_ids, p_sc, p_lens, p_gap = beam(llm, x, K, pad)
                ids, sc, lens, gap = beam(llm, x, K, pad, **proc)
                rep = any(lpr.has_repeated_ngram(p_ids[b, :int(p_lens[b])].tolist(), 2) for b in range(BATCH))
                if rep and not torch.equal(ids, p_ids) and gap >= MIN_MARGIN and p_gap >= MIN_MARGIN:
                    record(name, seed, [], K, proc, dict(ids=ids, scores=sc, lens=lens, margin=gap), dict(ids=p_ids, scores=p_sc, lens=p_lens, margin=p_gap))
                    return
            raise SystemExit(f"{model}_{name}: no prompt seed in {SEEDS} meets the conditions")

        greedy_case("rep13", dict(repetition_penalty=1.3), False)
        greedy_case("ngram2", dict(no_repeat_ngram_size=2), False)
        greedy_case("minnew6", dict(min_new_tokens=6), True)
        greedy_case("all3", dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6), True)
        beam_case("beam_k3", 3, dict(repetition_penalty=1.2, no_repeat_ngram_size=2))
    arrays["cases"] = np.asarray(names)
    path = os.path.join(REPO, "tests", "golden", "logits_proc_tiny.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), {len(names)} cases")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
