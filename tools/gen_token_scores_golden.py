#!/usr/bin/env python
"""Writes tests/golden/token_scores_tiny.npz: what the reference class returns (CPU, fp32, HF `generate(inputs_embeds=...,
return_dict_in_generate=True, output_scores=True)`) and transformers' `compute_transition_scores(sequences, scores,
normalize_logits=True)` for it, on a tiny random-init 2-layer model with vocab 1 000.

Cases: greedy without EOS; greedy with each logits processor (repetition_penalty 1.3, no_repeat_ngram_size 2, min_new_tokens 6); two EOS
mixes (every row stops early; one row stops, the others run to the budget); batch 1; batch 3 with ragged (left-padded) prompts, with and
without EOS.  Per case: the seeds that make the weights and the prompt embeddings, the prompt lengths, the options, the ids, the per-row
lengths, the transition scores with 0.0 at and after a row's finish, and the smallest top-1 / top-2 margin of the scores along the path.
`model.norm.weight` is multiplied by `norm_mul` (the random-init models are almost flat); the prompt seed is searched until every margin
is >= 1e-3 (the fp32 kernels differ from torch by about 1e-5) and the case's own condition holds.  Only arrays and configuration values
are stored.

    python tools/gen_token_scores_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle.gen_golden import import_reference, build_ref_llama  # noqa: E402
from oracle.llama_oracle import LlamaCfg  # noqa: E402
import token_scores_ref as tsr  # noqa: E402

CFG = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384, vocab_size=1000,
           rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False, pad_token_id=0)
WEIGHT_SEED = 41
NORM_MUL = 32
MAX_NEW = 12
MIN_MARGIN = 1e-3
SEEDS = range(3000, 3200)


def run(llm, x, mask, eos, pad, **proc):
    g = llm.generation_config
    g.eos_token_id = list(eos) if len(eos) else None
    g.pad_token_id = pad
    with torch.no_grad():
        out = llm.generate(inputs_embeds=x, attention_mask=mask, max_new_tokens=MAX_NEW, do_sample=False, num_beams=1, output_scores=True,
                           return_dict_in_generate=True, **proc)
        trans = llm.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    seq = out.sequences
    B, n_cols = seq.shape
    live = torch.ones(B, dtype=torch.bool)
    lens = torch.full((B,), n_cols, dtype=torch.int64)
    lps = torch.zeros(B, MAX_NEW, dtype=torch.float32)
    margin = float("inf")
    for t, s in enumerate(out.scores):
        top = torch.topk(s.float(), 2, dim=-1).values
        for b in range(B):
            if not live[b]:
                continue
            assert int(s[b].argmax()) == int(seq[b, t])
            lps[b, t] = trans[b, t]
            margin = min(margin, float(top[b, 0] - top[b, 1]))
            if int(seq[b, t]) in eos:
                live[b] = False
                lens[b] = t + 1
    # the restatement of the definition agrees with transformers on the recorded path
    want = tsr.sequence_logprobs([s for s in out.scores], seq, eos)
    assert float((want[:, :n_cols] - lps[:, :n_cols].double()).abs().max()) < 1e-5
    ids = torch.full((B, MAX_NEW), pad, dtype=torch.int64)
    ids[:, :n_cols] = seq
    return ids, n_cols, lens, lps, margin


def main():
    _, llama_mod, _ = import_reference()
    cfg = LlamaCfg(rope_scaling=None, eos_token_ids=(), **CFG)
    llm, _ = build_ref_llama(llama_mod, cfg, WEIGHT_SEED)
    with torch.no_grad():
        llm.model.norm.weight.mul_(NORM_MUL)
    pad = CFG["pad_token_id"]
    arrays, names = {f"cfg.{k}": v for k, v in CFG.items()}, []
    arrays.update({"cfg.weight_seed": WEIGHT_SEED, "cfg.norm_mul": NORM_MUL, "cfg.max_new": MAX_NEW})

    def prompt(seed, lens):
        """left-padded (B, S, h) embeddings + mask; row b's rows are its own draw, so a row's prompt does not depend on the batch"""
        S = max(lens)
        x = torch.zeros(len(lens), S, CFG["hidden_size"])
        mask = torch.zeros(len(lens), S, dtype=torch.long)
        for b, n in enumerate(lens):
            x[b, S - n:] = torch.randn(n, CFG["hidden_size"], generator=torch.Generator().manual_seed(seed * 100 + b)) * 0.05
            mask[b, S - n:] = 1
        return x, mask

    def case(name, lens, proc, eos_rule):
        """eos_rule: None (no EOS); "all": the tokens the free run emits at steps 2 + b of row b; "one": the token row 0 emits at step 3"""
        for seed in SEEDS:
            x, mask = prompt(seed, lens)
            eos = []
            if eos_rule is not None:
                free, *_ = run(llm, x, mask, [], pad, **proc)
                eos = sorted({int(free[b, 2 + b]) for b in range(len(lens))}) if eos_rule == "all" else [int(free[0, 3])]
            ids, n_cols, rl, lps, margin = run(llm, x, mask, eos, pad, **proc)
            ok = margin >= MIN_MARGIN and bool((lps <= 0).all())
            if eos_rule == "all" and proc.get("min_new_tokens", 0) > 0:      # the EOS ids would stop every row before step 6: none may
                ok = ok and int(rl.min()) >= proc["min_new_tokens"]
            elif eos_rule == "all":
                ok = ok and int(rl.max()) < MAX_NEW
            if eos_rule == "one":
                ok = ok and int(rl[0]) < MAX_NEW and int(rl.max()) == MAX_NEW
            if not ok:
                continue
            names.append(name)
            arrays.update({f"{name}.input_seed": seed, f"{name}.prompt_lens": np.asarray(lens, dtype=np.int32), f"{name}.eos": np.asarray(eos, dtype=np.int64),
                           f"{name}.repetition_penalty": float(proc.get("repetition_penalty", 1.0)),
                           f"{name}.no_repeat_ngram_size": int(proc.get("no_repeat_ngram_size", 0)), f"{name}.min_new_tokens": int(proc.get("min_new_tokens", 0)),
                           f"{name}.ids": ids.numpy().astype(np.int32), f"{name}.n_cols": int(n_cols), f"{name}.lens": rl.numpy().astype(np.int32),
                           f"{name}.logprobs": lps.numpy(), f"{name}.min_margin": float(margin)})
            print(f"{name}: seed {seed} margin {margin:.2e} lens {rl.tolist()} mean logprob {float(lps.sum() / rl.sum()):.3f}")
            return
        raise SystemExit(f"{name}: no prompt seed in {SEEDS} meets the conditions")

    case("greedy", [17, 17, 17], {}, None)
    case("rep13", [17, 17, 17], dict(repetition_penalty=1.3), None)
    case("ngram2", [17, 17, 17], dict(no_repeat_ngram_size=2), None)
    case("minnew6", [17, 17, 17], dict(min_new_tokens=6), "all")
    case("eos_all", [17, 17, 17], {}, "all")
    case("eos_one", [17, 17, 17], {}, "one")
    case("batch1", [23], {}, None)
    case("batch1_eos", [23], {}, "all")
    case("ragged3", [9, 21, 14], {}, None)
    case("ragged3_eos", [9, 21, 14], {}, "one")
    arrays["cases"] = np.asarray(names)
    path = os.path.join(REPO, "tests", "golden", "token_scores_tiny.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), {len(names)} cases")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
