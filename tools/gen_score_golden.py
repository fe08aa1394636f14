#!/usr/bin/env python
"""Writes tests/golden/score_tiny.npz: the reference class's own numbers for GIVEN answers that are not its argmax (CPU, fp32), on the
model of tests/golden/token_scores_tiny.npz (tiny random-init 2-layer Llama, vocab 1 000, `model.norm.weight` x 32).

Per case — target lengths 1, 2 and 13 at the ragged prompt lengths 9 / 21 / 14 — and per sample: seeded prompt embeddings (row b of a
case is its own draw, as in the token-scores fixture), seeded RANDOM target ids, then
  logprobs   the per-token gather of log_softmax (in fp64) of the reference class's logits at rows [P - 1, P - 1 + n) of
             [prompt | embed(target[:-1])] against target, and
  loss       the reference class's forward(inputs_embeds=[prompt | embed(labels[1:])], labels=[labels]).loss with labels = [0 | target]:
             its labels[1:] convention scores exactly those rows, so loss = -mean(logprobs) up to fp32.
Only arrays and configuration values are stored.  Needs the reference checkout; the test suite never runs a program of the reference's.

    python tools/gen_score_golden.py
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

PROMPT_LENS = [9, 21, 14]
TARGET_LENS = [1, 2, 13]
INPUT_SEED = 5100
TARGET_SEED = 5200


def main():
    g = np.load(os.path.join(REPO, "tests", "golden", "token_scores_tiny.npz"))
    cfg_kw = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg.") and k[4:] not in ("weight_seed", "norm_mul", "max_new")}
    weight_seed, norm_mul = int(g["cfg.weight_seed"]), float(g["cfg.norm_mul"])
    _, llama_mod, _ = import_reference()
    cfg = LlamaCfg(rope_scaling=None, eos_token_ids=(), **cfg_kw)
    llm, _ = build_ref_llama(llama_mod, cfg, weight_seed)
    with torch.no_grad():
        llm.model.norm.weight.mul_(norm_mul)
    H, V = cfg.hidden_size, cfg.vocab_size
    emb = llm.model.embed_tokens
    arrays = {"prompt_lens": np.asarray(PROMPT_LENS, dtype=np.int32), "target_lens": np.asarray(TARGET_LENS, dtype=np.int32)}
    for n in TARGET_LENS:
        seed = INPUT_SEED + n
        targets = torch.randint(0, V, (len(PROMPT_LENS), n), generator=torch.Generator().manual_seed(TARGET_SEED + n))
        lps, losses, ranks = [], [], []
        for b, P in enumerate(PROMPT_LENS):
            prompt = torch.randn(P, H, generator=torch.Generator().manual_seed(seed * 100 + b)) * 0.05
            tg = targets[b]
            with torch.no_grad():
                seq = torch.cat([prompt, emb(tg[:-1])], 0)
                logits = llm(inputs_embeds=seq[None]).logits[0]
                lp = torch.log_softmax(logits[P - 1:P - 1 + n].double(), dim=-1).gather(1, tg.view(-1, 1))[:, 0]
                labels = torch.cat([torch.zeros(1, dtype=torch.long), tg])
                loss = llm(inputs_embeds=torch.cat([prompt, emb(labels[1:])], 0)[None], labels=[labels]).loss
            assert abs(float(loss) + float(lp.mean())) < 1e-4 * max(1.0, abs(float(loss))), (float(loss), float(lp.mean()))
            ranks += [int((logits[P - 1 + j] > logits[P - 1 + j, tg[j]]).sum()) for j in range(n)]
            lps.append(lp.numpy())
            losses.append(float(loss))
        assert sum(r > 0 for r in ranks) >= max(1, len(ranks) - 1), ranks            # the targets are NOT the argmax (what the greedy fixture cannot cover)
        arrays.update({f"n{n}.input_seed": seed, f"n{n}.targets": targets.numpy().astype(np.int32), f"n{n}.logprobs": np.stack(lps).astype(np.float64),
                       f"n{n}.loss": np.asarray(losses, dtype=np.float32)})
        print(f"n={n}: seed {seed} losses {[round(v, 4) for v in losses]} target ranks {ranks}")
    path = os.path.join(REPO, "tests", "golden", "score_tiny.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} B)")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
