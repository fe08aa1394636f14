#!/usr/bin/env python
"""Writes tests/golden/beam_tiny.npz: beam-search fixtures recorded from the reference class (CPU, HF `generate(num_beams=K)`).

Per case: the options, what the reference returned (ids, sequences_scores, lengths) and, for the CPU replay of tests/beam_ref.py,
each step's per-row top-(M + 4) of HF's `scores` (log-probabilities before the running score is added, HF's row order s * K + j).
The tiny random-init models have almost flat distributions (candidate gaps down to 4e-6, a few fp32 ulps), far too small to ask two
devices for the same ids, so `model.norm.weight` is multiplied by `norm_mul` to sharpen the logits, and a case is written only if
the smallest gap between consecutive live candidates among the top M + 1 of every step is >= 1e-3 (10x the fp32 tolerance F32_TOL =
1e-4): a condition on the inputs.  The replay must reproduce the reference exactly before anything is written.

    python tools/gen_beam_golden.py
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

MIN_GAP = 1e-3
MAX_NEW = 12
BATCH = 3
MODELS = {"tiny_mha": (TINY_MHA, 32, 17), "tiny_gqa": (TINY_LLAMA, 31, 21)}      # config, weight seed, prompt length


def run_reference(llm, x, K, eos, lp, es, R, pad):
    g = llm.generation_config
    g.eos_token_id = list(eos) if eos else None
    g.pad_token_id = pad
    with torch.no_grad():
        out = llm.generate(inputs_embeds=x, max_new_tokens=MAX_NEW, num_beams=K, num_return_sequences=R, length_penalty=lp, early_stopping=es,
                           do_sample=False, output_scores=True, return_dict_in_generate=True)
    seqs = out.sequences
    lens = (out.beam_indices >= 0).sum(dim=1)
    ids = torch.full((seqs.shape[0], MAX_NEW), pad, dtype=torch.int64)
    ids[:, :seqs.shape[1]] = seqs
    for r in range(ids.shape[0]):
        ids[r, int(lens[r]):] = pad
    M = beam_ref.n_candidates(K, len(eos))
    top = [torch.topk(s.float(), M + 4, dim=-1) for s in out.scores]
    val = torch.stack([t.values for t in top])           # (steps, B * K, M + 4)
    idx = torch.stack([t.indices for t in top])
    return ids, out.sequences_scores.float(), lens, val, idx


def replay(val, idx, K, eos, lp, es, R, pad):
    ref = beam_ref.BeamRef(BATCH, K, MAX_NEW, eos, lp, es, pad)
    for t in range(val.shape[0]):
        ref.step_logprobs(val[t].view(BATCH, K, -1), idx[t].view(BATCH, K, -1))
    assert ref.all_done(), "the reference stopped before every sequence was done"
    return ref


def main():
    _, llama_mod, _ = import_reference()
    arrays, names = {}, []

    def case(name, model, norm_mul, eos, K, lp, es, R=1, need_eos_props=False):
        cfg, seed, S = MODELS[model]
        llm, _ = build_ref_llama(llama_mod, cfg, seed)
        with torch.no_grad():
            llm.model.norm.weight.mul_(norm_mul)
        x = torch.randn(BATCH, S, cfg.hidden_size, generator=torch.Generator().manual_seed(1000 + seed)) * 0.05
        pad = cfg.pad_token_id
        ids, scores, lens, val, idx = run_reference(llm, x, K, eos, lp, es, R, pad)
        ref = replay(val, idx, K, eos, lp, es, R, pad)
        r_ids, r_scores, r_lens = ref.result(R)
        assert torch.equal(r_ids.view(-1, MAX_NEW), ids), (name, r_ids, ids)
        assert torch.equal(r_lens.view(-1), lens), (name, r_lens, lens)
        assert torch.equal(r_scores.view(-1), scores), (name, r_scores, scores)
        if need_eos_props:
            # a hypothesis shorter than the budget, a sequence that runs all MAX_NEW steps, a step whose source beam is not the row's own
            assert int(lens.min()) < MAX_NEW and val.shape[0] == MAX_NEW and ref.reordered, (name, lens, val.shape[0], ref.reordered)
        print(f"{name}: lens {lens.tolist()} min gap {ref.min_gap:.2e} re-ordered after step 0: {ref.reordered_late}")
        if ref.min_gap < MIN_GAP:
            print(f"  left out: gap {ref.min_gap:.2e} < {MIN_GAP}")
            return ids
        names.append(name)
        es_code = {False: 0, True: 1, "never": 2}[es]
        arrays.update({f"{name}.model": model, f"{name}.weight_seed": seed, f"{name}.input_seed": 1000 + seed, f"{name}.S": S, f"{name}.norm_mul": norm_mul,
                       f"{name}.eos": np.asarray(eos, dtype=np.int64), f"{name}.K": K, f"{name}.R": R, f"{name}.length_penalty": lp,
                       f"{name}.early_stopping": es_code, f"{name}.pad": pad, f"{name}.max_new": MAX_NEW, f"{name}.batch": BATCH,
                       f"{name}.ids": ids.numpy().astype(np.int32), f"{name}.scores": scores.numpy(), f"{name}.lens": lens.numpy().astype(np.int32),
                       f"{name}.top_val": val.numpy(), f"{name}.top_idx": idx.numpy().astype(np.int32), f"{name}.min_gap": ref.min_gap, f"{name}.reordered_late": ref.reordered_late})
        return ids

    def derive_eos(model, norm_mul):
        """tokens the no-EOS K = 3 run emits at steps 3, 6 and 9 of sequences 0, 1 and 2"""
        cfg, seed, S = MODELS[model]
        llm, _ = build_ref_llama(llama_mod, cfg, seed)
        with torch.no_grad():
            llm.model.norm.weight.mul_(norm_mul)
        x = torch.randn(BATCH, S, cfg.hidden_size, generator=torch.Generator().manual_seed(1000 + seed)) * 0.05
        ids, *_ = run_reference(llm, x, 3, (), 1.0, False, 1, cfg.pad_token_id)
        return sorted({int(ids[0, 3]), int(ids[1, 6]), int(ids[2, 9])})

    eos_mha = derive_eos("tiny_mha", 32)
    eos_gqa = derive_eos("tiny_gqa", 32)
    print("eos ids:", eos_mha, eos_gqa)
    case("mha_k2_eos", "tiny_mha", 32, eos_mha, 2, 1.0, False, need_eos_props=True)
    case("mha_k3_eos_early", "tiny_mha", 32, eos_mha, 3, 1.0, True, need_eos_props=True)
    case("mha_k3_eos_lp2", "tiny_mha", 32, eos_mha, 3, 2.0, False, need_eos_props=True)
    case("mha_k4", "tiny_mha", 32, (), 4, 1.0, False)
    case("gqa_k2_eos_lp2", "tiny_gqa", 32, eos_gqa, 2, 2.0, False, need_eos_props=True)
    case("gqa_k4", "tiny_gqa", 8, (), 4, 1.0, False)
    case("mha_k3_eos_never", "tiny_mha", 32, eos_mha, 3, 1.0, "never")
    case("mha_k3_eos_r3", "tiny_mha", 32, eos_mha, 3, 1.0, False, R=3)
    assert sum(bool(arrays[f"{n}.reordered_late"]) for n in names) >= 4, "too few cases move generated K/V positions between slots"
    arrays["cases"] = np.asarray(names)
    path = os.path.join(REPO, "tests", "golden", "beam_tiny.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB), {len(names)} cases")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
