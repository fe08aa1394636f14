"""Beam search restated in plain torch (a helper module of the beam tests, not a conftest).

The specification is HF's vectorised `_beam_search` (hf:generation/utils.py: `_get_top_k_continuations`,
`_get_running_beams_for_next_iteration`, `_update_finished_beams`, `_check_early_stop_heuristic`,
`_beam_search_has_unfinished_sequences`) for prompts given as embeddings (decoder_prompt_len = 0, max_length = max_new_tokens)
with do_sample = False — the seven steps of include/speechllm.h above sl_beam_opts.  Every score is a float32 tensor and every
operation on it is the float32 torch operation HF performs, so a replay from the same per-row candidate lists reproduces HF's
scores to the last bit; ties (which HF leaves to torch.topk) are ordered by larger value, then lower flat index j * V + v.
"""
import torch

NEG = -1.0e9
F32 = torch.float32


def n_candidates(num_beams, n_eos):
    return max(2, 1 + n_eos) * num_beams


def _top(values, k):
    """indices of the k largest entries of a 1-D float32 tensor, earlier index first on ties"""
    v = values.tolist()
    return sorted(range(len(v)), key=lambda i: (-v[i], i))[:k]


class BeamRef:
    def __init__(self, nseq, num_beams, max_new, eos_ids=(), length_penalty=1.0, early_stopping=False, pad_id=0):
        assert early_stopping in (False, True, "never")
        K = num_beams
        self.nseq, self.K, self.max_new, self.eos = nseq, K, max_new, [int(e) for e in eos_ids]
        self.lp, self.es, self.pad = float(length_penalty), early_stopping, int(pad_id)
        self.M = n_candidates(K, len(self.eos))
        self.t = [0] * nseq
        self.run_hist = torch.zeros((nseq, K, max_new), dtype=torch.int64)
        self.run_score = torch.full((nseq, K), NEG, dtype=F32)
        self.run_score[:, 0] = 0.0
        self.next_ids = torch.zeros((nseq, K), dtype=torch.int64)
        self.src_beam = torch.zeros((nseq, K), dtype=torch.int64)
        self.fin_hist = torch.zeros((nseq, K, max_new), dtype=torch.int64)
        self.fin_score = torch.full((nseq, K), NEG, dtype=F32)
        self.fin_flag = torch.zeros((nseq, K), dtype=torch.bool)
        self.fin_len = torch.zeros((nseq, K), dtype=torch.int64)
        self.open = [True] * nseq
        self.done = [False] * nseq
        self.min_gap = float("inf")        # smallest difference between consecutive live candidates among the top M + 1, over not-done sequences
        self.reordered = False             # some step chose a source beam other than the row's own (at step 0 every beam but the first does)
        self.reordered_late = False        # ... and some step after the first did: generated K/V positions move between slots

    def len_pen(self, length):
        return torch.tensor(float(length) ** self.lp, dtype=F32)      # python double pow, rounded once: what `tensor / python_float` divides by

    def step_logprobs(self, val, tok):
        """val, tok: (nseq, K, L) — per running beam the L >= M largest log-probabilities (float32, WITHOUT the running score) and tokens"""
        return self.step_acc(val.to(F32) + self.run_score[:, :, None], tok)

    def step_acc(self, acc, tok):
        """acc, tok: (nseq, K, L) — per running beam L >= M accumulated scores (log-probability + running score) and their tokens"""
        acc = acc.to(F32)
        for s in range(self.nseq):
            self._step_seq(s, acc[s], tok[s])

    def _step_seq(self, s, acc, tok):
        K, M, t = self.K, self.M, self.t[s]
        assert t < self.max_new
        ent = [(float(acc[j, i]), j, int(tok[j, i])) for j in range(K) for i in range(acc.shape[1])]
        ent.sort(key=lambda e: (-e[0], e[1], e[2]))
        if not self.done[s]:
            live = [e[0] for e in ent[:M + 1] if e[0] > -1.0e8]
            for a, b in zip(live, live[1:]):
                self.min_gap = min(self.min_gap, a - b)
        cand = ent[:M]
        c_sc = torch.tensor([e[0] for e in cand], dtype=F32)
        c_j = [e[1] for e in cand]
        c_v = [e[2] for e in cand]
        last = (t + 1 == self.max_new)
        hit = torch.tensor([last or (v in self.eos) for v in c_v])
        # 4. next running beams
        rv = c_sc + hit.to(F32) * NEG
        sel = _top(rv, K)
        old_hist = self.run_hist[s].clone()
        for k, c in enumerate(sel):
            self.run_hist[s, k] = old_hist[c_j[c]]
            self.run_hist[s, k, t] = c_v[c]
            self.run_score[s, k] = rv[c]
            self.next_ids[s, k] = c_v[c]
            self.src_beam[s, k] = c_j[c]
            if c_j[c] != k:
                self.reordered = True
                self.reordered_late = self.reordered_late or t > 0
        # 5. finished set
        full = bool(self.fin_flag[s].all()) and self.es is True
        did = hit & (torch.arange(M) < K)
        fs = c_sc / self.len_pen(t + 1)
        fs = fs + float(full) * NEG
        fs = fs + float(not self.open[s]) * NEG
        fs = fs + (~did).to(F32) * NEG
        comb = torch.cat([self.fin_score[s], fs])
        selc = _top(comb, K)
        o_hist, o_flag, o_len = self.fin_hist[s].clone(), self.fin_flag[s].clone(), self.fin_len[s].clone()
        for p, i in enumerate(selc):
            self.fin_score[s, p] = comb[i]
            if i < K:
                self.fin_hist[s, p], self.fin_flag[s, p], self.fin_len[s, p] = o_hist[i], o_flag[i], o_len[i]
            else:
                c = i - K
                self.fin_hist[s, p] = old_hist[c_j[c]]
                self.fin_hist[s, p, t] = c_v[c]
                self.fin_hist[s, p, t + 1:] = 0
                self.fin_flag[s, p], self.fin_len[s, p] = bool(did[c]), t + 1
        # 6. early-stop heuristic
        L = self.max_new if (self.es == "never" and self.lp > 0.0) else t + 1
        allf = bool(self.fin_flag[s].all())
        worst = self.fin_score[s].min() if allf else torch.tensor(NEG, dtype=F32)
        self.open[s] = self.open[s] and bool(self.run_score[s, 0] / self.len_pen(L) > worst)
        # 7. done
        if (not self.open[s]) or (self.es is True and allf) or last:
            self.done[s] = True
        self.t[s] = t + 1

    def all_done(self):
        return all(self.done)

    def result(self, num_return_sequences=1):
        """(ids (nseq, R, max_new) int64 with pad past each length, scores (nseq, R) float32, lengths (nseq, R) int64)"""
        R = num_return_sequences
        ids = self.fin_hist[:, :R].clone()
        lens = self.fin_len[:, :R].clone()
        pos = torch.arange(self.max_new)[None, None, :]
        ids[pos >= lens[:, :, None]] = self.pad
        return ids, self.fin_score[:, :R].clone(), lens
