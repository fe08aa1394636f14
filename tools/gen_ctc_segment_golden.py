#!/usr/bin/env python
"""Writes tests/golden/ctc_segment_tiny.npz: CTC segmentation fixtures recorded from HF's tokenizer and the reference's preprocessing (CPU).

Per sequence of seeded greedy ids (the ls960-ft vocabulary: `<pad>` 0 = blank, `<s>` 1, `</s>` 2, `<unk>` 3, `|` 4 = word delimiter, letters
5 .. 31): the word offsets `Wav2Vec2CTCTokenizer.decode(ids, output_word_offsets=True)` returns, and the list the reference's
`get_hubert_ctc_pool_ranges` stores for them with pool_range 4 (it only needs a list subclass with `add_column`).  Sequences whose decode has no
word are kept with zero words and zero ranges recorded: the reference raises IndexError there.  Data only; tests/ctc_segment_ref.py must
reproduce every recorded list before anything is written.

    python tools/gen_ctc_segment_golden.py
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle.gen_golden import REF  # noqa: E402
import ctc_segment_ref as ref  # noqa: E402

VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|"] + list("ETAONIHSRDLUMWCFGYPBVK'XJQZ")
BLANK, DELIM, POOL_RANGE = 0, 4, 4


def sequences():
    """hand-made edge cases, then seeded random sequences at several blank / delimiter densities"""
    L_ = 7
    seqs = [[BLANK] * 9, [DELIM] * 5, [L_], [BLANK], [DELIM], [L_, L_, 8, BLANK, BLANK, 9, DELIM, BLANK, 10, 10], [BLANK, BLANK, L_, 8, 9],
            [L_] * 3 + [DELIM] + [8] * 4 + [DELIM] + [9] * 5 + [DELIM] + [10] * 8, [L_, DELIM] * 6, [L_, DELIM] * 6 + [L_],
            [BLANK, 1, L_, 2, BLANK, DELIM, 3, 3, BLANK], [L_, BLANK] * 40 + [DELIM, BLANK, 8], [DELIM, DELIM, L_, BLANK, DELIM, DELIM, BLANK, 8, DELIM]]
    rng = np.random.RandomState(20241)
    for T, p_blank, p_delim in [(1, .3, .3), (2, .3, .3), (17, .5, .2), (63, .6, .1), (64, .6, .1), (65, .2, .4), (130, .7, .08), (257, .6, .1),
                                (300, .9, .05), (300, .1, .02), (500, .5, .3), (1500, .65, .08)]:
        for _ in range(2):
            u = rng.rand(T)
            letters = rng.randint(1, len(VOCAB), size=T)
            letters[letters == DELIM] = 5
            ids = np.where(u < p_blank, BLANK, np.where(u < p_blank + p_delim, DELIM, letters))
            seqs.append(np.repeat(ids, rng.randint(1, 4, size=T))[:T].tolist())      # CTC-like runs of repeated ids
    return seqs


class Rows(list):
    def add_column(self, name, column):
        return Rows(dict(row, **{name: c}) for row, c in zip(self, column))


def main():
    from transformers import Wav2Vec2CTCTokenizer
    spec = importlib.util.spec_from_file_location("ref_preprocess_utils", os.path.join(REF, "preprocess_data", "utils.py"))
    ref_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_utils)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "vocab.json"), "w") as f:
            json.dump({tok: i for i, tok in enumerate(VOCAB)}, f)
        tok = Wav2Vec2CTCTokenizer(os.path.join(d, "vocab.json"), unk_token="<unk>", pad_token="<pad>", bos_token="<s>", eos_token="</s>",
                                   word_delimiter_token="|")
    seqs = sequences()
    ids_flat, ids_len, words_flat, words_len, ranges_flat, ranges_len = [], [], [], [], [], []
    for ids in seqs:
        out = tok.decode(ids, output_word_offsets=True)
        words = [(int(w["start_offset"]), int(w["end_offset"])) for w in out.word_offsets]
        assert words == ref.words(ids, BLANK, DELIM), (ids, words, ref.words(ids, BLANK, DELIM))
        if words:
            ds = ref_utils.get_hubert_ctc_pool_ranges(Rows([{"hubert_word_offsets": out.word_offsets}]), pool_range=POOL_RANGE)
            ranges = [(int(a), int(b)) for a, b in ds[0]["pool_ranges_4"]]
            assert ranges == ref.raw_ranges(words, len(ids), POOL_RANGE), (ids, ranges)
        else:
            ranges = []
        ids_flat += ids; ids_len.append(len(ids))
        words_flat += words; words_len.append(len(words))
        ranges_flat += ranges; ranges_len.append(len(ranges))
    path = os.path.join(REPO, "tests", "golden", "ctc_segment_tiny.npz")
    np.savez_compressed(path, ids=np.asarray(ids_flat, np.int32), ids_len=np.asarray(ids_len, np.int32),
                        words=np.asarray(words_flat, np.int32).reshape(-1, 2), words_len=np.asarray(words_len, np.int32),
                        ranges=np.asarray(ranges_flat, np.int32).reshape(-1, 2), ranges_len=np.asarray(ranges_len, np.int32),
                        blank_id=BLANK, delim_id=DELIM, pool_range=POOL_RANGE, vocab=np.asarray(VOCAB))
    print(f"wrote {path}: {len(seqs)} sequences, {len(words_flat)} words, {len(ranges_flat)} ranges, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
