"""No GPU: the host side of the CTC segmentation — the new C exports and their argument checks (all answered before any launch), the pure-Python
restatement tests/ctc_segment_ref.py against the recorded fixture (HF's word offsets, the reference's pool ranges) and against the live HF
tokenizer, the promises of packed mode, the capacity bound, and the inference class without a segmenter."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import ctc_segment_ref as ref
from conftest import REPO, golden, pkg

L = pkg("_lib")
ops = pkg("ops")
inf_mod = pkg("inference")

NEW_EXPORTS = {"sl_ctc_greedy_batch", "sl_ctc_pool_ranges_batch", "sl_ctc_pool_ranges_capacity", "sl_ctc_words_capacity"}
SL_ERR_ARG = -1


def fixture_sequences():
    g = golden("ctc_segment_tiny")
    ids, words, ranges = g["ids"].tolist(), g["words"].tolist(), g["ranges"].tolist()
    out, i0, w0, r0 = [], 0, 0, 0
    for n, nw, nr in zip(g["ids_len"].tolist(), g["words_len"].tolist(), g["ranges_len"].tolist()):
        out.append((ids[i0:i0 + n], [tuple(w) for w in words[w0:w0 + nw]], [tuple(r) for r in ranges[r0:r0 + nr]]))
        i0, w0, r0 = i0 + n, w0 + nw, r0 + nr
    return out, int(g["blank_id"]), int(g["delim_id"]), int(g["pool_range"])


def test_new_symbols_are_declared_exported_and_additive():
    hdr = open(os.path.join(REPO, "include", "speechllm.h")).read()
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", hdr))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(L.EXPORTS)
    lib = C.CDLL(L.LIB_PATH)
    for name in sorted(NEW_EXPORTS):
        assert hasattr(lib, name), name
    assert L.lib().sl_version() == 7          # additive: no ABI bump
    codes = dict(re.findall(r"#define (SL_CTC_RANGES_[A-Z]+) (\d+)", hdr))
    assert int(codes["SL_CTC_RANGES_PACKED"]) == L.CTC_RANGES_PACKED and int(codes["SL_CTC_RANGES_RAW"]) == L.CTC_RANGES_RAW


def test_argument_errors_come_back_as_sl_err_arg_without_a_device():
    lib = L.lib()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)

    def err(rc, *words):
        assert rc == SL_ERR_ARG
        msg = lib.sl_last_error().decode()
        assert all(w in msg for w in words), msg

    # the head
    err(lib.sl_ctc_greedy_batch(None, p, p, p, 10, 64, 32, L.SL_BF16, None), "null")
    err(lib.sl_ctc_greedy_batch(p, None, p, p, 10, 64, 32, L.SL_BF16, None), "null")
    err(lib.sl_ctc_greedy_batch(p, p, p, None, 10, 64, 32, L.SL_BF16, None), "null")
    err(lib.sl_ctc_greedy_batch(p, p, None, p, 10, 64, 65, L.SL_BF16, None), "V=65")
    err(lib.sl_ctc_greedy_batch(p, p, None, p, 10, 64, 0, L.SL_F32, None), "V=0")
    err(lib.sl_ctc_greedy_batch(p, p, None, p, 10, 68, 32, L.SL_F16, None), "H=68")
    err(lib.sl_ctc_greedy_batch(p, p, None, p, 10, 64, 32, 9, None), "dtype")
    assert lib.sl_ctc_greedy_batch(p, p, None, p, 0, 64, 32, L.SL_BF16, None) == 0           # no rows: nothing to do

    # the segmentation
    cap, wcap = lib.sl_ctc_pool_ranges_capacity(100, 3), lib.sl_ctc_words_capacity(100, 3)
    assert cap == 100 + 2 * 3 and wcap == (100 + 3) // 2

    def seg(ids=p, offs=p, n_utt=3, n_rows=100, blank=0, delim=4, pr=4, mode=L.CTC_RANGES_PACKED, table=p, tcap=cap, counts=p, words=None, wc=0,
            wcounts=None):
        return lib.sl_ctc_pool_ranges_batch(ids, offs, n_utt, n_rows, blank, delim, pr, mode, table, tcap, counts, words, wc, wcounts, None)

    err(seg(ids=None), "null")
    err(seg(offs=None), "null")
    err(seg(table=None), "null")
    err(seg(counts=None), "null")
    err(seg(n_utt=0), "n_utt=0")
    err(seg(blank=4), "blank_id and delim_id are both 4")
    err(seg(pr=0), "pool_range=0")
    err(seg(pr=-4), "pool_range=-4")
    err(seg(mode=2), "mode 2")
    err(seg(tcap=cap - 1), "range table holds 105", "106")
    err(seg(words=p, wc=wcap), "come together")
    err(seg(wcounts=p), "come together")
    err(seg(words=p, wc=wcap - 1, wcounts=p), "word table holds 50", "51")


def test_restatement_equals_the_recorded_hf_word_offsets_and_reference_ranges():
    seqs, blank, delim, pr = fixture_sequences()
    assert len(seqs) >= 30 and max(len(s[0]) for s in seqs) == 1500
    n_noword = 0
    for ids, words, ranges in seqs:
        assert ref.words(ids, blank, delim) == words
        if words:
            assert ref.raw_ranges(words, len(ids), pr) == ranges
        else:                   # the reference raises IndexError here: nothing recorded; the documented divergence is the one range (0, T)
            n_noword += 1
            assert ranges == [] and ref.raw_ranges(words, len(ids), pr) == [(0, len(ids))]
    assert n_noword >= 3
    assert sum(1 for _, _, r in seqs if any(a == b for a, b in r)) >= 1                                           # the recipe does store empty pairs ...
    assert sum(1 for ids, _, r in seqs if any(b > len(ids) for _, b in r)) >= 1                                   # ... and pairs past the utterance


def random_ids(rng, T, p_blank, p_delim, V=32, blank=0, delim=4):
    u = rng.rand(T)
    letters = rng.randint(0, V, size=T)
    letters[(letters == blank) | (letters == delim)] = 7
    return np.where(u < p_blank, blank, np.where(u < p_blank + p_delim, delim, letters)).tolist()


def test_restatement_equals_the_live_hf_tokenizer(tmp_path):
    transformers = pytest.importorskip("transformers")
    g = golden("ctc_segment_tiny")
    vocab = [str(v) for v in g["vocab"].tolist()]
    (tmp_path / "vocab.json").write_text(json.dumps({tok: i for i, tok in enumerate(vocab)}))
    tok = transformers.Wav2Vec2CTCTokenizer(str(tmp_path / "vocab.json"), unk_token="<unk>", pad_token="<pad>", bos_token="<s>", eos_token="</s>",
                                            word_delimiter_token="|")
    rng = np.random.RandomState(5)
    for i in range(60):
        ids = random_ids(rng, int(rng.randint(1, 200)), *[(.5, .2), (.7, .1), (.1, .4)][i % 3], V=len(vocab))
        got = [(int(w["start_offset"]), int(w["end_offset"])) for w in tok.decode(ids, output_word_offsets=True).word_offsets]
        assert got == ref.words(ids, 0, 4), ids


def test_packed_mode_never_yields_an_empty_or_foreign_pair_and_the_host_packer_accepts_it():
    rng = np.random.RandomState(11)
    for i in range(1000):
        T = int(rng.randint(1, 120))
        ids = random_ids(rng, T, *[(.5, .2), (.8, .1), (.1, .1), (0., .5), (.3, 0.)][i % 5])
        pr = (1, 3, 4, 7)[i % 4]
        words = ref.words(ids)
        tok0 = 1000 * (i % 3)
        packed = ref.packed_ranges(words, T, pr, tok0=tok0)
        assert packed and all(tok0 <= a < b <= tok0 + T for a, b in packed)
        raw = ref.raw_ranges(words, T, pr)
        assert len(packed) <= len(raw) <= ref.capacity(T) and len(words) <= ref.word_capacity(T)
        if i % 10 == 0:       # the list form `ctc_pool_ranges=` takes: utterance-relative; the host packer clamps nothing further and refuses nothing
            rel = [(a - tok0, b - tok0) for a, b in packed]
            table, counts = ops.segment_ranges_pack([rel, rel], [T, T])
            assert counts == [len(rel)] * 2 and table.tolist() == [list(r) for r in rel] + [[a + T, b + T] for a, b in rel]


@pytest.mark.parametrize("T", [1, 2, 7, 8, 63, 64, 65, 1500])
def test_worst_case_patterns_stay_within_the_capacity_bound(T):
    """alternating letter / delimiter: ceil(T / 2) one-frame words, each a chunk and a gap, plus the first gap: 2 ceil(T / 2) + 1 ranges, which is the
    bound T + 2 when T is odd (T + 1 when even); one long word with pool_range 1 attains it for every T.  Words: ceil(T / 2) = (T + 1) // 2."""
    lib = L.lib()
    assert ref.capacity(T) == lib.sl_ctc_pool_ranges_capacity(T, 1) and ref.word_capacity(T) == lib.sl_ctc_words_capacity(T, 1)
    alternating = [7 if i % 2 == 0 else 4 for i in range(T)]
    w = ref.words(alternating)
    assert len(w) == (T + 1) // 2 == ref.word_capacity(T)                                   # the word bound is attained
    assert len(ref.raw_ranges(w, T, 4)) == 2 * ((T + 1) // 2) + 1 <= ref.capacity(T)
    if T % 2:
        assert len(ref.raw_ranges(w, T, 4)) == ref.capacity(T)                              # attained
    letters = [7] * T
    assert ref.words(letters) == [(0, T)]
    for pr in (1, 4):
        n = len(ref.raw_ranges([(0, T)], T, pr))
        assert n == 2 + -(-T // pr) <= ref.capacity(T)
    assert len(ref.raw_ranges([(0, T)], T, 1)) == ref.capacity(T)                           # attained for every T
    long_word = [0, 7] + [0] * (T - 3) + [9] if T >= 3 else letters                         # one word held open by blanks
    assert len(ref.raw_ranges(ref.words(long_word), T, 4)) <= ref.capacity(T)


def test_inference_class_without_a_segmenter_has_no_get_ctc_pool_ranges():
    cls = inf_mod.LLMSpeechTextInference
    assert not hasattr(cls, "get_ctc_pool_ranges")
    inf = object.__new__(cls)
    inf.ctc_segmenter = None
    assert not hasattr(inf, "get_ctc_pool_ranges")
    with pytest.raises(AttributeError, match="'LLMSpeechTextInference' object has no attribute 'get_ctc_pool_ranges'"):
        inf.get_ctc_pool_ranges(torch.zeros(1, 16000))

    class Stub:
        def pool_ranges(self, audios, pool_range=4, raw=False):
            assert len(audios) == 1 and audios[0].shape == (16000,) and not raw
            return [[(0, 4), (4, 49)]]

    inf.ctc_segmenter = Stub()
    assert inf.get_ctc_pool_ranges(torch.zeros(1, 16000)) == [(0, 4), (4, 49)]            # the name ref:inference.py:100-105 calls
