"""Pure-Python restatement of the CTC segmentation: greedy ids -> words -> pool ranges (raw and packed).

Words: HF's Wav2Vec2CTCTokenizer word offsets (group_tokens=True, skip_special_tokens=False) without the run-length detour: inside every
maximal stretch of frames that holds no delimiter, [first non-blank frame, last non-blank frame + 1); a stretch without a non-blank
frame has no word; every id other than blank / delimiter is a letter.  Ranges: ref:preprocess_data/utils.py:155-188.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

Pair = Tuple[int, int]


def words(ids: Sequence[int], blank_id: int = 0, delim_id: int = 4) -> List[Pair]:
    out: List[Pair] = []
    first = last = None
    for t, v in enumerate(list(ids) + [delim_id]):      # the end of the utterance closes a word like a delimiter
        if v == delim_id:
            if first is not None:
                out.append((first, last + 1))
            first = last = None
        elif v != blank_id:
            if first is None:
                first = t
            last = t
    return out


def raw_ranges(word_list: Sequence[Pair], T: int, pool_range: int = 4) -> List[Pair]:
    """The list the reference's get_hubert_ctc_pool_ranges stores: utterance-relative, unclamped, empty pairs kept.  No word: [(0, T)]."""
    if not word_list:
        return [(0, T)]
    out: List[Pair] = [(0, word_list[0][0])]
    for i, (s, e) in enumerate(word_list):
        a = s
        while a < e:
            out.append((a, a + pool_range))
            a += pool_range
        out.append((e, word_list[i + 1][0]) if i + 1 < len(word_list) else (e, e + 2 * pool_range))
    return out


def packed_ranges(word_list: Sequence[Pair], T: int, pool_range: int = 4, tok0: int = 0) -> List[Pair]:
    """raw_ranges clamped to [0, T), pairs that are empty afterwards dropped, tok0 added."""
    out = []
    for a, b in raw_ranges(word_list, T, pool_range):
        a, b = min(max(a, 0), T), min(max(b, 0), T)
        if b > a:
            out.append((a + tok0, b + tok0))
    return out


def capacity(T: int) -> int:
    """The stated bound on the number of ranges of an utterance of T frames (include/speechllm.h): T + 2."""
    return T + 2


def word_capacity(T: int) -> int:
    return (T + 1) // 2
