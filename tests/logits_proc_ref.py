"""HF's three logits processors (hf:generation/logits_process.py RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
MinNewTokensLengthLogitsProcessor) restated in plain torch for one row at a time, in the order hf:generation/utils.py
_get_logits_processor applies them.  `hist` is the row's GENERATED tokens (the prompt is embeddings: HF's input_ids start empty)."""
import torch

NEG_INF = float("-inf")


def repetition_penalty(scores: torch.Tensor, hist, p: float) -> torch.Tensor:
    """gather, then scatter: a token that occurs twice is penalised once"""
    out = scores.clone()
    if p == 1.0 or len(hist) == 0:
        return out
    idx = torch.as_tensor(list(hist), dtype=torch.long)
    s = scores[idx]
    out[idx] = torch.where(s < 0, s * torch.tensor(p, dtype=scores.dtype), s / torch.tensor(p, dtype=scores.dtype))
    return out


def banned_ngram_tokens(hist, g: int):
    """tokens that followed an occurrence of the last g - 1 tokens (g = 1: every token of the history)"""
    hist = list(hist)
    n = len(hist)
    if g <= 0 or n < g:
        return []
    prefix = hist[n - g + 1:]
    return sorted({hist[i + g - 1] for i in range(n - g + 1) if hist[i:i + g - 1] == prefix})


def no_repeat_ngram(scores: torch.Tensor, hist, g: int) -> torch.Tensor:
    out = scores.clone()
    banned = banned_ngram_tokens(hist, g)
    if banned:
        out[torch.as_tensor(banned, dtype=torch.long)] = NEG_INF
    return out


def min_new_tokens(scores: torch.Tensor, hist, min_new: int, eos) -> torch.Tensor:
    out = scores.clone()
    if len(hist) < min_new and len(eos) > 0:
        out[torch.as_tensor(list(eos), dtype=torch.long)] = NEG_INF
    return out


def process_row(scores: torch.Tensor, hist, p: float = 1.0, g: int = 0, min_new: int = 0, eos=()) -> torch.Tensor:
    return min_new_tokens(no_repeat_ngram(repetition_penalty(scores, hist, p), hist, g), hist, min_new, eos)


def process(scores: torch.Tensor, hists, p: float = 1.0, g: int = 0, min_new: int = 0, eos=()) -> torch.Tensor:
    """scores (rows, V); hists: one token list per row"""
    return torch.stack([process_row(scores[r], hists[r], p, g, min_new, eos) for r in range(scores.shape[0])])


def has_repeated_ngram(tokens, g: int) -> bool:
    tokens = list(tokens)
    seen = set()
    for i in range(len(tokens) - g + 1):
        k = tuple(tokens[i:i + g])
        if k in seen:
            return True
        seen.add(k)
    return False
