"""AudioLlamaForCausalLM: host-side mirror of ref:model/audio_llama.py:18-113 driving the HIP Llama path.

Surface kept from the reference / HF base class it inherits: `from_pretrained(path, use_cache=True,
torch_dtype=...)`, `.model.embed_tokens(ids)`, `.forward(inputs_embeds=, attention_mask=, labels=,
output_hidden_states=)` -> object with `.logits/.hidden_states/.loss`, `.generate(input_ids=None,
inputs_embeds=, max_new_tokens=)` -> LongTensor(B, n_new) of NEW tokens only (the prompt is embeddings:
hf:generation/utils.py:736-744), `.eval()`, `.to(device)`, `.parameters()`.

RMSNorm, RoPE, GQA attention, SwiGLU, lm_head, argmax, EOS handling and the KV cache all run in
libspeechllm (sl_llama_prefill / sl_generate); generation is greedy by construction
(SURVEY.md §9 Q3).  `generate` also takes HF's `repetition_penalty`, `no_repeat_ngram_size` and
`min_new_tokens` (sl_logits_process, off by default).  No PyTorch fallback exists.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import ops
from .weights import KNOWN_LLAMA, LlamaArch, LlamaDeviceWeights, format_unsupported


class GenerateOutput:
    """What generate(return_dict_in_generate=True) returns (HF's GenerateDecoderOnlyOutput, the fields this port fills): `sequences` (rows,
    n_cols) int64; `token_logprobs` (rows, n_cols) float32 with output_scores=True, else None; `sequences_scores` (rows) float32 — beam
    search: HF's sequences_scores; otherwise the sum of a row's token_logprobs when scores are on, else None."""
    __slots__ = ("sequences", "token_logprobs", "sequences_scores")

    def __init__(self, sequences, token_logprobs=None, sequences_scores=None):
        self.sequences, self.token_logprobs, self.sequences_scores = sequences, token_logprobs, sequences_scores


class ScoreOutput:
    """What score() returns: the log-probabilities of GIVEN answers (teacher forcing).
      token_logprobs      list of float32 (n_b,) tensors: log_softmax(logits)[target] per position, 0.0 at an ignored position (id < 0)
      sequence_logprobs   (B,) float32: the sum over a sequence's counted positions
      n_tokens            (B,) int64: counted (not ignored) positions
      top1_match          list of bool (n_b,) tensors, with return_top1: the target IS the model's first maximum (False at ignored positions)
      paths               set of the lm_head forms the call ran: "rows" (fp32 logits + sl_score_rows) and / or "fused" (the planes)"""
    __slots__ = ("token_logprobs", "sequence_logprobs", "n_tokens", "top1_match", "paths")

    def __init__(self, token_logprobs, sequence_logprobs, n_tokens, top1_match=None, paths=()):
        self.token_logprobs, self.sequence_logprobs, self.n_tokens, self.top1_match, self.paths = token_logprobs, sequence_logprobs, n_tokens, top1_match, set(paths)

    @property
    def nll(self) -> torch.Tensor:
        """(B,) per-sequence mean negative log-probability over the counted positions (nan for a sequence that counts none)"""
        return -self.sequence_logprobs.double() / self.n_tokens.double()

    def perplexity(self) -> float:
        """exp(mean over sequences of nll): the quantity Trainer.validate logs"""
        return float(torch.exp(self.nll.mean()))


def score_plan(prompt_lens: Sequence[int], targets: Sequence[Sequence[int]], max_ctx: int, max_seqs: int, pad_id: int = 0):
    """Host bookkeeping of score(), no device work: sequence b is its P_b prompt rows followed by the embeddings of target[:-1], rows
    [P_b - 1, P_b - 1 + n_b) are scored against target (row P_b - 1 + j predicts target[j]).  Ids < 0 are ignored positions: they stay in the
    labels as they are and feed the pad row as input.  Returns a list of calls of at most max_seqs sequences, each a dict of
    seqs (indices), lens, score_start, n_score, labels (packed, sequence-major) and input_ids (the appended rows' ids, packed).
    Raises SpeechLLMError for an empty target, a prompt of zero rows or a sequence beyond max_ctx."""
    if len(prompt_lens) != len(targets):
        raise L.SpeechLLMError(f"{len(prompt_lens)} prompts for {len(targets)} targets")
    if len(targets) == 0:
        raise L.SpeechLLMError("score needs at least one sequence")
    if int(max_seqs) < 1:
        raise L.SpeechLLMError(f"max_seqs={max_seqs}: a call takes at least one sequence")
    for b, (P, tg) in enumerate(zip(prompt_lens, targets)):
        if int(P) < 1:
            raise L.SpeechLLMError(f"sequence {b}: a prompt of zero rows has no position that predicts the first target token")
        if len(tg) < 1:
            raise L.SpeechLLMError(f"sequence {b}: empty target")
        if int(P) + len(tg) - 1 > int(max_ctx):
            raise L.SpeechLLMError(f"sequence {b}: prompt ({int(P)}) + target ({len(tg)}) - 1 rows exceed max_ctx={int(max_ctx)}")
    calls = []
    for b0 in range(0, len(targets), int(max_seqs)):
        seqs = list(range(b0, min(b0 + int(max_seqs), len(targets))))
        call = dict(seqs=seqs, lens=[], score_start=[], n_score=[], labels=[], input_ids=[])
        for b in seqs:
            tg = [int(v) for v in targets[b]]
            call["lens"].append(int(prompt_lens[b]) + len(tg) - 1)
            call["score_start"].append(int(prompt_lens[b]) - 1)
            call["n_score"].append(len(tg))
            call["labels"] += tg
            call["input_ids"] += [v if v >= 0 else int(pad_id) for v in tg[:-1]]
        calls.append(call)
    return calls


class KVSession:
    """A K/V cache that outlives a generate call: what `llm.new_session(n_seq)` returns and generate(past_key_values=) /
    generate_packed(session=) / forward(use_cache=True, past_key_values=) continue on.  It owns its K and V tensors — n_seq slots at
    the model's max_ctx in the model's kv_format, never the model's shared buffer, so calls without a session leave it alone — and
    the host bookkeeping the library leaves to its caller:
      valid_len[s]   cache positions [0, valid_len[s]) of slot s hold the sequence's K/V; everything above is overwritten next call
      pending_id[s]  the last generated token (EOS, or the last one under the budget): it was selected but never fed back, so the
                     next call's rows begin with its embedding; None before the first call and after a forward()
      shared_prefix  the promise of the FIRST call (positions [0, P) of every slot are equal), which later calls keep reading
    All n_seq sequences take part in every call, in slot order."""

    def __init__(self, n_seq: int, max_ctx: int, kv_format: int = L.KV_MODEL_DTYPE, k: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None):
        if int(n_seq) < 1:
            raise L.SpeechLLMError(f"a session needs at least one sequence, not {n_seq}")
        self.n_seq, self.max_ctx, self.kv_format = int(n_seq), int(max_ctx), int(kv_format)
        self.k, self.v = k, v
        self.valid_len: List[int] = [0] * self.n_seq
        self.pending_id: List[Optional[int]] = [None] * self.n_seq
        self.shared_prefix = 0
        self.turns = 0

    @property
    def fresh(self) -> bool:
        return not any(self.valid_len)

    def get_seq_length(self, s: int = 0) -> int:
        return self.valid_len[s]

    def kv_struct(self) -> "L.KVCache":
        kv = L.KVCache()
        kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx = self.k.data_ptr(), self.v.data_ptr(), self.n_seq, self.max_ctx
        kv.shared_prefix, kv.reserved = int(self.shared_prefix), self.kv_format
        return kv

    def check_room(self, lens: Sequence[int], max_new_tokens: int = 0) -> None:
        """raises, before anything is launched, when a sequence's past + new rows + budget leave the cache"""
        if len(lens) != self.n_seq:
            raise L.SpeechLLMError(f"{len(lens)} sequences for a session of {self.n_seq}: every sequence takes part in every call, in slot order")
        for s, n in enumerate(lens):
            if self.valid_len[s] + int(n) + int(max_new_tokens) > self.max_ctx:
                raise L.SpeechLLMError(f"sequence {s}: past ({self.valid_len[s]}) + prompt ({int(n)}) + max_new_tokens ({int(max_new_tokens)}) exceeds max_ctx={self.max_ctx}")

    def advance(self, lens: Sequence[int], ids=None, eos_ids: Sequence[int] = (), budgets: Optional[Sequence[int]] = None) -> None:
        """Bookkeeping after a call that fed `lens[s]` rows (a prepended pending token counted) and returned the id matrix `ids` (n_seq, cols):
        sequence s generated g_s tokens — up to and including its first EOS, else its budget (budgets[s], or every column); pads are not counted —
        so valid_len = past + len + g - 1 (the last token was selected, not fed) and pending_id = that token.  ids None (a forward()): the rows
        alone, no pending token."""
        if len(lens) != self.n_seq:
            raise L.SpeechLLMError(f"{len(lens)} sequences for a session of {self.n_seq}")
        rows = None if ids is None else (ids.tolist() if hasattr(ids, "tolist") else [list(r) for r in ids])
        if rows is not None and len(rows) != self.n_seq:
            raise L.SpeechLLMError(f"{len(rows)} id rows for a session of {self.n_seq}")
        eos = set(int(e) for e in eos_ids)
        for s in range(self.n_seq):
            if rows is None:
                self.valid_len[s] += int(lens[s])
                self.pending_id[s] = None
                continue
            row = rows[s]
            cap = min(len(row), int(budgets[s])) if budgets is not None else len(row)
            if cap < 1:
                raise L.SpeechLLMError(f"sequence {s}: no generated token to account for")
            g = next((i + 1 for i in range(cap) if int(row[i]) in eos), cap)
            self.valid_len[s] += int(lens[s]) + g - 1
            self.pending_id[s] = int(row[g - 1])
        self.turns += 1


class _EmbedTokens:
    """`llm.model.embed_tokens(ids)` (ref:utils.py:63-64, ref:inference.py:85,121) as a HIP row gather."""

    def __init__(self, owner: "AudioLlamaForCausalLM"):
        self._o = owner

    def __call__(self, ids: torch.Tensor) -> torch.Tensor:
        w = self._o._dev()
        shape = tuple(ids.shape)
        out = ops.embed_gather(w.embed, ids)
        return out.view(*shape, w.arch.hidden_size)

    @property
    def weight(self) -> torch.Tensor:
        return self._o._dev().embed


class AudioLlamaForCausalLM:
    def __init__(self, arch: LlamaArch, state_dict: Dict[str, torch.Tensor], torch_dtype: torch.dtype = torch.bfloat16,
                 device=None, max_ctx: int = 2048, max_batch: int = 16, pack_decode: bool = True, kv_cache_dtype=None, weight_dtype=None,
                 linear_dtype=None):
        # float16 computes in fp16 (the reference's torch_dtype=float16, ref:inference.py:47-51); bfloat16 in bf16; float32 is the
        # exact parity mode.  Logits are fp32 in every mode.
        L.dtype_code(torch_dtype)    # raises for anything else
        # kv_cache_dtype: None = K/V rows in the model dtype; "fp8" / torch.float8_e4m3fn = one OCP e4m3 byte per element (half the
        # bytes the decode attention reads and half the cache; 16-bit models only, results differ from the 16-bit cache's)
        self.kv_format = L.kv_format_code(kv_cache_dtype)
        if self.kv_format == L.KV_FP8_E4M3 and not L.is16(torch_dtype):
            raise L.SpeechLLMError("kv_cache_dtype='fp8' needs a bfloat16 or float16 model: float32 is the parity mode and keeps its K/V cache in float32")
        self.arch = arch
        self.dtype = torch_dtype
        self.pack_decode = pack_decode
        # weight_dtype: None = decode weights in the model dtype; "fp8" / torch.float8_e4m3fn = decode steps of up to sl_w8_max_rows() rows read e4m3
        # weight images (one byte per element, one fp32 scale per output row: half the bytes a small batch streams per token); larger batches
        # and prefill keep the 16-bit weights.  16-bit models only; results differ from the 16-bit weights' (e4m3_dequantised_state_dict).
        # "mxfp4" (alias "fp4") = the same with MXFP4 weight images (e2m1 elements, one e8m0 scale per 32: a quarter of the bytes), up to
        # sl_w4_max_rows() rows; a different model again (mxfp4_dequantised_state_dict).
        self.weight_format = L.WDEC_MODEL_DTYPE
        self.linear_format = L.WDEC_MODEL_DTYPE
        self.set_weight_dtype(weight_dtype)
        # linear_dtype: None = every product in the model dtype; "mx" (alias "mxfp8_mxfp4") = the four products of every decoder layer run as
        # MXFP8 activations x MXFP4 weights on the block-scaled MFMA, in prefill and at every decode batch.  16-bit models only; a
        # different model (mx_dequantised_state_dict + MXFP8 activations); independent of kv_cache_dtype, exclusive with weight_dtype.
        self.set_linear_dtype(linear_dtype)
        self.config = SimpleNamespace(vocab_size=arch.vocab_size, hidden_size=arch.hidden_size,
                                      num_hidden_layers=arch.num_hidden_layers, eos_token_id=list(arch.eos_token_ids),
                                      pad_token_id=arch.pad_token_id, use_return_dict=True)
        # Greedy by default: BASELINE.json's north_star specifies greedy decode (the reference never passes
        # do_sample, so a hub generation_config.json decides; from_pretrained keeps that file's sampling parameters here and its
        # do_sample flag under `hub_do_sample`, but sampling is only used when a caller sets do_sample=True).
        self.generation_config = SimpleNamespace(eos_token_id=list(arch.eos_token_ids), pad_token_id=arch.pad_token_id,
                                                 do_sample=False, temperature=1.0, top_k=50, top_p=1.0, hub_do_sample=None,
                                                 num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                                                 repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
                                                 return_dict_in_generate=False, output_scores=False,
                                                 min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
        self.sample_seed = 0
        self._sd = state_dict
        self.device = torch.device("cpu")
        self.max_ctx, self.max_batch, self.pack_decode = max_ctx, max_batch, pack_decode
        self._w: Optional[LlamaDeviceWeights] = None
        self._kv = None
        self._ws: Optional[torch.Tensor] = None
        self._ws_mx: Optional[torch.Tensor] = None         # linear_dtype='mx' calls' workspace
        self._score_ws: Optional[torch.Tensor] = None      # score()'s own workspace
        self.model =SimpleNamespace(embed_tokens=_EmbedTokens(self))
        self.last_timings_ms = None
        self.last_generate_stats = None
        self.last_beam_scores = None       # beam search: (B * num_return_sequences) float32 sequences_scores of the last call
        self.last_beam_lengths = None      # ... and the hypotheses' lengths (an EOS that ended one is counted)
        self.last_token_logprobs = None    # output_scores=True: (B, n_cols) float32 log-probabilities of the last call's tokens
        if device is not None:
            self.to(device)

    # -- construction ---------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, name_or_path: str, use_cache: bool = True, torch_dtype: torch.dtype = torch.bfloat16, **kw):
        """Local directory with config.json + *.safetensors (HF layout).  Hub ids cannot be fetched
        (no network): a known id without a local directory raises with instructions."""
        if not os.path.isdir(name_or_path):
            raise L.SpeechLLMError(
                f"'{name_or_path}' is not a local directory. Download the checkpoint (config.json + *.safetensors) and pass "
                "its path; hub downloads are not available to this build.")
        with open(os.path.join(name_or_path, "config.json")) as f:
            arch = LlamaArch.from_hf_config(json.load(f))
        from safetensors.torch import load_file
        sd: Dict[str, torch.Tensor] = {}
        for fn in sorted(os.listdir(name_or_path)):
            if fn.endswith(".safetensors"):
                sd.update(load_file(os.path.join(name_or_path, fn)))
        if not sd:
            raise L.SpeechLLMError(f"no *.safetensors files under {name_or_path}")
        obj = cls(arch, sd, torch_dtype=torch_dtype, **kw)
        gc_path = os.path.join(name_or_path, "generation_config.json")
        if os.path.exists(gc_path):
            with open(gc_path) as f:
                gc = json.load(f)
            g = obj.generation_config
            g.temperature, g.top_k, g.top_p = float(gc.get("temperature", 1.0)), int(gc.get("top_k", 50)), float(gc.get("top_p", 1.0))
            g.hub_do_sample = bool(gc.get("do_sample", False))
            cls.apply_warper_config(g, gc)
            if gc.get("eos_token_id") is not None:
                e = gc["eos_token_id"]
                g.eos_token_id = list(e) if isinstance(e, (list, tuple)) else [e]
            if gc.get("pad_token_id") is not None:
                g.pad_token_id = gc["pad_token_id"]
        return obj

    @staticmethod
    def apply_warper_config(g, values: dict) -> None:
        """min_p / typical_p / epsilon_cutoff / eta_cutoff of a generation_config.json (or of the yaml's runtime section) -> `g`; a key
        that is absent or null leaves the field as it is, a value outside its range raises (L.warp_opts)."""
        found = {k: values[k] for k in L.WARP_OFF if values.get(k) is not None}
        L.warp_opts(found)
        for k, v in found.items():
            setattr(g, k, float(v))

    def eval(self):
        return self

    def parameters(self):
        return iter(())  # frozen LLM: no trainable parameters are exposed (ref:trainer.py:63-64)

    def to(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self._w is None:
            self._w = LlamaDeviceWeights(self.arch, self._sd, self.device, self.dtype, rope_len=max(self.max_ctx, 64))
            if self.pack_decode:
                self._w.build_decode_weights()
            for code in (self.weight_format, self.linear_format):
                if code != L.WDEC_MODEL_DTYPE:
                    self._w.build_format(L.WEIGHT_FORMATS[code])
            self._sd = None  # device copy is the only copy from here on (6.4 GB bf16 for Llama-3.2-3B)
        return self

    def set_kv_cache_dtype(self, kv_cache_dtype) -> None:
        """Switch the K/V cache format (None / "fp8" / torch.float8_e4m3fn); the cache buffers of the other format are released."""
        fmt = L.kv_format_code(kv_cache_dtype)
        if fmt == L.KV_FP8_E4M3 and not L.is16(self.dtype):
            raise L.SpeechLLMError("kv_cache_dtype='fp8' needs a bfloat16 or float16 model")
        if fmt != self.kv_format:
            self._kv = None
            self.kv_format = fmt

    def _check_format(self, code: int) -> None:
        """Refuse a weight format this model cannot take, before it is set; build its images where the weights are on the device already.
        weight_dtype and linear_dtype exclude each other; the format's own rules are weights.format_unsupported's."""
        if code == L.WDEC_MODEL_DTYPE:
            return
        fmt = L.WEIGHT_FORMATS[code]
        this, other = ("weight", "linear") if fmt.option == "weight_dtype" else ("linear", "weight")
        if getattr(self, other + "_format", L.WDEC_MODEL_DTYPE) != L.WDEC_MODEL_DTYPE:
            raise L.SpeechLLMError(f"{this}_dtype and {other}_dtype exclude each other: linear_dtype='mx' already runs every layer product on 4-bit weights")
        why = format_unsupported(fmt, self.arch, self.dtype)
        if why:
            raise L.SpeechLLMError(why)
        if fmt.decode_images and not self.pack_decode:
            raise L.SpeechLLMError(f"{fmt.label} needs pack_decode=True: the {fmt.images} weights are decode copies beside the packed 16-bit ones")
        if getattr(self, "_w", None) is not None:
            self._w.build_format(fmt)

    def set_weight_dtype(self, weight_dtype) -> None:
        """Switch the decode-weight format (None / "fp8" / torch.float8_e4m3fn / "mxfp4").  The images are built on first use and kept; which
        struct a call runs is decided per call (_struct_for), and a decode graph captured for one struct is never replayed for another."""
        fmt = L.weight_format_code(weight_dtype)
        self._check_format(fmt)
        self.weight_format = fmt

    def set_linear_dtype(self, linear_dtype) -> None:
        """Switch the layer products between the model dtype (None) and MXFP8 x MXFP4 ("mx", alias "mxfp8_mxfp4").  The MX weight images are built
        on first use and kept; which struct a call runs is decided per call (_struct_for), and a decode graph captured for one struct is never
        replayed for another."""
        fmt = L.linear_format_code(linear_dtype)
        self._check_format(fmt)
        self.linear_format = fmt

    def _struct_for(self, B: int, entry: Optional[str] = None):
        """(model struct, its name) for a call of B sequences: the struct of the format that is switched on, where the batch is within the format's
        row limit (e4m3, MXFP4; MX linears have none) — an entry the format does not run (WeightFormat.refused) raises, it never falls back"""
        w = self._dev()
        for code in (self.linear_format, self.weight_format):
            fmt = L.WEIGHT_FORMATS[code]
            if code == L.WDEC_MODEL_DTYPE:
                continue
            if entry in fmt.refused:
                raise L.SpeechLLMError(f"{fmt.label} does not run {fmt.refused[entry]}: call set_{fmt.option}(None) for it")
            max_rows = fmt.max_rows
            if not max_rows or B <= max_rows:
                return w.format_built(code)[0], fmt.name
        return w.struct, "16-bit" if L.is16(self.dtype) else "float32"

    def _dev(self) -> LlamaDeviceWeights:
        if self._w is None:
            raise L.SpeechLLMError("LLM weights are not on the GPU: call .to('cuda') — the hot path is HIP-only")
        return self._w

    # -- buffers --------------------------------------------------------------------------------
    def _kv_cache(self, slots: int, shared_prefix: int = 0):
        a = self.arch
        if self._kv is None or self._kv[0].shape[1] < slots or self._kv[0].shape[3] != self.max_ctx:
            self._kv = None        # release the smaller cache BEFORE the larger one is allocated (2 048 slots x 448 positions of Llama-3.2-3B: 105 GB)
            shape = (a.num_hidden_layers, slots, a.num_key_value_heads, self.max_ctx, a.head_dim)
            kv_dtype = self.dtype
            if self.kv_format == L.KV_FP8_E4M3:      # e4m3 rows: byte buffers of exactly sl_kv_cache_bytes (the library refuses what it has not built)
                kv_dtype = torch.uint8
                nbytes = ops.kv_cache_bytes(self._dev().struct, slots, self.max_ctx, self.kv_format)
                assert nbytes == shape[0] * shape[1] * shape[2] * shape[3] * shape[4], (nbytes, shape)
            k = torch.zeros(shape, device=self.device, dtype=kv_dtype)
            v = torch.zeros(shape, device=self.device, dtype=kv_dtype)
            self._kv = (k, v)
        k, v = self._kv
        kv = L.KVCache()
        kv.k_cache, kv.v_cache, kv.slots, kv.max_ctx = k.data_ptr(), v.data_ptr(), k.shape[1], self.max_ctx
        kv.shared_prefix = int(shared_prefix)
        kv.reserved = self.kv_format                 # sl_kv_cache.reserved: the K/V format
        return kv

    # -- multi-turn sessions -----------------------------------------------------------------------
    def new_session(self, n_seq: int) -> KVSession:
        """A KVSession of n_seq sequences: its own K / V tensors (n_layers, n_seq, n_kv, max_ctx, D) in this model's kv_format."""
        a = self.arch
        w = self._dev()
        shape = (a.num_hidden_layers, int(n_seq), a.num_key_value_heads, self.max_ctx, a.head_dim)
        kv_dtype = self.dtype
        if self.kv_format == L.KV_FP8_E4M3:
            kv_dtype = torch.uint8
            assert ops.kv_cache_bytes(w.struct, int(n_seq), self.max_ctx, self.kv_format) == shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
        return KVSession(n_seq, self.max_ctx, self.kv_format, torch.zeros(shape, device=self.device, dtype=kv_dtype),
                         torch.zeros(shape, device=self.device, dtype=kv_dtype))

    def _check_session(self, session: KVSession) -> None:
        if not isinstance(session, KVSession):
            raise L.SpeechLLMError(f"past_key_values / session must be a KVSession (llm.new_session(n_seq)), not {type(session).__name__}")
        if session.k is None or session.v is None:
            raise L.SpeechLLMError("the session owns no cache: create it with llm.new_session(n_seq)")
        if session.kv_format != self.kv_format or session.max_ctx != self.max_ctx or session.k.dtype != (torch.uint8 if self.kv_format == L.KV_FP8_E4M3 else self.dtype):
            raise L.SpeechLLMError("the session was created for another kv_cache_dtype, dtype or max_ctx than this model has now")

    def _session_rows(self, session: KVSession, x: torch.Tensor, lens: Sequence[int]):
        """The rows a continued call feeds: each sequence's pending token (selected by the last call, never fed back) in front of its new rows."""
        if session.fresh or all(p is None for p in session.pending_id):
            return x, [int(n) for n in lens]
        if any(p is None for p in session.pending_id):
            raise L.SpeechLLMError("some sequences of the session have a pending token and some have none: they take their turns together")
        pend = self.model.embed_tokens(L.h2d(session.pending_id, torch.int32, self.device)).to(x.dtype)
        parts, o = [], 0
        for s, n in enumerate(lens):
            parts += [pend[s:s + 1], x[o:o + int(n)]]
            o += int(n)
        return torch.cat(parts, 0).contiguous(), [int(n) + 1 for n in lens]

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self.linear_format == L.WDEC_MX_LINEAR:
            # linear_dtype='mx' needs more bytes (the quantised rows): its own buffer, so that the other setting's workspace — and the decode
            # graphs captured on it — are where they were when the option is switched off again
            if self._ws_mx is None or self._ws_mx.numel() < nbytes:
                self._ws_mx = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            return self._ws_mx
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    @staticmethod
    def _pack(inputs_embeds, attention_mask=None):
        """(B,S,h) [+ left-padding mask] or list of (S_i,h)  ->  packed (sum S_i, h), lengths."""
        if torch.is_tensor(inputs_embeds):
            B, S, _ = inputs_embeds.shape
            if attention_mask is None:
                return inputs_embeds.reshape(B * S, -1).contiguous().clone(), [S] * B
            lens = attention_mask.sum(dim=1).tolist()
            rows = [inputs_embeds[b, S - int(n):] for b, n in enumerate(lens)]  # left padding (ref:utils.py:76-82)
            return torch.cat(rows, 0).contiguous(), [int(n) for n in lens]
        return torch.cat(list(inputs_embeds), 0).contiguous(), [int(x.shape[0]) for x in inputs_embeds]

    # -- forward (prefill with all-position logits; training / validation callers) ----------------
    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, labels=None, output_hidden_states=False,
                use_cache=None, past_key_values=None, **unused):
        """use_cache=True with past_key_values=<KVSession> (and neither labels nor output_hidden_states): the rows continue the session's
        sequences (sl_llama_prefill_cont) — a pending token of an earlier generate is fed first — and the result carries the LAST position's
        logits only, (B, 1, vocab), with the session in past_key_values.  Otherwise as ever: all-position logits, past_key_values None."""
        w = self._dev()
        a = self.arch
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        if use_cache and past_key_values is not None and labels is None and not output_hidden_states:
            return self._forward_session(past_key_values, inputs_embeds, attention_mask)
        B, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        x, lens = self._pack(inputs_embeds.to(self.dtype), attention_mask)
        n_tok = x.shape[0]
        if max(lens) > self.max_ctx:
            raise L.SpeechLLMError(f"sequence of {max(lens)} tokens exceeds max_ctx={self.max_ctx}")
        lib = L.lib()
        kv = self._kv_cache(B)
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        cu_c = (C.c_int32 * (B + 1))(*cu)
        struct, _ = self._struct_for(B)      # prefill reads the row-major set of either struct: the same bits
        ws = self._workspace(lib.sl_llama_workspace_bytes(C.byref(struct), n_tok, B))
        last_logits = torch.empty((B, a.vocab_size), device=self.device, dtype=torch.float32)
        ctx = torch.empty(B, device=self.device, dtype=torch.int32)
        taps = torch.empty((a.num_hidden_layers + 1, n_tok, a.hidden_size), device=self.device, dtype=self.dtype)
        L.check(lib.sl_llama_prefill(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, last_logits.data_ptr(), ctx.data_ptr(),
                                     taps.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_prefill")
        # all-position logits from the post-norm hidden state (ref:model/audio_llama.py:67 with num_logits_to_keep=0)
        logits_packed = ops.gemm(taps[-1], w.lm_head, out_f32=True)

        def unpack(t):  # packed (n_tok, C) -> left-padded (B, S, C)
            out = t.new_zeros((B, S, t.shape[-1]))
            for b, n in enumerate(lens):
                out[b, S - n:] = t[cu[b]:cu[b + 1]]
            return out

        logits = unpack(logits_packed)
        hidden_states = tuple(unpack(taps[i]) for i in range(a.num_hidden_layers + 1)) if output_hidden_states else None
        loss = None
        if labels is not None:
            # per-sample response-only next-token CE, batch mean (ref:model/audio_llama.py:72-101): logits[-n:-1] vs labels[1:]
            acc = torch.zeros(1, device=self.device, dtype=torch.float32)
            for b, lab in enumerate(labels):
                lab = lab.reshape(-1).to(self.device)
                n = int(lab.shape[0])
                rows = logits_packed[cu[b + 1] - n: cu[b + 1] - 1]
                ops.ce_loss(rows, lab[1:].to(torch.int32).contiguous(), 1.0 / ((n - 1) * B), acc, None, dtype=self.dtype)
            loss = acc[0]
        return SimpleNamespace(loss=loss, logits=logits, hidden_states=hidden_states, past_key_values=None, attentions=None)

    def _forward_session(self, session: KVSession, inputs_embeds, attention_mask=None):
        self._check_session(session)
        a = self.arch
        x, lens = self._pack(inputs_embeds.to(self.dtype) if torch.is_tensor(inputs_embeds) else [e.to(self.dtype) for e in inputs_embeds], attention_mask)
        x, lens = self._session_rows(session, x, lens)
        session.check_room(lens)
        B = session.n_seq
        lib = L.lib()
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + n)
        cu_c = (C.c_int32 * (B + 1))(*cu)
        past_c = (C.c_int32 * B)(*session.valid_len)
        kv = session.kv_struct()
        struct, _ = self._struct_for(B)
        ws = self._workspace(lib.sl_llama_workspace_bytes(C.byref(struct), x.shape[0], B))
        logits = torch.empty((B, a.vocab_size), device=self.device, dtype=torch.float32)
        ctx = torch.empty(B, device=self.device, dtype=torch.int32)
        L.check(lib.sl_llama_prefill_cont(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, past_c, None, B, logits.data_ptr(), ctx.data_ptr(), ws.data_ptr(),
                                          ws.numel(), L.stream_ptr()), "sl_llama_prefill_cont")
        session.advance(lens)
        return SimpleNamespace(loss=None, logits=logits.view(B, 1, a.vocab_size), hidden_states=None, past_key_values=session, attentions=None)

    __call__ = forward

    # -- teacher-forced scoring -------------------------------------------------------------------
    def _score_slots(self) -> int:
        """sequences one sl_llama_score call takes: the slots of the K/V cache the model already holds (score never replaces it, so a
        generate() after it finds its buffers — and its captured graphs — where they were), max_batch when there is none yet"""
        if self._kv is not None and self._kv[0].shape[3] == self.max_ctx:
            return min(int(self._kv[0].shape[1]), L.MAX_DECODE_BATCH)
        return min(max(1, int(self.max_batch)), L.MAX_DECODE_BATCH)

    def score(self, prompt_embeds, target_ids, *, attention_mask=None, return_top1: bool = False, row_chunk: Optional[int] = None, force_path: int = 0) -> ScoreOutput:
        """Log-probabilities of given answers under given prompts, batched (sl_llama_score).
        prompt_embeds: list of (P_b, H) tensors, or a left-padded (B, S, H) tensor with attention_mask.  target_ids: list of 1-D id tensors
        (or id lists).  Sequence b is its prompt followed by embed_tokens(target[:-1]); rows [P_b - 1, P_b - 1 + n_b) are scored against
        target_b, so token_logprobs[b][j] = log P(target_b[j] | prompt_b, target_b[:j]).  Ids < 0 (HF's -100) are ignored positions: 0.0,
        counted nowhere, their input embedding is the pad row.  Batches beyond the K/V cache's slots (or SL_MAX_DECODE_BATCH) are split
        into consecutive calls.  row_chunk: lm_head rows per pass (None / 0: the library's default); force_path: 0 = the library's rule,
        1 = fp32 logits everywhere, 2 = the fused planes wherever a pass has more than 64 rows.  An empty target, a prompt of zero rows or
        a sequence beyond max_ctx raises before any device work.  No generation state, captured graph or session is touched; the
        model's K/V cache is overwritten in slots [0, B) as by any prefill."""
        if torch.is_tensor(prompt_embeds):
            if prompt_embeds.dim() != 3:
                raise L.SpeechLLMError("prompt_embeds must be a list of (P_b, H) tensors or a (B, S, H) tensor")
            Bp, S, _ = prompt_embeds.shape
            if attention_mask is None:
                prompts = [prompt_embeds[b] for b in range(Bp)]
            else:
                plens = attention_mask.sum(dim=1).tolist()
                prompts = [prompt_embeds[b, S - int(n):] for b, n in enumerate(plens)]      # left padding (ref:utils.py:76-82)
        else:
            prompts = list(prompt_embeds)
        targets = [tg.reshape(-1).tolist() if torch.is_tensor(tg) else [int(v) for v in tg] for tg in target_ids]
        chunk = 0 if row_chunk is None else int(row_chunk)
        if chunk < 0:
            raise L.SpeechLLMError(f"row_chunk={row_chunk}: must be >= 0 (0 / None = the library's default)")
        if int(force_path) not in (0, 1, 2):
            raise L.SpeechLLMError(f"force_path={force_path}: 0 (rule), 1 (fp32 logits) or 2 (fused)")
        pad = self.generation_config.pad_token_id
        calls = score_plan([int(p.shape[0]) for p in prompts], targets, self.max_ctx, self._score_slots(), 0 if pad is None else int(pad))
        self._dev()
        a = self.arch
        lib = L.lib()
        opts = L.ScoreOpts()
        opts.row_chunk, opts.force_path = chunk, int(force_path)
        token_lps, seq_sums, seq_counts, matches, paths = [], [], [], [], set()
        for call in calls:
            nseq, n_rows = len(call["seqs"]), len(call["labels"])
            emb = self.model.embed_tokens(L.h2d(call["input_ids"], torch.int32, self.device)).to(self.dtype) if call["input_ids"] else None
            parts, o = [], 0
            for i, b in enumerate(call["seqs"]):
                parts.append(prompts[b].to(self.device, self.dtype))
                k = call["n_score"][i] - 1
                if k:
                    parts.append(emb[o:o + k])
                    o += k
            x = torch.cat(parts, 0).contiguous() if len(parts) > 1 else parts[0].contiguous().clone()      # the library overwrites x
            cu = [0]
            for n in call["lens"]:
                cu.append(cu[-1] + n)
            cu_c = (C.c_int32 * (nseq + 1))(*cu)
            start_c, ns_c = (C.c_int32 * nseq)(*call["score_start"]), (C.c_int32 * nseq)(*call["n_score"])
            labels = L.h2d(call["labels"], torch.int32, self.device)
            kv = self._kv_cache(max(nseq, self._score_slots()))
            struct, _ = self._struct_for(nseq, "score")      # the layers read the row-major set of either struct
            nbytes = lib.sl_llama_score_workspace_bytes(C.byref(struct), x.shape[0], nseq, n_rows, C.byref(opts))
            if nbytes == 0:
                L.check(-1, "sl_llama_score_workspace_bytes")
            if self._score_ws is None or self._score_ws.numel() < nbytes:      # its own buffer: generate()'s workspace stays where its graphs expect it
                self._score_ws = None
                self._score_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            ws = self._score_ws
            lp = torch.empty(n_rows, device=self.device, dtype=torch.float32)
            top1 = torch.empty(n_rows, device=self.device, dtype=torch.int32) if return_top1 else None
            ssum = torch.empty(nseq, device=self.device, dtype=torch.float32)
            scnt = torch.empty(nseq, device=self.device, dtype=torch.int32)
            shit = torch.empty(nseq, device=self.device, dtype=torch.int32)
            L.check(lib.sl_llama_score(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, nseq, start_c, ns_c, labels.data_ptr(), lp.data_ptr(), L.ptr(top1),
                                       ssum.data_ptr(), scnt.data_ptr(), shit.data_ptr(), C.byref(opts), ws.data_ptr(), ws.numel(), L.stream_ptr()), "sl_llama_score")
            bits = int(lib.sl_llama_score_last_paths())
            paths |= {name for bit, name in ((L.SCORE_PATH_ROWS, "rows"), (L.SCORE_PATH_FUSED, "fused")) if bits & bit}
            o = 0
            for n in call["n_score"]:
                token_lps.append(lp[o:o + n])
                if return_top1:
                    matches.append((top1[o:o + n] == labels[o:o + n]) & (labels[o:o + n] >= 0))
                o += n
            seq_sums.append(ssum)
            seq_counts.append(scnt)
        return ScoreOutput(token_lps, torch.cat(seq_sums), torch.cat(seq_counts).to(torch.int64), matches if return_top1 else None, paths)

    # -- generation -----------------------------------------------------------------------------
    def generate(self, input_ids=None, inputs_embeds=None, max_new_tokens: int = 256, attention_mask=None, use_eos: bool = True,
                 do_sample: Optional[bool] = None, temperature: Optional[float] = None, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, seed: Optional[int] = None, num_beams: Optional[int] = None,
                 length_penalty: Optional[float] = None, early_stopping=None, num_return_sequences: Optional[int] = None,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None,
                 return_dict_in_generate: Optional[bool] = None, output_scores: Optional[bool] = None, past_key_values: Optional[KVSession] = None,
                 min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                 eta_cutoff: Optional[float] = None, **unused):
        """past_key_values=<KVSession> (llm.new_session(B)): the call runs in the session's cache and CONTINUES it — the prompt rows are the
        new rows only (the follow-up question), the earlier turns are the cache; see generate_packed(session=).  Not with num_beams > 1 or
        num_return_sequences > 1.
        do_sample=True with num_return_sequences=R > 1: R sampled answers per prompt -> (B * R, n_cols), prompt-major as HF returns them
        (sl_generate_n: each prompt is prefilled once); greedy search with R > 1 raises, as in HF.
        num_beams > 1: beam search (hf:generation/utils.py _beam_search, sl_beam_generate) -> (B * num_return_sequences, n_cols),
        n_cols the longest returned hypothesis; `last_beam_scores` / `last_beam_lengths` hold HF's sequences_scores and the lengths.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens: HF's logits processors (sl_logits_process) over the GENERATED tokens, in
        every mode; None falls back to `generation_config` (HF's defaults 1.0 / 0 / 0 = off: the call is then exactly the call without them).
        return_dict_in_generate / output_scores (None: `generation_config`): with return_dict_in_generate a GenerateOutput(sequences,
        token_logprobs, sequences_scores) comes back instead of the tensor.  token_logprobs (B, n_cols) float32, only with output_scores:
        log_softmax(the scores the selection saw)[chosen token] — HF's compute_transition_scores(normalize_logits=True) — 0.0 at and after
        a row's finish.  sequences_scores: `last_beam_scores` in beam mode, else the per-row sum of token_logprobs when scores are on.
        output_scores without return_dict_in_generate returns the tensor and sets `last_token_logprobs`.  Beam search with output_scores
        raises: per-token scores along beam back-pointers are not built.
        min_p / typical_p / epsilon_cutoff / eta_cutoff: HF's four further warpers behind temperature / top-k / top-p, in HF's order, in the
        device sampler; None falls back to `generation_config` (None / 1.0 / 0.0 / 0.0 = off: the call is then exactly the
        call without them).  A value outside its range raises; without do_sample they are ignored, as temperature is."""
        g = self.generation_config
        ret_dict = bool(getattr(g, "return_dict_in_generate", False) if return_dict_in_generate is None else return_dict_in_generate)
        want_scores = bool(getattr(g, "output_scores", False) if output_scores is None else output_scores)
        logits = self.logits_options(g.repetition_penalty if repetition_penalty is None else repetition_penalty,
                                     g.no_repeat_ngram_size if no_repeat_ngram_size is None else no_repeat_ngram_size,
                                     g.min_new_tokens if min_new_tokens is None else min_new_tokens, max_new_tokens)
        K = int(g.num_beams if num_beams is None else num_beams)
        R = int(g.num_return_sequences if num_return_sequences is None else num_return_sequences)
        sampling = bool(g.do_sample if do_sample is None else do_sample)
        if K < 1:
            raise L.SpeechLLMError(f"num_beams={K}: must be >= 1")
        if K > 1 and sampling:
            raise L.SpeechLLMError("num_beams > 1 with do_sample=True (beam sampling) is not built: use beam search or sampling")
        if R < 1 or (R > K and not (K == 1 and sampling)):
            raise L.SpeechLLMError(f"num_return_sequences={R} outside [1, num_beams={K}]" + (" (greedy search returns one sequence per prompt: several need do_sample=True)" if K == 1 else ""))
        session = past_key_values
        if session is not None and (K > 1 or R > 1):
            raise L.SpeechLLMError("a session continues one answer per sequence: num_beams > 1 and num_return_sequences > 1 are not built with past_key_values")
        skw = {} if session is None else dict(session=session)
        w = self._dev()
        a = self.arch
        if inputs_embeds is None:
            if input_ids is None:
                raise L.SpeechLLMError("generate needs inputs_embeds or input_ids")
            inputs_embeds = self.model.embed_tokens(input_ids)
        x, lens = self._pack(inputs_embeds.to(self.dtype) if torch.is_tensor(inputs_embeds) else [e.to(self.dtype) for e in inputs_embeds],
                             attention_mask)
        if K > 1 and want_scores:
            raise L.SpeechLLMError("output_scores with num_beams > 1 is not built (per-token scores along beam back-pointers); sequences_scores "
                                   "/ last_beam_scores hold the hypotheses' scores")
        if K > 1:
            beams = dict(num_beams=K, num_return_sequences=R, length_penalty=float(g.length_penalty if length_penalty is None else length_penalty),
                         early_stopping=g.early_stopping if early_stopping is None else early_stopping)
            ids, n_cols = self.generate_packed(x, lens, max_new_tokens, use_eos=use_eos, beams=beams, logits=logits)
            seqs = ids[:, :n_cols].to(torch.int64)
            return GenerateOutput(seqs, None, self.last_beam_scores) if ret_dict else seqs
        sample = None
        if sampling:
            # hf:generation/utils.py logits warpers: temperature, top-k (HF default 50), top-p, then one draw per row
            if seed is None:
                seed, self.sample_seed = self.sample_seed, self.sample_seed + 1
            sample = dict(temperature=float(g.temperature if temperature is None else temperature), top_k=int(g.top_k if top_k is None else top_k),
                          top_p=float(g.top_p if top_p is None else top_p), seed=int(seed),
                          min_p=getattr(g, "min_p", None) if min_p is None else min_p,
                          typical_p=getattr(g, "typical_p", None) if typical_p is None else typical_p,
                          epsilon_cutoff=getattr(g, "epsilon_cutoff", None) if epsilon_cutoff is None else epsilon_cutoff,
                          eta_cutoff=getattr(g, "eta_cutoff", None) if eta_cutoff is None else eta_cutoff)
            L.warp_opts({k: sample[k] for k in L.WARP_OFF})      # a value out of range raises here, before any device work
        if not want_scores:
            ids, n_cols = self.generate_packed(x, lens, max_new_tokens, use_eos=use_eos, sample=sample, logits=logits, num_return=R, **skw)
            seqs = ids[:, :n_cols].to(torch.int64)
            return GenerateOutput(seqs, None, None) if ret_dict else seqs
        ids, n_cols, lps = self.generate_packed(x, lens, max_new_tokens, use_eos=use_eos, sample=sample, logits=logits, scores=True, num_return=R, **skw)
        seqs, lps = ids[:, :n_cols].to(torch.int64), lps[:, :n_cols].clone()
        self.last_token_logprobs = lps
        return GenerateOutput(seqs, lps, lps.sum(dim=1)) if ret_dict else seqs      # pads hold 0.0: the sum runs over the row's generated length

    @staticmethod
    def logits_options(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, max_new_tokens: Optional[int] = None) -> Optional[dict]:
        """The `logits` dict of generate_packed from HF's three keywords, None when all are off; a value outside the library's limits
        (speechllm.h sl_logits_opts) raises."""
        p, g, mn = repetition_penalty, no_repeat_ngram_size, min_new_tokens
        if isinstance(p, bool) or not isinstance(p, (int, float)) or p != p or p in (float("inf"), float("-inf")) or p <= 0:
            raise L.SpeechLLMError(f"repetition_penalty={p!r}: must be a finite number > 0 (1.0 = off)")
        if isinstance(g, bool) or not isinstance(g, int) or g < 0:
            raise L.SpeechLLMError(f"no_repeat_ngram_size={g!r}: must be an integer >= 0 (0 = off)")
        if isinstance(mn, bool) or not isinstance(mn, int) or mn < 0:
            raise L.SpeechLLMError(f"min_new_tokens={mn!r}: must be an integer >= 0 (0 = off)")
        if max_new_tokens is not None and mn > int(max_new_tokens):
            raise L.SpeechLLMError(f"min_new_tokens={mn} exceeds max_new_tokens={int(max_new_tokens)}")
        if float(p) == 1.0 and g == 0 and mn == 0:
            return None
        return dict(repetition_penalty=float(p), no_repeat_ngram_size=int(g), min_new_tokens=int(mn))

    @classmethod
    def _logits_struct(cls, logits: Optional[dict], max_new_tokens: int):
        """`logits` dict -> L.LogitsOpts, or None (a NULL pointer: the library then runs exactly the call without processors)"""
        if logits is None:
            return None
        unknown = set(logits) - {"repetition_penalty", "no_repeat_ngram_size", "min_new_tokens"}
        if unknown:
            raise L.SpeechLLMError(f"logits: unknown keys {sorted(unknown)}")
        d = cls.logits_options(logits.get("repetition_penalty", 1.0), logits.get("no_repeat_ngram_size", 0), logits.get("min_new_tokens", 0), max_new_tokens)
        if d is None:
            return None
        lp = L.LogitsOpts()
        lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = d["repetition_penalty"], d["no_repeat_ngram_size"], d["min_new_tokens"]
        return lp

    def _generate_preamble(self, lens, max_new_tokens, use_eos, shared_prefix):
        """What generate_packed and _beam_packed check and build alike: the context and shared-prefix limits, then
        (cu_seqlens, eos ids, n_eos, use_eos, pad) as the library takes them."""
        if max(lens) + max_new_tokens > self.max_ctx:
            raise L.SpeechLLMError(f"prompt ({max(lens)}) + max_new_tokens ({max_new_tokens}) exceeds max_ctx={self.max_ctx}")
        if not 0 <= shared_prefix <= min(lens):
            raise L.SpeechLLMError(f"shared_prefix={shared_prefix} outside [0, shortest prompt={min(lens)}]")
        cu = [0]
        for n in lens:
            cu.append(cu[-1] + int(n))
        cu_c = (C.c_int32 * (len(lens) + 1))(*cu)
        gen = self.generation_config
        eos = list(gen.eos_token_id) if isinstance(gen.eos_token_id, (list, tuple)) else ([] if gen.eos_token_id is None else [gen.eos_token_id])
        pad = gen.pad_token_id if gen.pad_token_id is not None else (eos[0] if eos else 0)
        return cu_c, (C.c_int32 * max(1, len(eos)))(*eos), len(eos), bool(use_eos and len(eos) > 0), pad

    def _record_generate_stats(self, st, rows, fmt_name, **extra):
        self.last_timings_ms = (st.prefill_ms, st.decode_ms)
        self.last_generate_stats = {"rows": rows, "n_steps": int(st.n_steps), "decode_launches": int(st.decode_launches), "compactions": int(st.compactions),
                                    "final_rows": int(st.final_rows), "row_steps": int(st.row_steps), "weight_format": fmt_name, **extra}

    def generate_packed(self, x: torch.Tensor, lens: Sequence[int], max_new_tokens: int, use_eos: bool = True, sample: Optional[dict] = None,
                        shared_prefix: int = 0, row_limits: Optional[Sequence[int]] = None, compact: Optional[bool] = None, check_every: int = 4,
                        beams: Optional[dict] = None, logits: Optional[dict] = None, scores: bool = False, num_return: int = 1,
                        session: Optional[KVSession] = None):
        """x: packed prompt embeddings (sum S_i, h) on the GPU (overwritten).  Returns (int32 (B, max_new) host tensor, n_cols).
        shared_prefix = P: the caller's promise that the first P rows of every sequence are the same rows (one prompt template in
        front of the audio, ref:inference.py:95-113) — the batched decode attention then reads those P cache positions from slot 0
        (sl_kv_cache.shared_prefix); ids and logits are bit for bit those of P = 0.
        row_limits: one token budget per sequence (a per-request max_new_tokens; the row then finishes like a row that emitted EOS).
        compact: with EOS / budgets on, the batch is compacted as its rows finish (sl_generate_opts.compact) — the decode step then
        costs what the LIVE rows cost; per-sequence results are those of the uncompacted batch (`last_generate_stats` has the counts).
        beams: dict(num_beams=K, length_penalty=1.0, early_stopping=False, num_return_sequences=1) -> beam search (sl_beam_generate) on
        B * K decode rows: returns (int32 (B * R, max_new) ids, the longest hypothesis' length) and sets `last_beam_scores` /
        `last_beam_lengths`; not with row_limits or sampling; `compact` is ignored (done sequences keep their rows).
        logits: dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0) -> HF's logits processors over each row's generated
        tokens (sl_generate_lp / sl_beam_generate_lp), in every mode; every step then runs the unfused lm_head -> fp32 logits -> processors
        -> select.  None, or all three off: exactly the call without them.
        scores=True: returns (ids, n_cols, logprobs), logprobs a float32 (B, max_new) host tensor of the chosen tokens' log-probabilities
        (sl_generate_sc; 0.0 at and after a row's finish); above 64 rows a greedy step keeps the fused lm_head top-1 and carries a third
        partial.  Not with beams.  False: exactly the call without them.
        sample: dict(temperature, top_k, top_p, seed) and, optionally, min_p / typical_p / epsilon_cutoff / eta_cutoff (None or the off value
        0 / 1.0 / 0 / 0: off) -> one draw per row and step (sl_generate_w when one of the four is on; a dict without them is the call it was).
        num_return = R > 1 (sampling only): R answers per prompt from ONE prefill (sl_generate_n) -> (B * R, max_new) ids / logprobs,
        prompt-major; row_limits then has B * R entries; the cache holds B prompt slots + B * R row slots.  The draws are those of a call
        on every prompt repeated R times.  `last_generate_stats` has prefill_seqs and attn_path ("copy" / "grouped").
        compact None: True, and False with a session.
        session: a KVSession of len(lens) sequences (sl_generate_cont).  Its first call is this call run uncompacted into the session's cache;
        a later call feeds, per sequence, the embedding of the pending token (the last one generated, never fed back) and then the rows of
        `x`, on top of the valid_len positions the cache holds; valid_len / pending_id are then advanced from the returned ids (up to the
        first EOS or the row's budget, pads not counted).  shared_prefix is the FIRST call's promise and is kept; later calls pass none.
        The logits processors see this call's generated tokens only.  Not with beams or num_return > 1; compact=True raises (compaction
        moves rows into the slots of finished ones and would destroy the K/V the session keeps); a prompt that leaves max_ctx raises
        before anything is launched."""
        R = int(num_return)
        if session is not None:
            self._check_session(session)
            if beams is not None or R > 1:
                raise L.SpeechLLMError("a session continues one answer per sequence: beams and num_return > 1 are not built with it")
            if compact:
                raise L.SpeechLLMError("compact=True with a session: compaction moves live rows into the slots of finished rows and destroys the K/V the session keeps")
            if not session.fresh and shared_prefix:
                raise L.SpeechLLMError("shared_prefix belongs to a session's first call (its promise is kept: session.shared_prefix)")
            x, lens = self._session_rows(session, x, lens)
            session.check_room(lens, max_new_tokens)
        compact = (session is None) if compact is None else bool(compact)
        if R < 1:
            raise L.SpeechLLMError(f"num_return_sequences={R}: must be >= 1")
        if R > 1 and sample is None and beams is None:
            raise L.SpeechLLMError(f"num_return_sequences={R} with greedy search: several answers per prompt need sampling")
        w = self._dev()
        a = self.arch
        lib = L.lib()
        B = len(lens)
        if beams is not None:
            if row_limits is not None:
                raise L.SpeechLLMError("row_limits and beams together are not built: a beam search has one max_new_tokens for the call")
            if sample is not None:
                raise L.SpeechLLMError("sampling and beams together (beam sampling) are not built")
            if scores:
                raise L.SpeechLLMError("scores and beams together are not built: last_beam_scores holds the hypotheses' scores")
            return self._beam_packed(x, lens, max_new_tokens, use_eos, shared_prefix, check_every, beams, logits)
        if B * R > L.MAX_DECODE_BATCH:
            raise L.SpeechLLMError(f"{B * R} sequences in one generate call; the library takes {L.MAX_DECODE_BATCH} (split the batch: sequences are independent)")
        cu_c, eos_c, n_eos, use_eos, pad = self._generate_preamble(lens, max_new_tokens, use_eos, shared_prefix)
        if session is not None:
            if session.fresh:
                session.shared_prefix = int(shared_prefix)
            kv = session.kv_struct()
        else:
            kv = self._kv_cache(B * (R + 1) if R > 1 else B, shared_prefix)
        n_prompts, B = B, B * R      # B: decode rows = rows of every returned array
        out = (C.c_int32 * (B * max_new_tokens))()
        o = L.GenerateOpts()
        # the ids are handed over as configured; with use_eos = 0 the library ignores them (rows then finish on their budgets only)
        o.eos_ids_host, o.n_eos, o.pad_id, o.use_eos = eos_c, n_eos, int(pad), int(use_eos)
        o.max_new_tokens, o.check_every, o.compact = int(max_new_tokens), int(check_every), int(bool(compact))
        lim_c = None
        if row_limits is not None:
            if len(row_limits) != B:
                raise L.SpeechLLMError(f"row_limits has {len(row_limits)} entries for {B} sequences")
            lim_c = (C.c_int32 * B)(*[int(v) for v in row_limits])
            o.row_limits_host = lim_c
        if sample is not None:
            o.sample, o.temperature, o.top_k, o.top_p = 1, float(sample["temperature"]), int(sample["top_k"]), float(sample["top_p"])
            o.seed = int(sample["seed"]) & 0xFFFFFFFFFFFFFFFF
        # min_p / typical_p / epsilon_cutoff / eta_cutoff: None when every one is off, and the calls below are then the ones they were
        wp = None if sample is None else L.warp_opts({k: sample.get(k) for k in L.WARP_OFF})
        st = L.GenerateStats()
        lp = self._logits_struct(logits, max_new_tokens)
        lp_ref = C.byref(lp) if lp is not None else None
        struct, fmt_name = self._struct_for(B, "generate_n" if R > 1 else None)
        lps = None
        if R > 1:
            if scores:
                lps = (C.c_float * (B * max_new_tokens))()
            nbytes = lib.sl_generate_workspace_bytes_n(C.byref(struct), x.shape[0], n_prompts, max_new_tokens, lp_ref, int(bool(scores)), R)
            if nbytes == 0:
                L.check(-1, "sl_generate_workspace_bytes_n")
            ws = self._workspace(nbytes)
            if wp is not None:
                L.check(lib.sl_generate_w(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, n_prompts, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr(), lp_ref, lps, R, None, None, C.byref(wp)), "sl_generate_w")
            else:
                L.check(lib.sl_generate_n(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, n_prompts, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr(), lp_ref, lps, R), "sl_generate_n")
            self._record_generate_stats(st, B, fmt_name, prefill_seqs=n_prompts, num_return_sequences=R,
                                        attn_path={1: "copy", 2: "grouped"}[int(lib.sl_generate_last_attn_path())])
            ids = torch.frombuffer(out, dtype=torch.int32).clone().view(B, max_new_tokens)
            if scores:
                return ids, int(st.n_steps), torch.frombuffer(lps, dtype=torch.float32).clone().view(B, max_new_tokens)
            return ids, int(st.n_steps)
        if session is not None:
            lps = (C.c_float * (B * max_new_tokens))() if scores else None
            past_c = (C.c_int32 * B)(*session.valid_len)
            ws = self._workspace(lib.sl_generate_workspace_bytes_cont(C.byref(struct), x.shape[0], B, max_new_tokens, lp_ref, int(bool(scores))))
            if wp is not None:
                L.check(lib.sl_generate_w(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr(), lp_ref, lps, 1, past_c, None, C.byref(wp)), "sl_generate_w")
            else:
                L.check(lib.sl_generate_cont(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                             L.stream_ptr(), lp_ref, lps, past_c, None), "sl_generate_cont")
            ids = torch.frombuffer(out, dtype=torch.int32).clone().view(B, max_new_tokens)
            gen = self.generation_config
            eos = (list(gen.eos_token_id) if isinstance(gen.eos_token_id, (list, tuple)) else ([] if gen.eos_token_id is None else [gen.eos_token_id])) if use_eos else []
            session.advance(lens, ids, eos, row_limits)
            self._record_generate_stats(st, B, fmt_name, session_turn=session.turns)
            if scores:
                return ids, int(st.n_steps), torch.frombuffer(lps, dtype=torch.float32).clone().view(B, max_new_tokens)
            return ids, int(st.n_steps)
        if wp is not None:      # the workspace is the unwarped call's (speechllm.h)
            lps = (C.c_float * (B * max_new_tokens))() if scores else None
            ws = self._workspace(lib.sl_generate_workspace_bytes_sc(C.byref(struct), x.shape[0], B, max_new_tokens, lp_ref, int(bool(scores))))
            L.check(lib.sl_generate_w(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                      L.stream_ptr(), lp_ref, lps, 1, None, None, C.byref(wp)), "sl_generate_w")
        elif scores:
            lps = (C.c_float * (B * max_new_tokens))()
            ws = self._workspace(lib.sl_generate_workspace_bytes_sc(C.byref(struct), x.shape[0], B, max_new_tokens, lp_ref, 1))
            L.check(lib.sl_generate_sc(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                       L.stream_ptr(), lp_ref, lps), "sl_generate")
        else:
            ws = self._workspace(lib.sl_generate_workspace_bytes_lp(C.byref(struct), x.shape[0], B, max_new_tokens, lp_ref))
            L.check(lib.sl_generate_lp(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, C.byref(st), ws.data_ptr(), ws.numel(),
                                       L.stream_ptr(), lp_ref), "sl_generate")
        self._record_generate_stats(st, B, fmt_name)
        ids = torch.frombuffer(out, dtype=torch.int32).clone().view(B, max_new_tokens)
        if scores:
            return ids, int(st.n_steps), torch.frombuffer(lps, dtype=torch.float32).clone().view(B, max_new_tokens)
        return ids, int(st.n_steps)

    def _beam_packed(self, x, lens, max_new_tokens, use_eos, shared_prefix, check_every, beams, logits=None):
        lib = L.lib()
        B = len(lens)
        unknown = set(beams) - {"num_beams", "length_penalty", "early_stopping", "num_return_sequences"}
        if unknown:
            raise L.SpeechLLMError(f"beams: unknown keys {sorted(unknown)}")
        K, R = int(beams.get("num_beams", 1)), int(beams.get("num_return_sequences", 1))
        if not 1 <= K <= 8:
            raise L.SpeechLLMError(f"num_beams={K} outside [1, 8]")
        if not 1 <= R <= K:
            raise L.SpeechLLMError(f"num_return_sequences={R} outside [1, num_beams={K}]")
        if B * K > L.MAX_DECODE_BATCH:
            raise L.SpeechLLMError(f"{B} sequences x {K} beams = {B * K} decode rows; the library takes {L.MAX_DECODE_BATCH} (split the batch)")
        cu_c, eos_c, n_eos, use_eos, pad = self._generate_preamble(lens, max_new_tokens, use_eos, shared_prefix)
        kv = self._kv_cache(B * K, shared_prefix)
        o = L.BeamOpts()
        o.eos_ids_host, o.n_eos, o.pad_id, o.use_eos = eos_c, n_eos, int(pad), int(use_eos)
        o.max_new_tokens, o.check_every = int(max_new_tokens), int(check_every)
        o.num_beams, o.num_return_sequences = K, R
        o.early_stopping = L.early_stopping_code(beams.get("early_stopping", False))
        o.length_penalty = float(beams.get("length_penalty", 1.0))
        out = (C.c_int32 * (B * R * max_new_tokens))()
        scores = (C.c_float * (B * R))()
        lengths = (C.c_int32 * (B * R))()
        st = L.GenerateStats()
        lp = self._logits_struct(logits, max_new_tokens)
        lp_ref = C.byref(lp) if lp is not None else None
        struct, fmt_name = self._struct_for(B * K, "beam")
        nbytes = lib.sl_beam_generate_workspace_bytes_lp(C.byref(struct), x.shape[0], B, C.byref(kv), C.byref(o), lp_ref)
        if nbytes == 0:
            L.check(-1, "sl_beam_generate_workspace_bytes")
        ws = self._workspace(nbytes)
        L.check(lib.sl_beam_generate_lp(C.byref(struct), C.byref(kv), x.data_ptr(), cu_c, B, C.byref(o), out, scores, lengths, C.byref(st), ws.data_ptr(),
                                        ws.numel(), L.stream_ptr(), lp_ref), "sl_beam_generate")
        self._record_generate_stats(st, B * K, fmt_name, num_beams=K)
        self.last_beam_scores = torch.frombuffer(scores, dtype=torch.float32).clone()
        self.last_beam_lengths = torch.frombuffer(lengths, dtype=torch.int32).clone()
        ids = torch.frombuffer(out, dtype=torch.int32).clone().view(B * R, max_new_tokens)
        return ids, int(self.last_beam_lengths.max())
