"""LLMSpeechTextInference: drop-in mirror of ref:inference.py:18-137 on the HIP path.

Same constructor signature, attributes (`config, device, audio_encoder, llm_type, llm_tokenizer,
prompt_prefix, prompt_suffix, llm`) and methods (`generate_llm_response`, `generate_text_response`,
`generate_audio_response`) with the reference's order of operations:
    audio -> AudioEncoder -> [text[1:] | audio] -> [prefix | . | suffix[1:]] -> greedy generate -> decode.
Optional keyword arguments (`tokenizer`, `llm`, `dtype`) let callers inject a tokenizer object or
already-built models where hub downloads are impossible; when omitted the reference's loading path
(local checkpoint directory named by `config.model.llm_type`) is followed.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch

from . import _lib as L
from .audio_encoder import AudioEncoder
from .audio_llama import AudioLlamaForCausalLM
from .utils import (LLAMA_PROMPT_PREFIX, LLAMA_PROMPT_SUFFIX, MINICHAT_PROMPT_PREFIX, MINICHAT_PROMPT_SUFFIX,
                    merge_prompt_tokens)


class LLMSpeechTextInference():
    def __init__(self, config, audio_encoder_checkpoint, device, *, tokenizer=None, llm: Optional[AudioLlamaForCausalLM] = None,
                 audio_encoder: Optional[AudioEncoder] = None, dtype: torch.dtype = torch.bfloat16, kv_cache_dtype=None, weight_dtype=None,
                 ctc_segmenter=None, linear_dtype=None):
        self.config = config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SpeechLLMError("LLMSpeechTextInference runs on the MI355X HIP path only (device must be cuda:N)")
        # libspeechllm launches on the CURRENT HIP device and stream: a `-g N` run must not execute cuda:N's pointers on GPU 0
        torch.cuda.set_device(self.device)

        # Audio encoder (ref:inference.py:24-28): flat state-dict checkpoint, strict load.
        if audio_encoder is None:
            checkpoint = audio_encoder_checkpoint
            if isinstance(checkpoint, str):
                checkpoint = torch.load(checkpoint, map_location="cpu")
            # load_pretrained=False: the checkpoint below overwrites every tensor the reference's constructor would have fetched
            audio_encoder = AudioEncoder(self.config, self.device, dtype=dtype, load_pretrained=False)
            audio_encoder.load_state_dict(checkpoint)
        self.audio_encoder = audio_encoder.eval().to(self.device)

        # Optional CTC segmenter (an extension): a CTCSegmenter, or a HubertForCTC directory named by the keyword or by the yaml key
        # model.audio_encoder.ctc_segmenter.  With one, `ctc_pool` inference works from a waveform alone (get_ctc_pool_ranges exists, the
        # name ref:inference.py:100-105 calls); with none, nothing changes and `ctc_pool` without ranges raises the reference's AttributeError.
        if ctc_segmenter is None:
            ae_cfg = self.config.model.audio_encoder
            ctc_segmenter = ae_cfg.get("ctc_segmenter") if hasattr(ae_cfg, "get") else None
        if isinstance(ctc_segmenter, str):
            from .ctc_segmenter import CTCSegmenter
            ctc_segmenter = CTCSegmenter(ctc_segmenter, self.device, dtype=dtype)
        self.ctc_segmenter = ctc_segmenter

        # Tokenizer (ref:inference.py:31-37).
        self.llm_type = self.config.model.llm_type
        if tokenizer is None:
            from transformers import AutoTokenizer  # host-side text processing only
            tokenizer = AutoTokenizer.from_pretrained(self.llm_type, use_fast=False, padding_side="left")
            tokenizer.pad_token = tokenizer.eos_token
        self.llm_tokenizer = tokenizer

        # ref:inference.py:39-44 tests the substring "llama" in the hub id; a local checkpoint directory is judged by its own
        # name, not by whatever its parent directories are called
        if "llama" in os.path.basename(os.path.normpath(self.llm_type)).lower() or (not os.path.isdir(self.llm_type) and "llama" in self.llm_type.lower()):
            self.prompt_prefix, self.prompt_suffix = LLAMA_PROMPT_PREFIX, LLAMA_PROMPT_SUFFIX
        else:
            self.prompt_prefix, self.prompt_suffix = MINICHAT_PROMPT_PREFIX, MINICHAT_PROMPT_SUFFIX

        # Frozen LLM (ref:inference.py:46-52).
        if llm is None:
            llm = AudioLlamaForCausalLM.from_pretrained(self.llm_type, use_cache=True, torch_dtype=dtype, kv_cache_dtype=kv_cache_dtype, weight_dtype=weight_dtype,
                                                        linear_dtype=linear_dtype)
        elif L.kv_format_code(kv_cache_dtype) != llm.kv_format and kv_cache_dtype is not None:
            raise L.SpeechLLMError("kv_cache_dtype differs from the K/V cache format of the llm that was passed in: construct that llm with the same kv_cache_dtype")
        if llm.weight_format != L.weight_format_code(weight_dtype) and weight_dtype is not None:
            raise L.SpeechLLMError("weight_dtype differs from the decode-weight format of the llm that was passed in: construct that llm with the same weight_dtype")
        if llm.linear_format != L.linear_format_code(linear_dtype) and linear_dtype is not None:
            raise L.SpeechLLMError("linear_dtype differs from the layer-product format of the llm that was passed in: construct that llm with the same linear_dtype")
        self.llm = llm.eval().to(self.device)
        # runtime.num_beams / length_penalty / early_stopping of the config (absent in the shipped yamls: greedy) -> beam search
        from .config import runtime_beams, runtime_logits, runtime_num_return, runtime_warpers
        self.beams = runtime_beams(self.config)
        # runtime.num_return_sequences (absent in the shipped yamls: 1) -> that many SAMPLED answers per utterance, prompt-major
        self.num_return_sequences = runtime_num_return(self.config)
        if self.num_return_sequences > 1 and self.beams:
            raise ValueError("runtime.num_return_sequences > 1 with runtime.num_beams > 1 (beam sampling) is not built")
        # runtime.repetition_penalty / no_repeat_ngram_size / min_new_tokens (absent in the shipped yamls: off) -> HF's logits processors
        self.logits = runtime_logits(self.config)
        # runtime.min_p / typical_p / epsilon_cutoff / eta_cutoff (absent in the shipped yamls: off) -> the llm's generation_config: the sampler's
        # further warpers wherever a call samples
        warpers = runtime_warpers(self.config)
        if warpers:
            AudioLlamaForCausalLM.apply_warper_config(self.llm.generation_config, warpers)

    def __getattr__(self, name):
        # get_ctc_pool_ranges exists only with a segmenter: without one the class has no such attribute, as in the reference
        if name == "get_ctc_pool_ranges" and self.__dict__.get("ctc_segmenter") is not None:
            return self._ctc_pool_ranges_of
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{name}'")

    def _ctc_pool_ranges_of(self, audio_tensor, pool_range: int = 4):
        """get_ctc_pool_ranges(audio_tensor): one utterance ((N,) or (1, N) waveform) -> its list of utterance-relative (start, end) frame
        ranges, clamped to the utterance and without empty pairs: what the encoder's `ctc_pool_ranges=[...]` takes for it."""
        wave = torch.as_tensor(audio_tensor, dtype=torch.float32).reshape(-1)
        return self.ctc_segmenter.pool_ranges([wave], pool_range=pool_range)[0]

    def _logits_for(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens):
        """the config's logits processors, each overridden by a keyword that is not None -> the keywords of llm.generate"""
        d = dict(getattr(self, "logits", None) or {})
        for k, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
            if v is not None:
                d[k] = v
        return d

    def _mean_logprobs(self, ids: torch.Tensor, logprobs: torch.Tensor) -> List[float]:
        """One mean token log-probability per row over its generated length (up to and including the first EOS; pads hold 0.0)."""
        e = self.llm.generation_config.eos_token_id
        eos = list(e) if isinstance(e, (list, tuple)) else ([] if e is None else [e])
        out = []
        for row, lp in zip(ids.tolist(), logprobs.tolist()):
            n = next((i + 1 for i, tok in enumerate(row) if tok in eos), len(row))
            out.append(sum(lp[:n]) / max(n, 1))
        return out

    def _num_return(self, num_return_sequences) -> int:
        r = int(getattr(self, "num_return_sequences", 1) if num_return_sequences is None else num_return_sequences)
        if r < 1:
            raise ValueError(f"num_return_sequences={r}: must be >= 1")
        return r

    def generate_llm_response(self, inputs_embeds, max_new_tokens=256, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None,
                              return_scores=False, num_return_sequences=None):
        """return_scores=True: (texts, scores), one mean token log-probability per answer over its generated length (llm.generate with
        output_scores; not with beam search).  num_return_sequences=R > 1 (None: runtime.num_return_sequences): R sampled answers per
        prompt, prompt-major (llm.generate with do_sample=True)."""
        kw = dict(self.beams or {}, **self._logits_for(repetition_penalty, no_repeat_ngram_size, min_new_tokens))
        if self._num_return(num_return_sequences) > 1:
            kw.update(do_sample=True, num_return_sequences=self._num_return(num_return_sequences))
        if return_scores:
            res = self.llm.generate(input_ids=None, inputs_embeds=inputs_embeds, max_new_tokens=max_new_tokens, return_dict_in_generate=True,
                                    output_scores=True, **kw)
            self.last_generate_ids = res.sequences
            texts = self.llm_tokenizer.batch_decode(res.sequences, skip_special_tokens=True, clean_up_tokenization_spaces=True)
            return texts, self._mean_logprobs(res.sequences, res.token_logprobs)
        generate_ids = self.llm.generate(input_ids=None, inputs_embeds=inputs_embeds, max_new_tokens=max_new_tokens, **kw)
        self.last_generate_ids = generate_ids
        return self.llm_tokenizer.batch_decode(generate_ids, skip_special_tokens=True, clean_up_tokenization_spaces=True)

    def generate_text_response(self, input_text, max_new_tokens=256) -> str:
        # note the spaces around the user text (ref:inference.py:78)
        full_text_prompt = f"{self.prompt_prefix} {input_text}{self.prompt_suffix} "
        prompt_input_ids = self.llm_tokenizer(full_text_prompt, return_tensors='pt').input_ids.to(self.device)
        prompt_embeds = self.llm.model.embed_tokens(prompt_input_ids)
        return self.generate_llm_response(inputs_embeds=prompt_embeds, max_new_tokens=max_new_tokens)[0]

    def generate_audio_response(self, audio, additional_text_prompt="", max_new_tokens=256, repetition_penalty=None, no_repeat_ngram_size=None,
                                min_new_tokens=None, return_scores=False, num_return_sequences=None, ctc_pool_ranges=None):
        """num_return_sequences=R > 1 (None: runtime.num_return_sequences): the list of R sampled answers (and, with return_scores, the
        list of their scores) instead of one answer.  ctc_pool_ranges (an extension; the `ctc_pool` downsample only): this utterance's list of
        (start, end) frame ranges, as the dataset's `pool_ranges_4` holds them; without it `ctc_pool` fails as the reference does (Q2) unless a
        ctc_segmenter is set, which then derives them (get_ctc_pool_ranges)."""
        audio_tensor = torch.as_tensor(audio, dtype=torch.float32).unsqueeze(0).to(self.device)
        if self.audio_encoder.downsample_method == "ctc_pool" and ctc_pool_ranges is None:
            # the reference calls self.get_ctc_pool_ranges here, which it never defines: it exists with a ctc_segmenter only
            ctc_pool_ranges = self.get_ctc_pool_ranges(audio_tensor)
        if self.audio_encoder.encoder_base == "whisper":
            audio_embeds = self._whisper_audio_embeds(audio)
        else:
            audio_embeds = self.audio_encoder(audio_tensor, ctc_pool_ranges=None if ctc_pool_ranges is None else [ctc_pool_ranges])

        if len(additional_text_prompt) > 0:  # text prompt goes before the audio, BOS dropped (ref:inference.py:113-122)
            additional_text_input_ids = self.llm_tokenizer(additional_text_prompt, return_tensors='pt').input_ids[:, 1:].to(self.device)
            text_embeds = self.llm.model.embed_tokens(additional_text_input_ids)
            combined_embeds = torch.cat([text_embeds, audio_embeds], dim=1)
        else:
            combined_embeds = audio_embeds

        prompt_emb_sequence = merge_prompt_tokens(inputs_embeds=combined_embeds, tokenizer=self.llm_tokenizer,
                                                  embed_tokens=self.llm.model.embed_tokens, llm_type=self.llm_type,
                                                  device=self.device)
        R = self._num_return(num_return_sequences)
        if return_scores:
            texts, scores = self.generate_llm_response(prompt_emb_sequence, max_new_tokens, repetition_penalty, no_repeat_ngram_size, min_new_tokens, True, R)
            return (texts, scores) if R > 1 else (texts[0], scores[0])
        texts = self.generate_llm_response(prompt_emb_sequence, max_new_tokens, repetition_penalty, no_repeat_ngram_size, min_new_tokens, False, R)
        return texts if R > 1 else texts[0]

    def _whisper_audio_embeds(self, audio) -> torch.Tensor:
        """Whisper base (ref:config/llama3_whisper.yaml).  ref:inference.py:97-107 hands the raw waveform to the Whisper encoder,
        which cannot run; the working order of operations is the trainer's (ref:trainer.py:168-199, 278-291)
        and is what this follows: log-mel of the utterance padded / cut to the 30 s window (sl_whisper_logmel) -> encoder ->
        pool -> projector (sl_whisper_forward) -> crop to compute_num_audio_embeds(n_samples) rows."""
        from .utils import compute_num_audio_embeds
        wave = torch.as_tensor(audio, dtype=torch.float32).reshape(-1)
        sr = int(getattr(getattr(self.config, "audio", None), "sampling_rate", 16000) or 16000)
        feats = self.audio_encoder.feature_extractor([wave], return_tensors="pt", sampling_rate=sr).input_features
        padded = self.audio_encoder(feats)                                    # (1, P_window, llm_dim)
        keep = max(0, min(int(padded.shape[1]), compute_num_audio_embeds(int(wave.numel()), sr=sr)))
        return padded[:, :keep]

    def generate_audio_responses(self, audios, additional_text_prompts=None, max_new_tokens=256, repetition_penalty=None, no_repeat_ngram_size=None,
                                 min_new_tokens=None, return_scores=False, num_return_sequences=None, ctc_pool_ranges=None):
        """return_scores=True: (texts, scores), one mean token log-probability per answer; chunks are concatenated in order.
        ctc_pool_ranges (the `ctc_pool` downsample only): one list of (start, end) frame ranges per utterance; without it `ctc_pool` raises the
        reference's AttributeError (Q2) unless a ctc_segmenter is set, which then derives every chunk's ranges on the device.  All three downsample methods take the batched path below.
        num_return_sequences=R > 1 (None: runtime.num_return_sequences): R sampled answers per utterance from one prefill of each
        (generate_packed num_return), returned prompt-major: answer j of utterance i is entry i * R + j.
        Batched form of generate_audio_response (an extension: the reference answers one utterance per call).
        Every utterance is encoded and prefilled at its own length in ONE ragged batch — the encoder writes its embeddings
        straight into the packed prompt buffer `[prefix | text[1:] | audio | suffix[1:]]` — and decoded together, so that the
        weights are streamed once per step for the whole batch; rows that stop early leave the batch (sl_generate's compaction).
        Both encoder bases take this path (Whisper: log-mel of all windows -> one encoder pass -> each utterance's rows cropped to
        compute_num_audio_embeds, the trainer's order of operations ref:trainer.py:168-199,278-291); more utterances than one
        generate call takes (SL_MAX_DECODE_BATCH) are answered in consecutive chunks.  Results equal per-utterance calls (tests)."""
        n = len(audios)
        texts = list(additional_text_prompts) if additional_text_prompts is not None else [""] * n
        if len(texts) != n:
            raise ValueError(f"{len(texts)} text prompts for {n} utterances")
        R = self._num_return(num_return_sequences)
        if R > 1 and self.beams:
            raise L.SpeechLLMError("num_return_sequences > 1 with beam search (beam sampling) is not built")
        ctc = self.audio_encoder.downsample_method == "ctc_pool"
        if ctc and ctc_pool_ranges is None and getattr(self, "ctc_segmenter", None) is None:      # the reference calls an undefined self.get_ctc_pool_ranges
            raise AttributeError("'LLMSpeechTextInference' object has no attribute 'get_ctc_pool_ranges'")      # (with a segmenter every chunk derives its ranges on the device)
        if ctc and ctc_pool_ranges is not None and len(ctc_pool_ranges) != n:
            raise ValueError(f"{len(ctc_pool_ranges)} lists of ctc_pool ranges for {n} utterances")
        out: List[str] = []
        ids_all = []
        scores_all: List[float] = []
        chunk = L.MAX_DECODE_BATCH // (self.beams["num_beams"] if self.beams else R)      # a generate call is sized by its decode ROWS: utterances x beams (or answers)
        if chunk < 1:
            raise L.SpeechLLMError(f"num_return_sequences={R} exceeds the {L.MAX_DECODE_BATCH} decode rows of one generate call")
        for lo_ in range(0, n, chunk):
            ids = self._generate_chunk(audios[lo_:lo_ + chunk], texts[lo_:lo_ + chunk], max_new_tokens,
                                       self._logits_for(repetition_penalty, no_repeat_ngram_size, min_new_tokens), return_scores, R,
                                       ranges=list(ctc_pool_ranges[lo_:lo_ + chunk]) if ctc and ctc_pool_ranges is not None else None)
            if return_scores:
                ids, lps = ids
                scores_all += self._mean_logprobs(ids, lps)
            ids_all.append(ids)
            out += self.llm_tokenizer.batch_decode(ids, skip_special_tokens=True, clean_up_tokenization_spaces=True)
        # one (n, widest chunk) id matrix, pad-filled like a single HF call over the whole list would leave it
        width = max(int(i.shape[1]) for i in ids_all) if ids_all else 0
        pad = self.llm.generation_config.pad_token_id
        if pad is None:
            e = self.llm.generation_config.eos_token_id
            pad = (e[0] if isinstance(e, (list, tuple)) else e) if e else 0
        self.last_generate_ids = torch.cat([torch.nn.functional.pad(i, (0, width - int(i.shape[1])), value=int(pad)) for i in ids_all]) if ids_all else None
        return (out, scores_all) if return_scores else out

    def _generate_chunk(self, audios, texts, max_new_tokens, logits=None, scores=False, num_return=1, ranges=None, session=None, sample=None):
        """One generate call's worth of utterances -> LongTensor (n, n_cols) of new tokens (scores: and their (n, n_cols) log-probabilities).
        num_return = R > 1: (n * R, n_cols), R answers per utterance sampled with the llm's generation_config warpers."""
        x, lens, shared = self._prompt_chunk(audios, texts, ranges)
        skw = {} if session is None else dict(session=session)      # a conversation: the call runs in (and leaves its K/V in) the session's cache
        if num_return > 1:      # several answers are sampled ones: HF's warpers as llm.generate builds them
            g = self.llm.generation_config
            seed, self.llm.sample_seed = self.llm.sample_seed, self.llm.sample_seed + 1
            sample = dict(temperature=float(g.temperature), top_k=int(g.top_k), top_p=float(g.top_p), seed=int(seed), **self._warpers_for())
        if scores:
            ids, n_cols, lps = self.llm.generate_packed(x, lens, max_new_tokens, use_eos=True, shared_prefix=shared, beams=self.beams, logits=logits or None,
                                                        scores=True, sample=sample, num_return=num_return, **skw)
            return ids[:, :n_cols].to(torch.int64), lps[:, :n_cols]
        ids, n_cols = self.llm.generate_packed(x, lens, max_new_tokens, use_eos=True, shared_prefix=shared, beams=self.beams, logits=logits or None,
                                               sample=sample, num_return=num_return, **skw)
        return ids[:, :n_cols].to(torch.int64)

    def _prompt_chunk(self, audios, texts, ranges=None):
        """The packed prompt buffer of a chunk of utterances, `[prefix | text[1:] | audio | suffix[1:]]` per utterance with the encoder's
        embeddings written in place -> (x (sum lens, H), lens, the rows every prompt shares at its head).  What _generate_chunk generates
        from and score_audio_responses scores under."""
        from .utils import compute_num_audio_embeds, prompt_template
        n = len(audios)
        emb = self.llm.model.embed_tokens
        prefix, suffix = prompt_template(self.llm_type)
        pre_e = emb(self.llm_tokenizer(prefix, return_tensors="pt").input_ids.to(self.device))[0]
        suf_e = emb(self.llm_tokenizer(suffix, return_tensors="pt").input_ids.to(self.device))[0, 1:]
        txt_e = [emb(self.llm_tokenizer(t_, return_tensors="pt").input_ids[:, 1:].to(self.device))[0] if len(t_) > 0 else None for t_ in texts]
        waves = [torch.as_tensor(a, dtype=torch.float32).reshape(-1) for a in audios]
        enc = self.audio_encoder
        whisper = enc.encoder_base == "whisper"
        ranges_dev = None
        if whisper:
            sr = int(getattr(getattr(self.config, "audio", None), "sampling_rate", 16000) or 16000)
            feats = enc.feature_extractor(waves, return_tensors="pt", sampling_rate=sr).input_features
            padded = enc(feats)                                                  # (n, P_window, llm_dim): every 30 s window in one pass
            Ps = [max(0, min(int(padded.shape[1]), compute_num_audio_embeds(int(w.numel()), sr=sr))) for w in waves]
        elif enc.downsample_method == "pool":
            Ps = [(enc.arch.num_frames(int(w.numel())) - enc.pool_kernel) // enc.pool_stride + 1 for w in waves]
        elif enc.downsample_method == "stack":
            Ps = [enc.arch.num_frames(int(w.numel())) // enc.downsample_factor for w in waves]
        elif ranges is not None:                                                 # ctc_pool: one embedding per range
            Ps = [len(r) for r in ranges]
        else:                                                                    # ctc_pool from the waveforms alone: the chunk's table on the device
            ranges_dev = self.ctc_segmenter.ranges_packed(waves)
            Ps = list(ranges_dev[1])
        lens, heads = [], []
        for i in range(n):
            n_head = pre_e.shape[0] + (txt_e[i].shape[0] if txt_e[i] is not None else 0)
            heads.append(n_head)
            lens.append(n_head + Ps[i] + suf_e.shape[0])
        starts = [0]
        for ln in lens:
            starts.append(starts[-1] + ln)
        x = torch.empty((starts[-1], pre_e.shape[1]), device=self.device, dtype=self.llm.dtype)
        for i in range(n):
            o = starts[i]
            x[o:o + pre_e.shape[0]] = pre_e
            if txt_e[i] is not None:
                x[o + pre_e.shape[0]:o + heads[i]] = txt_e[i]
            if whisper:
                x[o + heads[i]:o + heads[i] + Ps[i]] = padded[i, :Ps[i]]
            x[o + heads[i] + Ps[i]:starts[i + 1]] = suf_e
        if not whisper:
            enc.encode_packed(waves, out=x, out_row_offsets=[starts[i] + heads[i] for i in range(n)], ctc_pool_ranges=ranges, ctc_pool_ranges_dev=ranges_dev)
        # every prompt opens with the same template rows (and the same instruction text when the caller gave one text for all):
        # the batched decode attention reads those cache positions once for the batch (sl_kv_cache.shared_prefix)
        shared = int(pre_e.shape[0])
        if txt_e[0] is not None and all(t_ == texts[0] for t_ in texts):
            shared += int(txt_e[0].shape[0])
        return x, lens, shared

    # -- teacher-forced scoring of given answers (an extension) ----------------------------------------------------------------------
    def _response_ids(self, responses) -> List[List[int]]:
        """responses as strings -> ids without BOS, the end-of-turn token appended as the model would emit it (its first EOS id); id lists
        (or id tensors) are taken as they are"""
        e = self.llm.generation_config.eos_token_id
        eos = list(e) if isinstance(e, (list, tuple)) else ([] if e is None else [e])
        out = []
        for r in responses:
            if isinstance(r, str):
                ids = [int(v) for v in self.llm_tokenizer(r, add_special_tokens=False).input_ids]
                out.append(ids + [int(eos[0])] if eos else ids)
            else:
                out.append([int(v) for v in (r.reshape(-1).tolist() if torch.is_tensor(r) else r)])
        return out

    @staticmethod
    def _merge_scores(parts):
        from .audio_llama import ScoreOutput
        if len(parts) == 1:
            return parts[0]
        tm = None if parts[0].top1_match is None else [m for p in parts for m in p.top1_match]
        return ScoreOutput([t_ for p in parts for t_ in p.token_logprobs], torch.cat([p.sequence_logprobs for p in parts]),
                           torch.cat([p.n_tokens for p in parts]), tm, set().union(*[p.paths for p in parts]))

    def score_audio_responses(self, audios, responses, additional_text_prompts=None, ctc_pool_ranges=None, return_top1=False):
        """The log-probabilities of given `responses` (strings or id lists, one per utterance) under the prompts generate_audio_responses
        builds for `audios`: the same template, the same encoder pass, in chunks -> the llm's ScoreOutput (token_logprobs, sequence_logprobs,
        n_tokens, .nll, .perplexity()).  Strings are tokenised without BOS and end with the end-of-turn token."""
        n = len(audios)
        texts = list(additional_text_prompts) if additional_text_prompts is not None else [""] * n
        if len(texts) != n or len(responses) != n:
            raise ValueError(f"{len(texts)} text prompts and {len(responses)} responses for {n} utterances")
        ctc = self.audio_encoder.downsample_method == "ctc_pool"
        if ctc and ctc_pool_ranges is None and getattr(self, "ctc_segmenter", None) is None:
            raise AttributeError("'LLMSpeechTextInference' object has no attribute 'get_ctc_pool_ranges'")
        if ctc and ctc_pool_ranges is not None and len(ctc_pool_ranges) != n:
            raise ValueError(f"{len(ctc_pool_ranges)} lists of ctc_pool ranges for {n} utterances")
        targets = self._response_ids(responses)
        parts = []
        for lo_ in range(0, n, L.MAX_DECODE_BATCH):
            hi_ = min(n, lo_ + L.MAX_DECODE_BATCH)
            x, lens, _ = self._prompt_chunk(audios[lo_:hi_], texts[lo_:hi_], list(ctc_pool_ranges[lo_:hi_]) if ctc and ctc_pool_ranges is not None else None)
            prompts, o = [], 0
            for ln in lens:
                prompts.append(x[o:o + ln])
                o += ln
            parts.append(self.llm.score(prompts, targets[lo_:hi_], return_top1=return_top1))
        return self._merge_scores(parts)

    def score_text_responses(self, texts, responses, return_top1=False):
        """score_audio_responses for the text prompt generate_text_response builds: `{prefix} {text}{suffix} ` per input text"""
        if len(texts) != len(responses):
            raise ValueError(f"{len(responses)} responses for {len(texts)} texts")
        emb = self.llm.model.embed_tokens
        prompts = [emb(self.llm_tokenizer(f"{self.prompt_prefix} {t_}{self.prompt_suffix} ", return_tensors='pt').input_ids.to(self.device))[0] for t_ in texts]
        return self.llm.score(prompts, self._response_ids(responses), return_top1=return_top1)

    # -- conversations: follow-up questions about the same recordings (an extension) -------------------------------------------------
    def _warpers_for(self, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        """the generation_config's min_p / typical_p / epsilon_cutoff / eta_cutoff, each overridden by a keyword that is not None -> the
        optional keys of generate_packed's `sample` dict (checked here: a value out of range raises before any device work)"""
        g = self.llm.generation_config
        given = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        d = {k: (getattr(g, k, None) if v is None else v) for k, v in given.items()}
        L.warp_opts(d)
        return d

    def _sample_for(self, do_sample=None, temperature=None, top_k=None, top_p=None, seed=None, min_p=None, typical_p=None, epsilon_cutoff=None,
                    eta_cutoff=None):
        """HF's sampling keywords -> the `sample` dict of generate_packed (None: greedy), as llm.generate builds it"""
        g = self.llm.generation_config
        if not bool(g.do_sample if do_sample is None else do_sample):
            return None
        if seed is None:
            seed, self.llm.sample_seed = self.llm.sample_seed, self.llm.sample_seed + 1
        return dict(temperature=float(g.temperature if temperature is None else temperature), top_k=int(g.top_k if top_k is None else top_k),
                    top_p=float(g.top_p if top_p is None else top_p), seed=int(seed), **self._warpers_for(min_p, typical_p, epsilon_cutoff, eta_cutoff))

    def start_conversation(self, audios, additional_text_prompts=None, max_new_tokens=256, repetition_penalty=None, no_repeat_ngram_size=None,
                           min_new_tokens=None, return_scores=False, ctc_pool_ranges=None, **sampling):
        """generate_audio_responses that KEEPS what it computed: -> (texts, conversation).  The utterances are answered in one batch whose K/V
        stays in a session of the llm (llm.new_session), and conversation.ask(texts) then answers a follow-up question per utterance for the
        cost of the new rows alone — no second pass over the audio prompt or the first answer.  One generate call's worth of utterances
        (SL_MAX_DECODE_BATCH); greedy or sampled (do_sample / temperature / top_k / top_p / seed / min_p / typical_p / epsilon_cutoff / eta_cutoff), never beams or several answers.
        return_scores: ((texts, scores), conversation)."""
        n = len(audios)
        texts = list(additional_text_prompts) if additional_text_prompts is not None else [""] * n
        if len(texts) != n:
            raise ValueError(f"{len(texts)} text prompts for {n} utterances")
        if self.beams or self._num_return(None) > 1:
            raise L.SpeechLLMError("a conversation continues one greedy or sampled answer per utterance: beam search and num_return_sequences > 1 are not built with it")
        if n > L.MAX_DECODE_BATCH:
            raise L.SpeechLLMError(f"{n} utterances in one conversation; a generate call takes {L.MAX_DECODE_BATCH}")
        ctc = self.audio_encoder.downsample_method == "ctc_pool"
        if ctc and ctc_pool_ranges is None and getattr(self, "ctc_segmenter", None) is None:
            raise AttributeError("'LLMSpeechTextInference' object has no attribute 'get_ctc_pool_ranges'")
        conv = Conversation(self, self.llm.new_session(n))
        res = self._generate_chunk(audios, texts, max_new_tokens, self._logits_for(repetition_penalty, no_repeat_ngram_size, min_new_tokens), return_scores, 1,
                                   ranges=list(ctc_pool_ranges) if ctc and ctc_pool_ranges is not None else None, session=conv.session,
                                   sample=self._sample_for(**sampling))
        return conv._decode(res, return_scores), conv


class Conversation:
    """What LLMSpeechTextInference.start_conversation returns beside the first answers: the llm's KVSession of the batch and `ask`."""

    def __init__(self, owner: LLMSpeechTextInference, session):
        self.owner, self.session = owner, session
        self.last_generate_ids = None

    def _decode(self, res, return_scores):
        o = self.owner
        ids, lps = res if return_scores else (res, None)
        self.last_generate_ids = o.last_generate_ids = ids
        texts = o.llm_tokenizer.batch_decode(ids, skip_special_tokens=True, clean_up_tokenization_spaces=True)
        return (texts, o._mean_logprobs(ids, lps)) if return_scores else texts

    def follow_up_ids(self, texts) -> List[torch.Tensor]:
        """One id row per utterance: utils.follow_up_prompt tokenised without BOS; where the pending token already is an EOS / eot id the
        template's leading eot is dropped, so that it is not fed twice."""
        from .utils import follow_up_ids
        o = self.owner
        e = o.llm.generation_config.eos_token_id
        eos = set(e if isinstance(e, (list, tuple)) else ([] if e is None else [e]))
        return [follow_up_ids(o.llm_tokenizer, o.llm_type, t_, drop_eot=p in eos) for t_, p in zip(texts, self.session.pending_id)]

    def ask(self, texts, max_new_tokens=256, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, return_scores=False, **sampling):
        """One follow-up question per utterance (a string for all, or a list) -> the answers (return_scores: (texts, scores))."""
        o, n = self.owner, self.session.n_seq
        texts = [texts] * n if isinstance(texts, str) else list(texts)
        if len(texts) != n:
            raise ValueError(f"{len(texts)} questions for a conversation of {n} utterances")
        rows = [o.llm.model.embed_tokens(i.to(o.device)) for i in self.follow_up_ids(texts)]
        x = torch.cat(rows, 0).to(o.llm.dtype).contiguous()
        logits = o._logits_for(repetition_penalty, no_repeat_ngram_size, min_new_tokens) or None
        out = o.llm.generate_packed(x, [int(r.shape[0]) for r in rows], max_new_tokens, use_eos=True, logits=logits, scores=bool(return_scores),
                                    sample=o._sample_for(**sampling), session=self.session)
        n_cols = out[1]
        ids = out[0][:, :n_cols].to(torch.int64)
        return self._decode((ids, out[2][:, :n_cols]) if return_scores else ids, return_scores)
