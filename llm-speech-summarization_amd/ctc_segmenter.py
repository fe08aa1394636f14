"""CTCSegmenter: the reference's ctc_pool preprocessing (ref:preprocess_data/utils.py:127-188) on the device, for ragged batches.

The reference's recipe runs a fine-tuned `HubertForCTC` at batch size 1, takes the argmax of its logits, asks
`Wav2Vec2CTCTokenizer.decode(output_word_offsets=True)` for the word offsets and turns them into `pool_ranges_4` in a Python loop.  Here
the same steps run on packed frames of any number of utterances:

    waveforms -> sl_hubert_forward (frames only: last_hidden)          the existing encoder, no new encoder code
              -> sl_ctc_greedy_batch (lm_head + argmax fused)          ids, the logits are never written
              -> sl_ctc_pool_ranges_batch (ids -> words -> ranges)      a device table sl_hubert_forward_ds takes as it is

A segmenter is a SECOND full HuBERT next to the AudioEncoder's: the reference segments with a separate fine-tuned CTC model
(hubert-large-ls960-ft), whose weights are not the speech-LLM encoder's.

Divergences from the reference, both in DESIGN.md section 3.9:
  * packed mode (the default) clamps every pair to its utterance and drops the pairs that are empty afterwards (the reference stores them and
    its encoder would average nothing into a NaN row); raw mode returns the reference's list exactly;
  * an utterance without a word gives the one range (0, T) (the reference raises IndexError on `ctc_word_offsets[0]`).
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L
from . import config as cfgm
from . import ops
from .audio_encoder import AudioEncoder
from .weights import HubertArch, read_hf_weight_files, resolve_pretrained_dir

_DUMMY_PROJ = 8      # rows of the unused embed_projection the wrapped AudioEncoder's weight table asks for


class CTCSegmenter:
    def __init__(self, path_or_arch: Union[str, HubertArch], device, dtype: torch.dtype = torch.bfloat16,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, blank_id: Optional[int] = None, delim_id: Optional[int] = None):
        """path_or_arch: a `HubertForCTC` checkpoint directory (config.json + weights with `hubert.*` and `lm_head.{weight,bias}` keys, and
        optionally vocab.json), a hub id whose snapshot is in the local HF cache, or a HubertArch together with `state_dict` in that key layout.
        blank_id / delim_id: the ids of `<pad>` and `|` in vocab.json, else 0 / 4 (the ls960-ft vocabulary), unless given."""
        self.device = torch.device(device)
        self.dtype = dtype
        self.path = None
        vocab_blank = vocab_delim = None
        if isinstance(path_or_arch, HubertArch):
            arch = path_or_arch
            if state_dict is None:
                raise L.SpeechLLMError("CTCSegmenter(arch, ...) needs state_dict=: `hubert.*` plus `lm_head.weight` / `lm_head.bias`")
        else:
            local = resolve_pretrained_dir(str(path_or_arch))
            if local is None or not os.path.exists(os.path.join(local, "config.json")):
                raise L.SpeechLLMError(f"CTC segmenter '{path_or_arch}': need a local HubertForCTC directory with config.json (there is no network)")
            with open(os.path.join(local, "config.json")) as f:
                arch = HubertArch.from_hf_config(json.load(f))
            if state_dict is None:
                state_dict = read_hf_weight_files(local)
                if state_dict is None:
                    raise L.SpeechLLMError(f"{local}: no weight files (model.safetensors / pytorch_model.bin)")
            vocab = os.path.join(local, "vocab.json")
            if os.path.exists(vocab):
                with open(vocab) as f:
                    v = json.load(f)
                vocab_blank, vocab_delim = v.get("<pad>"), v.get("|")
            self.path = local
        self.arch = arch
        self.blank_id = int(blank_id if blank_id is not None else (vocab_blank if vocab_blank is not None else 0))
        self.delim_id = int(delim_id if delim_id is not None else (vocab_delim if vocab_delim is not None else 4))
        if self.blank_id == self.delim_id:
            raise L.SpeechLLMError(f"CTC segmenter: blank_id and delim_id are both {self.blank_id}")
        if "lm_head.weight" not in state_dict:
            raise L.SpeechLLMError("CTC segmenter: the checkpoint has no lm_head.weight (a HubertForCTC checkpoint is needed, not a bare HubertModel)")
        head_w = state_dict["lm_head.weight"].detach().float()
        head_b = state_dict["lm_head.bias"].detach().float() if "lm_head.bias" in state_dict else None
        if head_w.dim() != 2 or head_w.shape[1] != arch.hidden_size or not 1 <= head_w.shape[0] <= 64:
            raise L.SpeechLLMError(f"CTC segmenter: lm_head.weight {tuple(head_w.shape)} must be (V <= 64, {arch.hidden_size})")
        self.vocab_size = int(head_w.shape[0])
        enc_sd = {"encoder." + k[len("hubert."):]: v.detach().float() for k, v in state_dict.items() if k.startswith("hubert.")}
        if "encoder.feature_projection.projection.weight" not in enc_sd:
            raise L.SpeechLLMError("CTC segmenter: no `hubert.*` encoder weights in the checkpoint")
        enc_sd["embed_projection.weight"] = torch.zeros(_DUMMY_PROJ, arch.hidden_size)      # never read: the frames-only path stops at last_hidden
        enc_sd["embed_projection.bias"] = torch.zeros(_DUMMY_PROJ)
        conf = cfgm.from_dict(dict(model=dict(audio_encoder=dict(base="hubert", type=self.path or "ctc-segmenter", downsample_method="ctc_pool",
                                                                 downsample_factor=1), llm_embedding_channels=_DUMMY_PROJ)))
        self.encoder = AudioEncoder(conf, self.device, dtype=dtype, arch=arch, load_pretrained=False)
        self.encoder.load_state_dict(enc_sd).eval()
        self.head_w = head_w.to(device=self.device, dtype=dtype).contiguous()
        self.head_b = head_b.to(device=self.device, dtype=dtype).contiguous() if head_b is not None else None

    # -- packed forms (device tensors) ---------------------------------------------------------------
    def _waves(self, audios) -> List[torch.Tensor]:
        if torch.is_tensor(audios) and audios.dim() == 1:
            audios = [audios]
        return [torch.as_tensor(a, dtype=torch.float32).reshape(-1) for a in audios]

    def ids_packed(self, audios) -> Tuple[torch.Tensor, List[int]]:
        """One ragged batch -> (int32 ids of all frames packed, frames per utterance)."""
        waves = self._waves(audios)
        _, _, hidden, T = self.encoder.encode_packed(waves, want_last_hidden=True, _frames_only=True)
        return ops.ctc_greedy(hidden, self.head_w, self.head_b), list(T)

    def _row_offsets(self, T: Sequence[int]) -> torch.Tensor:
        offs = [0]
        for t in T:
            offs.append(offs[-1] + int(t))
        return L.h2d(offs, torch.int64, self.device)

    def ranges_packed(self, audios, pool_range: int = 4) -> Tuple[torch.Tensor, List[int]]:
        """-> (int64 device table (sum counts, 2) of {first row, end row} in packed frame rows, counts per utterance): what
        AudioEncoder.encode_packed(ctc_pool_ranges_dev=...) takes for the same utterances in the same order.  The counts are the one
        device-to-host copy of the batch."""
        ids, T = self.ids_packed(audios)
        ranges, counts = ops.ctc_pool_ranges(ids, self._row_offsets(T), self.blank_id, self.delim_id, pool_range)
        counts = [int(c) for c in counts.cpu().tolist()]
        return ranges[:sum(counts)], counts

    # -- list forms ----------------------------------------------------------------------------------
    def greedy_ids(self, audios) -> List[torch.Tensor]:
        """One int32 device tensor of greedy CTC ids per utterance (views of one packed tensor)."""
        ids, T = self.ids_packed(audios)
        return list(torch.split(ids, T))

    @staticmethod
    def _split_pairs(table: torch.Tensor, counts: torch.Tensor) -> List[List[Tuple[int, int]]]:
        counts = [int(c) for c in counts.cpu().tolist()]
        rows = table[:sum(counts)].cpu().tolist()
        out, at = [], 0
        for c in counts:
            out.append([(int(a), int(b)) for a, b in rows[at:at + c]])
            at += c
        return out

    def word_offsets(self, audios) -> List[List[Tuple[int, int]]]:
        """HF's word offsets, one list of (start_offset, end_offset) frame pairs per utterance."""
        ids, T = self.ids_packed(audios)
        _, _, words, wcounts = ops.ctc_pool_ranges(ids, self._row_offsets(T), self.blank_id, self.delim_id, 4, want_words=True)
        return self._split_pairs(words, wcounts)

    def pool_ranges(self, audios, pool_range: int = 4, raw: bool = False) -> List[List[Tuple[int, int]]]:
        """Lists shaped like the dataset's `pool_ranges_4` column: utterance-relative (start, end) pairs.  raw=True: the reference's list exactly
        (unclamped, empty pairs kept); raw=False: clamped to the utterance, empty pairs dropped: what `ctc_pool_ranges=` accepts."""
        ids, T = self.ids_packed(audios)
        ranges, counts = ops.ctc_pool_ranges(ids, self._row_offsets(T), self.blank_id, self.delim_id, pool_range, raw=raw)
        per = self._split_pairs(ranges, counts)
        if raw:
            return per
        out, tok0 = [], 0
        for lst, t in zip(per, T):
            out.append([(a - tok0, b - tok0) for a, b in lst])
            tok0 += int(t)
        return out
