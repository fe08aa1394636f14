"""YAML config loader: accepts the reference's config schema verbatim (ref:config/llama3_hubert.yaml:1-47;
the reference loads it with OmegaConf, ref:inference.py:158) and exposes it with attribute access."""
from __future__ import annotations

import re

import yaml

# PyYAML (YAML 1.1) reads `5e-5` as a string; OmegaConf, which the reference uses, reads it as a float
# (ref:config/llama3_hubert.yaml:30 `lr: 5e-5`).  Resolve such scalars the OmegaConf way.
_FLOAT_RE = re.compile(r"^[+-]?(\d+\.?\d*|\.\d+)[eE][+-]?\d+$")


class AttrDict(dict):
    """dict with attribute access, nested, like the OmegaConf nodes the reference passes around."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _wrap(o):
    if isinstance(o, dict):
        return AttrDict({k: _wrap(v) for k, v in o.items()})
    if isinstance(o, list):
        return [_wrap(v) for v in o]
    if isinstance(o, str) and _FLOAT_RE.match(o):
        return float(o)
    return o


def load_config(path: str) -> AttrDict:
    with open(path) as f:
        return _wrap(yaml.safe_load(f))


def from_dict(d: dict) -> AttrDict:
    return _wrap(d)


_RUNTIME_DTYPES = {"fp32": "float32", "bf16": "bfloat16", "fp16": "float16"}


def runtime_kv_dtype(config):
    """The K/V cache format a config's `runtime.kv_dtype` names: `model` (default: rows in the model dtype) -> None, `fp8` -> "fp8"
    (OCP e4m3 rows, 16-bit models only) — the value the `kv_cache_dtype` keyword of the model classes takes."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    name = str((rt or {}).get("kv_dtype", "model"))
    if name not in ("model", "fp8"):
        raise ValueError(f"runtime.kv_dtype: {name!r} is not one of ['fp8', 'model']")
    return "fp8" if name == "fp8" else None


def runtime_weight_dtype(config):
    """The decode-weight format a config's `runtime.weight_dtype` names: `model` (default: the model dtype) -> None, `fp8` -> "fp8"
    (e4m3 weight images for decode steps of small batches, 16-bit models only), `mxfp4` / `fp4` -> "mxfp4" (MXFP4 weight images, the
    same range) — the value the `weight_dtype` keyword of the model classes takes."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    name = str((rt or {}).get("weight_dtype", "model"))
    if name not in ("model", "fp8", "mxfp4", "fp4"):
        raise ValueError(f"runtime.weight_dtype: {name!r} is not one of ['fp4', 'fp8', 'model', 'mxfp4']")
    if name in ("mxfp4", "fp4"):      # MXFP4 weight images (e2m1 elements, one e8m0 scale per 32); `fp4` is an alias
        return "mxfp4"
    return "fp8" if name == "fp8" else None


def runtime_linear_dtype(config):
    """The layer-product format a config's `runtime.linear_dtype` names: `model` (default: the model dtype) -> None, `mx` /
    `mxfp8_mxfp4` -> "mx" (MXFP8 activations x MXFP4 weights in every decoder-layer product, 16-bit models only) — the value the
    `linear_dtype` keyword of the model classes takes."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    name = str((rt or {}).get("linear_dtype", "model"))
    if name not in ("model", "mx", "mxfp8_mxfp4"):
        raise ValueError(f"runtime.linear_dtype: {name!r} is not one of ['model', 'mx', 'mxfp8_mxfp4']")
    return None if name == "model" else "mx"


def runtime_dtype(config) -> "torch.dtype":
    """The compute dtype a config's `runtime.dtype` names (default bf16): fp32 (exact-fp32 parity mode), bf16, or fp16
    (inference only, the reference's torch_dtype=float16 regime; training rejects it)."""
    import torch

    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    name = str((rt or {}).get("dtype", "bf16"))
    if name not in _RUNTIME_DTYPES:
        raise ValueError(f"runtime.dtype: {name!r} is not one of {sorted(_RUNTIME_DTYPES)}")
    return getattr(torch, _RUNTIME_DTYPES[name])


def runtime_logits(config):
    """The logits processors a config's `runtime` section names: optional `repetition_penalty` (default 1.0 = off),
    `no_repeat_ngram_size` (0 = off) and `min_new_tokens` (0 = off) -> None when all are off, else the dict the `logits` keyword of
    generate_packed takes."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    rt = rt or {}
    p = rt.get("repetition_penalty", 1.0)
    if isinstance(p, bool) or not isinstance(p, (int, float)) or p != p or p == float("inf") or p <= 0:
        raise ValueError(f"runtime.repetition_penalty: {p!r} is not a finite number > 0")
    out = dict(repetition_penalty=float(p))
    for key in ("no_repeat_ngram_size", "min_new_tokens"):
        v = rt.get(key, 0)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"runtime.{key}: {v!r} is not an integer >= 0")
        out[key] = int(v)
    if out["repetition_penalty"] == 1.0 and out["no_repeat_ngram_size"] == 0 and out["min_new_tokens"] == 0:
        return None
    return out


def runtime_warpers(config):
    """The sampling warpers a config's `runtime` section names: optional `min_p`, `typical_p`, `epsilon_cutoff`, `eta_cutoff` -> the dict of
    those present (empty in the shipped yamls), each a number in its range (min_p [0, 1], typical_p (0, 1], the cutoffs [0, 1)); they set
    the llm's generation_config and act where a call samples."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    rt = rt or {}
    ranges = dict(min_p=lambda v: 0.0 <= v <= 1.0, typical_p=lambda v: 0.0 < v <= 1.0, epsilon_cutoff=lambda v: 0.0 <= v < 1.0,
                  eta_cutoff=lambda v: 0.0 <= v < 1.0)
    out = {}
    for key, ok in ranges.items():
        v = rt.get(key)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(v):
            raise ValueError(f"runtime.{key}: {v!r} is outside its range")
        out[key] = float(v)
    return out


def runtime_beams(config):
    """The beam-search options a config's `runtime` section names: optional `num_beams` (default 1 = greedy), `length_penalty` (1.0) and
    `early_stopping` (false / true / "never") -> None for greedy, else the dict the `beams` keyword of generate_packed takes."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    rt = rt or {}
    k = rt.get("num_beams", 1)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 8:
        raise ValueError(f"runtime.num_beams: {k!r} is not an integer in [1, 8]")
    lp = rt.get("length_penalty", 1.0)
    if isinstance(lp, bool) or not isinstance(lp, (int, float)) or lp != lp or lp in (float("inf"), float("-inf")):
        raise ValueError(f"runtime.length_penalty: {lp!r} is not a finite number")
    es = rt.get("early_stopping", False)
    if not (isinstance(es, bool) or es == "never"):
        raise ValueError(f"runtime.early_stopping: {es!r} is not one of [False, True, 'never']")
    if k == 1:
        return None
    return dict(num_beams=int(k), length_penalty=float(lp), early_stopping=es, num_return_sequences=1)


def runtime_num_return(config) -> int:
    """`runtime.num_return_sequences` of a config (default 1): sampled answers per utterance; above 1 the answers are drawn with the
    llm's generation_config temperature / top_k / top_p (greedy search has one answer per prompt)."""
    rt = config.get("runtime", {}) if hasattr(config, "get") else {}
    r = (rt or {}).get("num_return_sequences", 1)
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        raise ValueError(f"runtime.num_return_sequences: {r!r} is not an integer >= 1")
    return int(r)
