"""Thin tensor-level wrappers over the per-op C-ABI entry points (used by the kernel parity tests and by
host code that composes ops outside the whole-model entry points).  Every function launches HIP kernels
on the current torch stream; nothing here computes on the CPU.
"""
from __future__ import annotations

import os
import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib as L


def gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         act: int = L.ACT_NONE, out_f32: bool = False, *, M: Optional[int] = None, K: Optional[int] = None,
         lda: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = act(A W^T + bias) + residual.  `M/K/lda` override the view for implicit-GEMM convolutions."""
    L.require_gpu(A, "A"); L.require_gpu(W, "W")
    N = W.shape[0]
    K = W.shape[1] if K is None else K
    M = A.shape[0] if M is None else M
    lda = A.stride(0) if lda is None else lda
    n_out = N // 2 if act == L.ACT_SILU_MUL else N
    if out is None:
        out = torch.empty((M, n_out), device=A.device, dtype=torch.float32 if out_f32 else A.dtype)
    a = L.GemmArgs()
    a.A, a.lda, a.strideA = L.ptr(A), lda, 0
    a.W, a.ldw, a.strideW = L.ptr(W), W.stride(0), 0
    a.C, a.ldc, a.strideC = L.ptr(out), out.stride(0), 0
    a.bias, a.strideBias = L.ptr(bias), 0
    a.residual, a.ldr, a.strideR = L.ptr(residual), (residual.stride(0) if residual is not None else 0), 0
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.dtype, a.act, a.out_f32 = L.dtype_code(A.dtype), act, int(out_f32)
    L.check(L.lib().sl_gemm(C.byref(a), L.stream_ptr()), "sl_gemm")
    return out


def gemm_batched(args: "L.GemmArgs") -> None:
    L.check(L.lib().sl_gemm(C.byref(args), L.stream_ptr()), "sl_gemm")


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float, gelu: bool = False) -> torch.Tensor:
    L.require_gpu(x, "x")
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    L.check(L.lib().sl_layernorm(L.ptr(x), L.ptr(y), L.ptr(g), L.ptr(b), rows, x.shape[-1], eps, int(gelu),
                                 L.dtype_code(x.dtype), L.stream_ptr()), "sl_layernorm")
    return y


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    L.require_gpu(x, "x")
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    L.check(L.lib().sl_rmsnorm(L.ptr(x), L.ptr(y), L.ptr(w), rows, x.shape[-1], eps, L.dtype_code(x.dtype), L.stream_ptr()),
            "sl_rmsnorm")
    return y


def hubert_conv0(wave: torch.Tensor, w: torch.Tensor, bias, gamma, beta, dtype: torch.dtype, k: int = 10, stride: int = 5,
                 eps: float = 1e-5) -> torch.Tensor:
    L.require_gpu(wave, "wave")
    n = wave.numel()
    Cout = w.shape[0]
    Lout = (n - k) // stride + 1
    out = torch.empty((Lout, Cout), device=wave.device, dtype=dtype)
    L.check(L.lib().sl_hubert_conv0(L.ptr(wave), n, L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(out), Cout, k, stride,
                                    eps, L.dtype_code(dtype), L.stream_ptr()), "sl_hubert_conv0")
    return out


def posconv_stage(x: torch.Tensor, groups: int, k: int) -> torch.Tensor:
    T, H = x.shape
    xg = torch.empty((groups, T + k, H // groups), device=x.device, dtype=x.dtype)
    L.check(L.lib().sl_posconv_stage(L.ptr(x), L.ptr(xg), T, H, groups, k, L.dtype_code(x.dtype), L.stream_ptr()), "sl_posconv_stage")
    return xg


def avgpool_rows(x: torch.Tensor, kernel: int = 8, stride: int = 4, ranges: Optional[torch.Tensor] = None) -> torch.Tensor:
    T, H = x.shape
    P = ranges.shape[0] if ranges is not None else (T - kernel) // stride + 1
    y = torch.empty((P, H), device=x.device, dtype=x.dtype)
    L.check(L.lib().sl_avgpool_rows(L.ptr(x), L.ptr(y), T, H, kernel, stride, L.ptr(ranges), P, L.dtype_code(x.dtype), L.stream_ptr()),
            "sl_avgpool_rows")
    return y


def hubert_conv0_batch(flat_waves: torch.Tensor, sample_offsets: Sequence[int], row_offsets: Sequence[int], w, bias, gamma, beta, dtype: torch.dtype,
                       k: int = 10, stride: int = 5, eps: float = 1e-5) -> torch.Tensor:
    """conv0 + LayerNorm + GELU of every utterance of a ragged batch in one launch -> packed (sum L_u, C) rows."""
    dev = flat_waves.device
    n_utt = len(sample_offsets) - 1
    desc = L.h2d([list(sample_offsets), list(row_offsets)], torch.int64, dev)
    out = torch.empty((row_offsets[-1], w.shape[0]), device=dev, dtype=dtype)
    max_L = max(row_offsets[u + 1] - row_offsets[u] for u in range(n_utt))
    L.check(L.lib().sl_hubert_conv0_batch(L.ptr(flat_waves), desc[0].data_ptr(), desc[1].data_ptr(), n_utt, max_L, L.ptr(w), L.ptr(bias), L.ptr(gamma),
                                          L.ptr(beta), L.ptr(out), w.shape[0], k, stride, eps, L.dtype_code(dtype), L.stream_ptr()), "sl_hubert_conv0_batch")
    return out


def posconv_stage_batch(x: torch.Tensor, seqlens: Sequence[int], groups: int, k: int) -> torch.Tensor:
    """sl_posconv_stage for every utterance of a packed batch in one launch; utterance u's (groups, T_u + k, H/groups) block
    starts (cu[u] + u k) * H elements into the flat result."""
    cu, klen = seq_descriptors(seqlens, x.device)
    H = x.shape[1]
    xg = torch.empty((x.shape[0] + len(seqlens) * k) * H, device=x.device, dtype=x.dtype)
    L.check(L.lib().sl_posconv_stage_batch(L.ptr(x), L.ptr(xg), cu.data_ptr(), klen.data_ptr(), len(seqlens), max(int(n) for n in seqlens), H, groups, k,
                                           L.dtype_code(x.dtype), L.stream_ptr()), "sl_posconv_stage_batch")
    return xg


def avgpool_batch(x: torch.Tensor, seqlens: Sequence[int], kernel: int, stride: int):
    """AvgPool1d over time of every utterance of a packed batch in one launch -> (packed pooled rows, P list)."""
    for u, t in enumerate(seqlens):          # as hubert_plan does in C: no zero or negative row count reaches the records
        if int(t) < kernel:
            raise L.SpeechLLMError(f"avgpool_batch: utterance {u} gives {int(t)} frames < pool kernel {kernel}")
    cu, klen = seq_descriptors(seqlens, x.device)
    H = x.shape[1]
    P = [(int(t) - kernel) // stride + 1 for t in seqlens]
    rec, row = [], 0
    for p_ in P:
        rec.append([p_, row * H, 0, 0])
        row += p_
    rec_t = L.h2d(rec, torch.int64, x.device)
    y = torch.empty((row, H), device=x.device, dtype=x.dtype)
    L.check(L.lib().sl_avgpool_batch(L.ptr(x), L.ptr(y), cu.data_ptr(), klen.data_ptr(), rec_t.data_ptr(), len(seqlens), max(P), H, kernel, stride,
                                     L.dtype_code(x.dtype), L.stream_ptr()), "sl_avgpool_batch")
    return y, P


def embed_gather(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    ids32 = ids.to(device=table.device, dtype=torch.int32).contiguous().view(-1)
    out = torch.empty((ids32.numel(), table.shape[1]), device=table.device, dtype=table.dtype)
    L.check(L.lib().sl_embed_gather(L.ptr(table), L.ptr(ids32), L.ptr(out), ids32.numel(), table.shape[1], L.dtype_code(table.dtype),
                                    L.stream_ptr()), "sl_embed_gather")
    return out


def attn_fwd(q, k, v, out, cu_q, cu_k, klen, *, q_strides, k_strides, v_strides, o_strides, nseq, max_qlen, n_heads, n_kv_heads,
             head_dim, causal, scale, dropout_p: float = 0.0, dropout_seed: int = 0, lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sl_attn_fwd on separate q / k / v / out views (strides in elements: (row, head)).  dropout_p > 0 and lse: the training-mode
    outputs of attn_packed_qkv (lse: fp32 (query rows, n_heads), indexed by the global query row)."""
    a = L.AttnArgs()
    a.q, a.q_row_stride, a.q_head_stride = L.ptr(q), q_strides[0], q_strides[1]
    a.k, a.k_row_stride, a.k_head_stride = L.ptr(k), k_strides[0], k_strides[1]
    a.v, a.v_row_stride, a.v_head_stride = L.ptr(v), v_strides[0], v_strides[1]
    a.out, a.o_row_stride, a.o_head_stride = L.ptr(out), o_strides[0], o_strides[1]
    a.cu_q, a.cu_k, a.klen = L.ptr(cu_q), L.ptr(cu_k), L.ptr(klen)
    a.nseq, a.max_qlen, a.n_heads, a.n_kv_heads = nseq, max_qlen, n_heads, n_kv_heads
    a.head_dim, a.causal, a.dtype, a.scale = head_dim, int(causal), L.dtype_code(out.dtype), scale
    a.dropout_p, a.dropout_seed = float(dropout_p), int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
    a.lse = L.ptr(lse)
    L.check(L.lib().sl_attn_fwd(C.byref(a), L.stream_ptr()), "sl_attn_fwd")
    return out


def attn_fwd_past(q, k, v, out, cu_q, cu_k, klen, k_past, v_past, past_len, past_row0, *, q_strides, k_strides, v_strides, o_strides, nseq, max_qlen,
                  n_heads, n_kv_heads, head_dim, max_ctx, kv_format, scale, causal=True, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """sl_attn_fwd_past: causal prefill attention of continued sequences — keys [0, past_len[s]) from one layer's cache (k_past / v_past
    (slots, n_kv, max_ctx, D), elements of the dtype or e4m3 bytes; past_row0[s] = slot * n_kv * max_ctx), then the klen[s] new rows of k / v."""
    a = L.AttnArgs()
    a.q, a.q_row_stride, a.q_head_stride = L.ptr(q), q_strides[0], q_strides[1]
    a.k, a.k_row_stride, a.k_head_stride = L.ptr(k), k_strides[0], k_strides[1]
    a.v, a.v_row_stride, a.v_head_stride = L.ptr(v), v_strides[0], v_strides[1]
    a.out, a.o_row_stride, a.o_head_stride = L.ptr(out), o_strides[0], o_strides[1]
    a.cu_q, a.cu_k, a.klen = L.ptr(cu_q), L.ptr(cu_k), L.ptr(klen)
    a.nseq, a.max_qlen, a.n_heads, a.n_kv_heads = nseq, max_qlen, n_heads, n_kv_heads
    a.head_dim, a.causal, a.dtype, a.scale = head_dim, int(causal), L.dtype_code(out.dtype if dtype is None else dtype), scale
    L.check(L.lib().sl_attn_fwd_past(C.byref(a), L.ptr(k_past), L.ptr(v_past), L.ptr(past_len), L.ptr(past_row0), int(max_ctx), int(kv_format),
                                     L.stream_ptr()), "sl_attn_fwd_past")
    return out


def attn_bwd(q, k, v, out, d_out, lse, dq, dk, dv, cu_q, cu_k, klen, *, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
             dk_strides, dv_strides, nseq, max_qlen, max_klen, n_tok_q, n_heads, n_kv_heads, head_dim, causal, scale, dropout_p: float = 0.0,
             dropout_seed: int = 0, delta: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sl_attn_bwd on separate views (strides in elements: (row, head)): dq / dk / dv <- the gradients of q / k / v given out, d_out and the
    forward's lse (fp32 (n_tok_q, n_heads)).  delta: fp32 (n_tok_q, n_heads) scratch for rowsum(d_out * out), allocated if None; returned."""
    if delta is None:
        delta = torch.empty((n_tok_q, n_heads), device=q.device, dtype=torch.float32)
    a = L.AttnBwdArgs()
    a.q, a.q_row_stride, a.q_head_stride = L.ptr(q), q_strides[0], q_strides[1]
    a.k, a.k_row_stride, a.k_head_stride = L.ptr(k), k_strides[0], k_strides[1]
    a.v, a.v_row_stride, a.v_head_stride = L.ptr(v), v_strides[0], v_strides[1]
    a.out, a.o_row_stride, a.o_head_stride = L.ptr(out), o_strides[0], o_strides[1]
    a.d_out, a.do_row_stride, a.do_head_stride = L.ptr(d_out), do_strides[0], do_strides[1]
    a.dq, a.dq_row_stride, a.dq_head_stride = L.ptr(dq), dq_strides[0], dq_strides[1]
    a.dk, a.dk_row_stride, a.dk_head_stride = L.ptr(dk), dk_strides[0], dk_strides[1]
    a.dv, a.dv_row_stride, a.dv_head_stride = L.ptr(dv), dv_strides[0], dv_strides[1]
    a.lse, a.delta = L.ptr(lse), L.ptr(delta)
    a.cu_q, a.cu_k, a.klen = L.ptr(cu_q), L.ptr(cu_k), L.ptr(klen)
    a.n_tok_q, a.nseq, a.max_qlen, a.max_klen = n_tok_q, nseq, max_qlen, max_klen
    a.n_heads, a.n_kv_heads, a.head_dim, a.causal, a.dtype = n_heads, n_kv_heads, head_dim, int(causal), L.dtype_code(q.dtype)
    a.scale, a.dropout_p, a.dropout_seed = scale, float(dropout_p), int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
    L.check(L.lib().sl_attn_bwd(C.byref(a), L.stream_ptr()), "sl_attn_bwd")
    return delta


_SEQ_DESC = {}


def seq_descriptors(seqlens: Sequence[int], device):
    """(cu_seqlens int32 (n+1), lens int32 (n)) device tensors of a packed batch, cached per length tuple (the KD step calls
    attention forward + backward for every layer with the same lengths)."""
    key = (tuple(int(n) for n in seqlens), str(device))
    d = _SEQ_DESC.get(key)
    if d is None:
        if len(_SEQ_DESC) > 64:
            _SEQ_DESC.clear()
        cu = [0]
        for n in key[0]:
            cu.append(cu[-1] + n)
        d = (L.h2d(cu, torch.int32, device), L.h2d(list(key[0]), torch.int32, device))
        _SEQ_DESC[key] = d
    return d


def attn_packed_qkv(qkv: torch.Tensor, seqlens: Sequence[int], n_heads: int, n_kv_heads: int, head_dim: int, causal: bool,
                    scale: float, dropout_p: float = 0.0, dropout_seed: int = 0, lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention over a packed fused (tokens, (nh+2nkv)*D) activation (the HuBERT layout).  dropout_p > 0: training-mode
    dropout of the attention probabilities (mask index ((token * nh + head) << 16) | key, see sl_attn_args).
    lse: optional fp32 (tokens, n_heads) buffer that receives the log-sum-exp (what attn_packed_qkv_bwd needs)."""
    dev = qkv.device
    cu, klen = seq_descriptors(seqlens, dev)
    ntok = qkv.shape[0]
    rs = qkv.stride(0)
    out = torch.empty((ntok, n_heads * head_dim), device=dev, dtype=qkv.dtype)
    qv = qkv
    kv = qkv[:, n_heads * head_dim:]
    vv = qkv[:, (n_heads + n_kv_heads) * head_dim:]
    a = L.AttnArgs()
    a.q, a.q_row_stride, a.q_head_stride = qv.data_ptr(), rs, head_dim
    a.k, a.k_row_stride, a.k_head_stride = kv.data_ptr(), rs, head_dim
    a.v, a.v_row_stride, a.v_head_stride = vv.data_ptr(), rs, head_dim
    a.out, a.o_row_stride, a.o_head_stride = out.data_ptr(), n_heads * head_dim, head_dim
    a.cu_q, a.cu_k, a.klen = cu.data_ptr(), cu.data_ptr(), klen.data_ptr()
    a.nseq, a.max_qlen, a.n_heads, a.n_kv_heads = len(seqlens), max(seqlens), n_heads, n_kv_heads
    a.head_dim, a.causal, a.dtype, a.scale = head_dim, int(causal), L.dtype_code(qkv.dtype), scale
    a.dropout_p, a.dropout_seed = float(dropout_p), int(dropout_seed) & 0xFFFFFFFFFFFFFFFF
    a.lse = L.ptr(lse)
    L.check(L.lib().sl_attn_fwd(C.byref(a), L.stream_ptr()), "sl_attn_fwd")
    return out


def attn_packed_qkv_bwd(qkv: torch.Tensor, out: torch.Tensor, d_out: torch.Tensor, lse: torch.Tensor, d_qkv: torch.Tensor, seqlens: Sequence[int],
                        n_heads: int, n_kv_heads: int, head_dim: int, causal: bool, scale: float, dropout_p: float = 0.0,
                        dropout_seed: int = 0) -> torch.Tensor:
    """Flash-style backward of attn_packed_qkv (sl_attn_bwd): d_qkv (same fused layout as qkv) <- [dQ | dK | dV]."""
    cu, klen = seq_descriptors(seqlens, qkv.device)
    rs, drs, D = qkv.stride(0), d_qkv.stride(0), head_dim
    koff, voff = n_heads * D, (n_heads + n_kv_heads) * D
    smax = max(int(n) for n in seqlens)
    attn_bwd(qkv, qkv[:, koff:], qkv[:, voff:], out, d_out, lse, d_qkv, d_qkv[:, koff:], d_qkv[:, voff:], cu, cu, klen, q_strides=(rs, D),
             k_strides=(rs, D), v_strides=(rs, D), o_strides=(out.stride(0), D), do_strides=(d_out.stride(0), D), dq_strides=(drs, D),
             dk_strides=(drs, D), dv_strides=(drs, D), nseq=len(seqlens), max_qlen=smax, max_klen=smax, n_tok_q=qkv.shape[0], n_heads=n_heads,
             n_kv_heads=n_kv_heads, head_dim=D, causal=causal, scale=scale, dropout_p=dropout_p, dropout_seed=dropout_seed)
    return d_qkv


def attn_dropout_bwd(P: torch.Tensor, Pd: torch.Tensor, dP: torch.Tensor, n_mat: int, smax: int, dims: torch.Tensor, ld: int, cu_q: torch.Tensor,
                     n_heads: int, n_kv_heads: int, r: int, p: float, seed: int) -> None:
    L.check(L.lib().sl_attn_dropout_bwd(L.ptr(P), L.ptr(Pd), L.ptr(dP), n_mat, smax, L.ptr(dims), ld, L.ptr(cu_q), n_heads, n_kv_heads, r, float(p),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, L.dtype_code(P.dtype), L.stream_ptr()), "sl_attn_dropout_bwd")


def rope_kv_append(qkv, k_cache, v_cache, tok_seq, tok_pos, cos, sin, n_heads, n_kv, D, max_ctx) -> None:
    L.check(L.lib().sl_rope_kv_append(L.ptr(qkv), L.ptr(k_cache), L.ptr(v_cache), L.ptr(tok_seq), L.ptr(tok_pos), L.ptr(cos), L.ptr(sin),
                                      qkv.shape[0], n_heads, n_kv, D, max_ctx, L.dtype_code(qkv.dtype), L.stream_ptr()),
            "sl_rope_kv_append")


def rope_kv_append_ex(qkv, k_cache, v_cache, tok_seq, tok_pos, cos, sin, n_heads, n_kv, D, max_ctx, kv_format: int = L.KV_MODEL_DTYPE) -> None:
    """sl_rope_kv_append with the cache format given: KV_FP8_E4M3 writes e4m3 bytes (uint8 caches) and the rotated K rows back into qkv."""
    L.check(L.lib().sl_rope_kv_append_ex(L.ptr(qkv), L.ptr(k_cache), L.ptr(v_cache), L.ptr(tok_seq), L.ptr(tok_pos), L.ptr(cos), L.ptr(sin),
                                         qkv.shape[0], n_heads, n_kv, D, max_ctx, L.dtype_code(qkv.dtype), int(kv_format), L.stream_ptr()),
            "sl_rope_kv_append_ex")


def attn_decode(q, q_stride, k_cache, v_cache, ctx_len, n_heads, n_kv, D, max_ctx, scale) -> torch.Tensor:
    B = ctx_len.shape[0]
    out = torch.empty((B, n_heads * D), device=q.device, dtype=q.dtype)
    L.check(L.lib().sl_attn_decode(L.ptr(q), q_stride, L.ptr(k_cache), L.ptr(v_cache), L.ptr(out), L.ptr(ctx_len), B, n_heads, n_kv, D,
                                   max_ctx, scale, L.dtype_code(q.dtype), L.stream_ptr()), "sl_attn_decode")
    return out


def _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids):
    """what every select entry takes besides its own arguments: (the EOS ids as a C array, the row-state arguments in the entries' order)"""
    eos = (C.c_int32 * max(1, len(eos_ids)))(*eos_ids)
    return eos, (L.ptr(unfinished), L.ptr(ctx_len), L.ptr(gen_count), L.ptr(finish_len), L.ptr(next_ids), L.ptr(out_ids), out_ids.shape[1])


def greedy_select(logits, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids) -> None:
    B, V = logits.shape
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_greedy_select(L.ptr(logits), B, V, eos, len(eos_ids), pad_id, int(use_eos), *state, L.stream_ptr()), "sl_greedy_select")


def gemm_top1(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """Row-wise top-1 of A W^T (+ bias) without storing the product (sl_gemm_ex_args.amax_*): returns (val, idx), each
    (ceil(N / 64), M): the largest value of every 64-column group and its column."""
    L.require_gpu(A, "A"); L.require_gpu(W, "W")
    M, K = A.shape
    N = W.shape[0]
    ng = (N + 63) // 64
    val = torch.empty((ng, M), device=A.device, dtype=torch.float32)
    idx = torch.empty((ng, M), device=A.device, dtype=torch.int32)
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = L.ptr(A), A.stride(0), L.ptr(W), W.stride(0), None, N
    a.bias = L.ptr(bias)
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.dtype, a.act, a.out_f32 = L.dtype_code(A.dtype), L.ACT_NONE, 1
    ex = L.GemmEx()
    ex.w_mod, ex.amax_val, ex.amax_idx = 1, L.ptr(val), L.ptr(idx)
    L.check(L.lib().sl_gemm_ex(C.byref(a), C.byref(ex), L.stream_ptr()), "sl_gemm_ex")
    return val, idx


def greedy_select_partial(val, idx, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, advance_ctx=True) -> None:
    ng, B = val.shape
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_greedy_select_partial(L.ptr(val), L.ptr(idx), ng, B, eos, len(eos_ids), pad_id, int(use_eos), int(advance_ctx), *state,
                                             L.stream_ptr()), "sl_greedy_select_partial")


def pack_weight(W: torch.Tensor) -> torch.Tensor:
    """(N,K) row-major -> fragment-packed buffer for the decode kernel (sl_pack_weight)."""
    L.require_gpu(W, "W")
    n, k = W.shape
    out = torch.empty(((n + 15) // 16 * 16, k), device=W.device, dtype=W.dtype)
    L.check(L.lib().sl_pack_weight(L.ptr(W), W.stride(0), L.ptr(out), n, k, L.dtype_code(W.dtype), L.stream_ptr()), "sl_pack_weight")
    return out


# ---- weight images (speechllm.h "e4m3 weight image", "MXFP4 weight image", "MX weight image"): bytes, packer, parts, dequantiser ----
def _image_bytes(fn_name: str, N: int, K: int) -> int:
    n = int(getattr(L.lib(), fn_name)(N, K))
    if n == 0:
        L.check(-1, fn_name)
    return n


def _pack_image(name: str, W: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N, K) bf16 / fp16 weight (row stride W.stride(0)) -> its `name` weight image, a uint8 buffer of the image's bytes.  On the GPU
    through the device packer sl_pack_weight_<name>, on the CPU through the host entry: the same routines, the same bytes."""
    n, k = W.shape
    if W.stride(1) != 1:
        raise L.SpeechLLMError(f"pack_weight_{name}: rows must be contiguous")
    bytes_fn = {"e4m3": "sl_w8_image_bytes", "mxfp4": "sl_w4_image_bytes", "mx": "sl_mx_weight_image_bytes"}[name]
    if out is None:
        out = torch.empty(_image_bytes(bytes_fn, n, k), device=W.device, dtype=torch.uint8)
    if out.numel() != _image_bytes(bytes_fn, n, k) or not out.is_contiguous() or out.dtype != torch.uint8:
        raise L.SpeechLLMError(f"pack_weight_{name}: out must be a contiguous uint8 buffer of {bytes_fn[3:]}(N, K)")
    if W.is_cuda:
        L.check(getattr(L.lib(), f"sl_pack_weight_{name}")(L.ptr(W), W.stride(0), L.ptr(out), n, k, L.dtype_code(W.dtype), L.stream_ptr()), f"sl_pack_weight_{name}")
    else:
        L.check(getattr(L.lib(), f"sl_pack_weight_{name}_host")(L.ptr(W), W.stride(0), L.ptr(out), n, k, L.dtype_code(W.dtype)), f"sl_pack_weight_{name}_host")
    return out


_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _e2m1_block_dequantise(codes: torch.Tensor, scale_bytes: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """e2m1 codes (Np, K) and e8m0 scale bytes (Np, K/32) -> the (N, K) fp64 matrix e2m1 * 2^(scale byte - 127), every value exact."""
    grid = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float64)
    v = grid[codes.long()].view(codes.shape[0], K // 32, 32) * torch.exp2(scale_bytes.double() - 127)[:, :, None]
    return v.view(codes.shape[0], K)[:N]


def w8_image_bytes(N: int, K: int) -> int:
    return _image_bytes("sl_w8_image_bytes", N, K)


def pack_weight_e4m3(W: torch.Tensor) -> torch.Tensor:
    """_pack_image of the e4m3 weight image (sl_pack_weight_e4m3): the fragment-major bytes and, behind them, one fp32 scale per (padded) output row."""
    return _pack_image("e4m3", W)


def w8_image_parts(img: torch.Tensor, N: int, K: int):
    """An e4m3 weight image -> (bytes (Np, K) uint8 in natural row / column order, scales (Np,) fp32); Np = ceil(N/16)*16."""
    Np = (N + 15) // 16 * 16
    b = img[:Np * K].view(Np // 16, K // 64, 4, 16, 2, 8)                # [f][j][lane >> 4][lane & 15][half][e]
    b = b.permute(0, 3, 1, 4, 2, 5).reshape(Np, K)                      # row 16 f + (lane & 15), column 64 j + 32 half + 8 (lane >> 4) + e
    s = img[Np * K:Np * K + 4 * Np].clone().view(torch.float32)
    return b, s


def w8_dequantise(img: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """An e4m3 weight image -> the (N, K) fp64 matrix the kernels multiply by: byte value x s[n], formed in fp64."""
    b, s = w8_image_parts(img.cpu(), N, K)
    return (b.contiguous().view(torch.float8_e4m3fn).double() * s.double()[:, None])[:N]


def w4_image_bytes(N: int, K: int) -> int:
    return _image_bytes("sl_w4_image_bytes", N, K)


def pack_weight_mxfp4(W: torch.Tensor) -> torch.Tensor:
    """_pack_image of the MXFP4 weight image (sl_pack_weight_mxfp4): the fragment-major e2m1 nibbles and, behind them, one e8m0 scale byte per
    row and 32 columns."""
    return _pack_image("mxfp4", W)


def w4_image_parts(img: torch.Tensor, N: int, K: int):
    """An MXFP4 weight image -> (e2m1 codes (Np, K) uint8 in natural row / column order, scale bytes (Np, K/32) uint8); Np = ceil(N/16)*16."""
    Np = (N + 15) // 16 * 16
    b = img[:Np * K // 2].view(Np // 16, K // 128, 4, 16, 4, 4)          # [f][j][lane >> 4][lane & 15][dword][byte]
    c = torch.stack([b & 15, b >> 4], dim=-1)                           # element 2b in the low nibble, 2b + 1 in the high one
    c = c.permute(0, 3, 1, 4, 2, 5, 6).reshape(Np, K)                   # row 16 f + (lane & 15), column 128 j + 32 dword + 8 (lane >> 4) + 2 byte + half
    s = img[Np * K // 2:Np * K // 2 + Np * K // 32].view(Np // 16, K // 128, 16, 4)      # [f][j][r][d]
    return c, s.permute(0, 2, 1, 3).reshape(Np, K // 32)


def w4_dequantise(img: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """An MXFP4 weight image -> the (N, K) fp64 matrix the kernels multiply by (_e2m1_block_dequantise)."""
    return _e2m1_block_dequantise(*w4_image_parts(img.cpu(), N, K), N, K)


# ---- MX linears (speechllm.h "MX weight image", "MXFP8 activation rows", sl_gemm_mx) ---------------------------------------------
def mx_weight_image_bytes(N: int, K: int) -> int:
    return _image_bytes("sl_mx_weight_image_bytes", N, K)


def pack_weight_mx(W: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """_pack_image of the MX weight image (sl_pack_weight_mx): the MXFP4 image's codes and scale bytes, arranged one 32-element block per
    lane for the block-scaled MFMA."""
    return _pack_image("mx", W, out)


def mx_image_parts(img: torch.Tensor, N: int, K: int):
    """An MX weight image -> (e2m1 codes (Np, K) uint8 in natural row / column order, scale bytes (Np, K/32) uint8); Np = ceil(N/16)*16."""
    Np = (N + 15) // 16 * 16
    b = img[:Np * K // 2].view(Np // 16, K // 128, 4, 16, 16)           # [f][j][lane >> 4][lane & 15][byte]
    c = torch.stack([b & 15, b >> 4], dim=-1)                           # element 2b in the low nibble, 2b + 1 in the high one
    c = c.permute(0, 3, 1, 2, 4, 5).reshape(Np, K)                      # row 16 f + (lane & 15), column 128 j + 32 (lane >> 4) + 2 byte + half
    s = img[Np * K // 2:Np * K // 2 + Np * K // 32].view(Np // 16, K // 128, 4, 16)      # [f][j][lane >> 4][lane & 15]
    return c, s.permute(0, 3, 1, 2).reshape(Np, K // 32)


def mx_dequantise(img: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """An MX weight image -> the (N, K) fp64 matrix the product multiplies by (_e2m1_block_dequantise)."""
    return _e2m1_block_dequantise(*mx_image_parts(img.cpu(), N, K), N, K)


def mxfp8_quantize_rows(x: torch.Tensor, out=None):
    """(M, K) bf16 / fp16 rows (row stride x.stride(0)), K % 32 == 0 -> (q (M, K) uint8 e4m3 bytes, scales (M, K/32) uint8 e8m0 bytes).
    GPU tensor: sl_mxfp8_quantize_rows; CPU tensor: sl_mxfp8_quantize_rows_host, the definition."""
    m, k = x.shape
    if x.stride(1) != 1:
        raise L.SpeechLLMError("mxfp8_quantize_rows: rows must be contiguous")
    if out is not None:      # (q, scales): contiguous uint8 buffers of M * K and M * K/32 bytes
        q, s = out
        if q.numel() != m * k or s.numel() != m * (k // 32) or not q.is_contiguous() or not s.is_contiguous():
            raise L.SpeechLLMError("mxfp8_quantize_rows: out must be contiguous buffers of M * K and M * K/32 bytes")
    else:
        q = torch.empty((m, k), device=x.device, dtype=torch.uint8)
        s = torch.empty((m, max(k // 32, 0)), device=x.device, dtype=torch.uint8)
    if x.is_cuda:
        L.check(L.lib().sl_mxfp8_quantize_rows(L.ptr(x), x.stride(0), L.ptr(q), L.ptr(s), m, k, L.dtype_code(x.dtype), L.stream_ptr()), "sl_mxfp8_quantize_rows")
    else:
        L.check(L.lib().sl_mxfp8_quantize_rows_host(L.ptr(x), x.stride(0), L.ptr(q), L.ptr(s), m, k, L.dtype_code(x.dtype)), "sl_mxfp8_quantize_rows_host")
    return q, s


def mxfp8_dequantise(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """MXFP8 rows -> the (M, K) fp64 values the product multiplies by: e4m3 * 2^(scale byte - 127); a NaN byte (0x7F / 0xFF) stays NaN."""
    q, scales = q.cpu(), scales.cpu()
    v = q.contiguous().view(torch.float8_e4m3fn).double()
    m, k = q.shape
    return (v.view(m, k // 32, 32) * torch.exp2(scales.double() - 127)[:, :, None]).view(m, k)


def gemm_mx(Aq: torch.Tensor, a_scales: torch.Tensor, Wimg: torch.Tensor, N: int, *, dtype: torch.dtype = torch.bfloat16, act: int = L.ACT_NONE,
            residual: Optional[torch.Tensor] = None, out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(dq(Aq) . dq(Wimg)^T) + residual (sl_gemm_mx): Aq (M, K) e4m3 bytes (row stride Aq.stride(0)) with a_scales (M, K/32), Wimg the
    MX weight image of an (N, K) weight.  `dtype` is the output's (and the residual's) 16-bit type; out_f32 writes float."""
    L.require_gpu(Aq, "Aq")
    m, k = Aq.shape
    if Aq.stride(1) != 1 or not a_scales.is_contiguous() or tuple(a_scales.shape) != (m, k // 32):
        raise L.SpeechLLMError("gemm_mx: Aq rows must be contiguous and a_scales a contiguous (M, K/32) tensor")
    nout = N // 2 if act == L.ACT_SILU_MUL else N
    if out is None:
        out = torch.empty((m, nout), device=Aq.device, dtype=torch.float32 if out_f32 else dtype)
    a = L.GemmMxArgs()
    a.Aq, a.lda, a.a_scales, a.W = L.ptr(Aq), Aq.stride(0), L.ptr(a_scales), L.ptr(Wimg)
    a.C, a.ldc = L.ptr(out), out.stride(0)
    a.residual, a.ldr = L.ptr(residual), (residual.stride(0) if residual is not None else 0)
    a.M, a.N, a.K, a.dtype, a.act, a.out_f32 = m, N, k, L.dtype_code(dtype), act, int(bool(out_f32))
    L.check(L.lib().sl_gemm_mx(C.byref(a), L.stream_ptr()), "sl_gemm_mx")
    return out


def gemm_decode(A: torch.Tensor, Wp: torch.Tensor, N: int, *, residual=None, act: int = L.ACT_NONE, out_f32: bool = False,
                fuse_rms: bool = False, eps: float = 1e-5, rope=None, out: Optional[torch.Tensor] = None,
                split_k: bool = True, rstd_in: Optional[torch.Tensor] = None, rstd_out: Optional[torch.Tensor] = None,
                norm_out: Optional[torch.Tensor] = None, norm_gain: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                w_layout: int = L.W_PACKED) -> torch.Tensor:
    """Decode GEMM on packed weights.  rope = dict(cos, sin, pos, seq, k_cache, v_cache, n_heads, n_kv, max_ctx) for ACT_ROPE_KV.
    split_k: hand the kernel a scratch buffer so that row counts > 64 may split K over blocks (gemm_stream.hip).
    w_layout = W_PACKED_E4M3: Wp is an e4m3 weight image (pack_weight_e4m3), for up to sl_w8_max_rows() rows.
    w_layout = W_PACKED_MXFP4: Wp is an MXFP4 weight image (pack_weight_mxfp4), for up to sl_w4_max_rows() rows."""
    M, K = A.shape
    if act == L.ACT_SILU_MUL:
        n_out = N // 2
    elif act == L.ACT_ROPE_KV:
        n_out = rope["n_heads"] * 128
    else:
        n_out = N
    if out is None:
        out = torch.empty((M, n_out), device=A.device, dtype=torch.float32 if out_f32 else A.dtype)
    a = L.GemmArgs()
    a.A, a.lda = L.ptr(A), A.stride(0)
    a.W, a.ldw = L.ptr(Wp), K
    a.C, a.ldc = L.ptr(out), out.stride(0)
    a.residual, a.ldr = L.ptr(residual), (residual.stride(0) if residual is not None else 0)
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.bias = L.ptr(bias)
    a.dtype, a.act, a.out_f32, a.w_layout = L.dtype_code(A.dtype), act, int(out_f32), int(w_layout)
    f = L.GemmFused()
    f.fuse_rms, f.rms_eps = int(fuse_rms), eps
    f.rstd_in, f.rstd_out = L.ptr(rstd_in), L.ptr(rstd_out)
    f.norm_out, f.norm_gain = L.ptr(norm_out), L.ptr(norm_gain)     # the reduce pass also writes the RMS-normalised rows (sl_gemm_fused.norm_out)
    if rope is not None:
        f.rope_cos, f.rope_sin, f.tok_pos, f.tok_seq = L.ptr(rope["cos"]), L.ptr(rope["sin"]), L.ptr(rope["pos"]), L.ptr(rope["seq"])
        f.k_cache, f.v_cache = L.ptr(rope["k_cache"]), L.ptr(rope["v_cache"])
        f.n_heads, f.n_kv_heads, f.max_ctx = rope["n_heads"], rope["n_kv"], rope["max_ctx"]
        f.reserved = int(rope.get("kv_format", L.KV_MODEL_DTYPE))      # the caches' K/V format (sl_gemm_fused.reserved)
    if split_k:
        need = int(L.lib().sl_gemm_split_workspace_bytes(M, N, K, a.dtype))
        if need > 0:
            ws = _split_ws(A.device, need)
            f.split_ws, f.split_ws_bytes = L.ptr(ws), ws.numel()
    L.check(L.lib().sl_gemm_fused_decode(C.byref(a), C.byref(f), L.stream_ptr()), "sl_gemm_fused_decode")
    return out


_SPLIT_WS = {}


def _split_ws(device, nbytes: int) -> torch.Tensor:
    ws = _SPLIT_WS.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)   # the first 8 KiB hold the K-split fix-up's counters: zero on first use
        _SPLIT_WS[device] = ws
    return ws


def attn_decode_split(q, q_stride, k_cache, v_cache, ctx_len, n_heads, n_kv, D, max_ctx, scale, out=None, ws=None) -> torch.Tensor:
    B = ctx_len.shape[0]
    if out is None:
        out = torch.empty((B, n_heads * D), device=q.device, dtype=q.dtype)
    if ws is None:
        ws = torch.empty(int(L.lib().sl_attn_decode_workspace_bytes(B, n_heads, n_kv, max_ctx)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().sl_attn_decode_split(L.ptr(q), q_stride, L.ptr(k_cache), L.ptr(v_cache), L.ptr(out), L.ptr(ws), L.ptr(ctx_len), B,
                                         n_heads, n_kv, D, max_ctx, scale, L.dtype_code(q.dtype), L.stream_ptr()), "sl_attn_decode_split")
    return out


def attn_decode_split_ex(q, q_stride, k_cache, v_cache, ctx_len, n_heads, n_kv, D, max_ctx, scale, kv_format: int = L.KV_MODEL_DTYPE,
                         shared_prefix: int = 0, out=None, ws=None) -> torch.Tensor:
    """attn_decode_split on a cache of either format (KV_FP8_E4M3: uint8 caches of e4m3 rows); positions below shared_prefix come from slot 0."""
    B = ctx_len.shape[0]
    if out is None:
        out = torch.empty((B, n_heads * D), device=q.device, dtype=q.dtype)
    if ws is None:
        ws = torch.empty(int(L.lib().sl_attn_decode_workspace_bytes(B, n_heads, n_kv, max_ctx)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().sl_attn_decode_split_ex(L.ptr(q), q_stride, L.ptr(k_cache), L.ptr(v_cache), L.ptr(out), L.ptr(ws), L.ptr(ctx_len), B,
                                            n_heads, n_kv, D, max_ctx, scale, L.dtype_code(q.dtype), int(kv_format), int(shared_prefix),
                                            L.stream_ptr()), "sl_attn_decode_split_ex")
    return out


def attn_group_plan(prefix_slot: Sequence[int], prefix_len: Sequence[int], rep: int):
    """sl_attn_group_plan_host (pure host): -> (list of B (prefix_slot, prefix_len, [rows]) records, n_used, the ctypes array)."""
    B = len(prefix_slot)
    recs = (L.AttnGroup * max(B, 1))()
    n_used = C.c_int32(0)
    L.check(L.lib().sl_attn_group_plan_host((C.c_int32 * max(B, 1))(*[int(v) for v in prefix_slot]), (C.c_int32 * max(B, 1))(*[int(v) for v in prefix_len]),
                                            B, int(rep), recs, C.byref(n_used)), "sl_attn_group_plan_host")
    out = [(int(r.prefix_slot), int(r.prefix_len), [int(r.rows[i]) for i in range(int(r.n_rows))]) for r in recs[:B]]
    return out, int(n_used.value), recs


def attn_decode_grouped(q, q_stride, k_cache, v_cache, ctx_len, prefix_slot: Sequence[int], prefix_len: Sequence[int], row_slot0: int, n_heads, n_kv, D,
                        max_ctx, scale, kv_format: int = L.KV_MODEL_DTYPE, out=None) -> torch.Tensor:
    """Decode attention of rows that share prompts (sl_attn_decode_grouped): row b attends [0, prefix_len[b]) of slot prefix_slot[b] and
    [prefix_len[b], ctx_len[b]) of slot row_slot0 + b.  prefix_slot / prefix_len are host sequences: the records are planned here."""
    B = ctx_len.shape[0]
    if out is None:
        out = torch.empty((B, n_heads * D), device=q.device, dtype=q.dtype)
    _, _, recs = attn_group_plan(prefix_slot, prefix_len, n_heads // n_kv)
    groups = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.int32).to(q.device)
    plen = torch.tensor([int(v) for v in prefix_len], dtype=torch.int32).to(q.device)
    ws = torch.empty(int(L.lib().sl_attn_decode_grouped_workspace_bytes(B, n_heads)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().sl_attn_decode_grouped(L.ptr(q), q_stride, L.ptr(k_cache), L.ptr(v_cache), L.ptr(out), L.ptr(ws), L.ptr(ctx_len), L.ptr(plen),
                                           L.ptr(groups), B, int(row_slot0), n_heads, n_kv, D, max_ctx, scale, L.dtype_code(q.dtype), int(kv_format),
                                           L.stream_ptr()), "sl_attn_decode_grouped")
    return out


def kv_cache_bytes(model_struct, slots: int, max_ctx: int, kv_format: int = L.KV_MODEL_DTYPE) -> int:
    """Bytes of ONE of the two caches (sl_kv_cache_bytes); raises where the library refuses the combination."""
    n = int(L.lib().sl_kv_cache_bytes(C.byref(model_struct), int(slots), int(max_ctx), int(kv_format)))
    if n == 0:
        L.check(-1, "sl_kv_cache_bytes")
    return n


# ---------------------------------------------------------------------------------------------
# training-side wrappers (sl_gemm_ex and train_ops.hip)
# ---------------------------------------------------------------------------------------------
def gemm_ex(A, W, *, M: int, N: int, K: int, lda: int, ldw: int, out: torch.Tensor, ldc: Optional[int] = None, bias=None,
            residual=None, ldr: int = 0, act: int = L.ACT_NONE, out_f32: bool = False, trans_a: bool = False, trans_w: bool = False,
            residual_f32: bool = False, aux_out=None, batch: int = 1, strideA: int = 0, strideW: int = 0, strideC: int = 0,
            strideBias: int = 0, strideR: int = 0, a_off: int = 0, w_off: int = 0, c_off: int = 0, r_off: int = 0,
            dtype: Optional[torch.dtype] = None, groups: Optional[torch.Tensor] = None, w_mod: int = 1, groups_ext: bool = False,
            ln_mr=None, ln_u=None, ln_c=None, stats_out=None, sk_ws: Optional[torch.Tensor] = None,
            post_op: int = 0, drop_p: float = 0.0, drop_seed: int = 0, drop_ld: int = 0, post_in=None, post_ld: int = 0, colsum_out=None,
            deferred_splits=None):
    """Raw-pointer GEMM with every backward feature; *_off are element offsets into the tensors.  ln_mr/ln_u/ln_c: the
    LayerNorm-folded consumer epilogue; stats_out: per-64-column {sum, sum of squares} of the stored rows (speechllm.h).
    post_op / drop_* / post_in / colsum_out: the training tape's epilogue fusions (sl_gemm_ex_args, ABI 7).
    deferred_splits: a ctypes c_int32 the library sets to the number of K runs it left un-reduced in sk_ws (0: `out` was written)."""
    dt = dtype or A.dtype
    esz = 4 if dt == torch.float32 else 2
    a = L.GemmArgs()
    a.A, a.lda, a.strideA = A.data_ptr() + a_off * esz, lda, strideA
    a.W, a.ldw, a.strideW = W.data_ptr() + w_off * esz, ldw, strideW
    a.C, a.ldc, a.strideC = out.data_ptr() + c_off * (4 if out_f32 else esz), (ldc if ldc is not None else out.stride(0)), strideC
    a.bias, a.strideBias = L.ptr(bias), strideBias
    a.residual = 0 if residual is None else residual.data_ptr() + r_off * (4 if residual_f32 else esz)
    a.ldr, a.strideR = ldr, strideR
    a.M, a.N, a.K, a.batch = M, N, K, batch
    a.dtype, a.act, a.out_f32, a.w_layout = L.dtype_code(dt), act, int(out_f32), L.W_ROWMAJOR
    e = L.GemmEx()
    e.trans_a, e.trans_w, e.residual_f32, e.aux_out = int(trans_a), int(trans_w), int(residual_f32), L.ptr(aux_out)
    e.groups, e.w_mod, e.groups_ext = L.ptr(groups), w_mod, int(groups_ext)
    e.ln_mr, e.ln_u, e.ln_c, e.stats_out = L.ptr(ln_mr), L.ptr(ln_u), L.ptr(ln_c), L.ptr(stats_out)
    if sk_ws is not None:       # stream-K workspace (streamk_workspace): zeroed once, one per stream
        e.sk_ws, e.sk_ws_bytes = sk_ws.data_ptr(), sk_ws.numel() * sk_ws.element_size()
    e.post_op, e.drop_p, e.drop_seed, e.drop_ld = int(post_op), float(drop_p), int(drop_seed) & 0xFFFFFFFFFFFFFFFF, int(drop_ld)
    e.post_in, e.post_ld, e.colsum_out = L.ptr(post_in), int(post_ld), L.ptr(colsum_out)
    if deferred_splits is not None:
        e.deferred_splits = C.cast(C.byref(deferred_splits), C.c_void_p)
    L.check(L.lib().sl_gemm_ex(C.byref(a), C.byref(e), L.stream_ptr()), "sl_gemm_ex")
    return out


def streamk_workspace(device) -> torch.Tensor:
    """A zeroed stream-K workspace (sl_gemm_ex_args.sk_ws): one per stream that launches GEMMs."""
    return torch.zeros(int(L.lib().sl_gemm_streamk_workspace_bytes()), device=device, dtype=torch.uint8)


def layernorm_stats(x: torch.Tensor, eps: float) -> torch.Tensor:
    """(rows, 2) fp32 {mean, rstd} of every row of x (sl_layernorm_stats) — the first layer's input of the folded encoder."""
    rows, cols = x.shape
    mr = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
    L.check(L.lib().sl_layernorm_stats(L.ptr(x), rows, cols, eps, L.ptr(mr), L.dtype_code(x.dtype), L.stream_ptr()), "sl_layernorm_stats")
    return mr


def layernorm_stats_finalize(stats: torch.Tensor, cols: int, eps: float) -> torch.Tensor:
    """(rows, 2) fp32 {mean, rstd} from a producer GEMM's (rows, cols/64, 2) segment sums (sl_layernorm_stats_finalize)."""
    rows, segs = stats.shape[0], stats.shape[1]
    mr = torch.empty((rows, 2), device=stats.device, dtype=torch.float32)
    L.check(L.lib().sl_layernorm_stats_finalize(L.ptr(stats), segs, rows, cols, eps, L.ptr(mr), L.stream_ptr()), "sl_layernorm_stats_finalize")
    return mr


def transpose_pad(x: torch.Tensor, rows: int, cols: int, ld_out: Optional[int] = None) -> torch.Tensor:
    """(cols, ld_out) = x[:rows, :cols]^T, zero-filled beyond `rows` (sl_transpose_pad)."""
    ld_out = rows if ld_out is None else ld_out
    vec = 4 if x.dtype == torch.float32 else 8
    ldy = (ld_out + vec - 1) // vec * vec
    y = torch.empty((cols, ldy), device=x.device, dtype=x.dtype)
    L.check(L.lib().sl_transpose_pad(L.ptr(x), x.stride(0), L.ptr(y), ldy, rows, cols, ld_out, L.dtype_code(x.dtype), L.stream_ptr()), "sl_transpose_pad")
    return y if ldy == ld_out else y[:, :ld_out]


def dgrad(dY: torch.Tensor, W: torch.Tensor, out: Optional[torch.Tensor] = None, wt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX (M, K_in) = dY (M, N_out) . W (N_out, K_in).  wt: W stored transposed (K_in, N_out), contiguous — then the
    product is a plain K-contiguous GEMM and runs the LDS-DMA tiled kernels instead of the transposed-operand loader."""
    if wt is not None:
        return gemm(dY, wt, out=out)
    M, Nout = dY.shape
    Kin = W.shape[1]
    if out is None:
        out = torch.empty((M, Kin), device=dY.device, dtype=dY.dtype)
    return gemm_ex(dY, W, M=M, N=Kin, K=Nout, lda=dY.stride(0), ldw=W.stride(0), out=out, trans_w=True)


def wgrad_acc(dY: torch.Tensor, X: torch.Tensor, dW: torch.Tensor, *, ldx: Optional[int] = None, Kin: Optional[int] = None,
              M: Optional[int] = None, db: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW (N_out, K_in) fp32 += dY^T (N_out, M) . X (M, K_in); X rows may overlap (ldx < K_in: implicit-GEMM conv windows).
    db (fp32, N_out): the bias gradient db += colsum(dY) — inside the token-major product where that kernel runs, else a sl_colsum launch."""
    M = dY.shape[0] if M is None else M
    Nout = dY.shape[1]
    Kin = X.shape[1] if Kin is None else Kin
    tt = (ldx is None and M >= 256 and dY.dtype == torch.bfloat16 and Nout % 128 == 0 and Kin % 128 == 0 and dY.stride(0) % 8 == 0 and X.stride(0) % 8 == 0
          and dY.data_ptr() % 16 == 0 and X.data_ptr() % 16 == 0 and os.environ.get("SL_WGRAD_TR", "1") != "0")
    if db is not None and not (tt and os.environ.get("SL_TAPE_FUSE", "1") != "0"):
        colsum_acc(dY[:M], db)
        db = None
    if tt:
        return gemm_ex(dY, X, M=Nout, N=Kin, K=M, lda=dY.stride(0), ldw=X.stride(0), out=dW, ldc=dW.stride(0), residual=dW, ldr=dW.stride(0),
                       out_f32=True, residual_f32=True, trans_a=True, trans_w=True, dtype=dY.dtype, colsum_out=db)
    if ldx is None and M >= 256:
        # plain Linear: contract over token rows on K-contiguous copies (dY^T, X^T zero-padded to a whole number of K slabs) so
        # the product runs the LDS-DMA tiled kernels; the doubly-transposed register loader measured ~100 TF/s on these shapes
        Mp = (M + 63) // 64 * 64
        dYT = transpose_pad(dY, M, Nout, Mp)
        XT = transpose_pad(X, M, Kin, Mp)
        return gemm_ex(dYT, XT, M=Nout, N=Kin, K=Mp, lda=Mp, ldw=Mp, out=dW, ldc=dW.stride(0), residual=dW, ldr=dW.stride(0), out_f32=True,
                       residual_f32=True, dtype=dY.dtype)
    return gemm_ex(dY, X, M=Nout, N=Kin, K=M, lda=dY.stride(0), ldw=(X.stride(0) if ldx is None else ldx), out=dW, ldc=dW.stride(0),
                   residual=dW, ldr=dW.stride(0), out_f32=True, residual_f32=True, trans_a=True, trans_w=True, dtype=dY.dtype)


def gelu_bwd(dy, pre):
    dx = torch.empty_like(dy)
    L.check(L.lib().sl_gelu_bwd(L.ptr(dy), L.ptr(pre), L.ptr(dx), dy.numel(), L.dtype_code(dy.dtype), L.stream_ptr()), "sl_gelu_bwd")
    return dx


def axpby(x, y, a=1.0, b=1.0):
    L.check(L.lib().sl_axpby(L.ptr(x), L.ptr(y), a, b, y.numel(), L.dtype_code(y.dtype), L.stream_ptr()), "sl_axpby")
    return y


def dropout(x: torch.Tensor, p: float, seed: int, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (residual or 0) + keep * x / (1 - p) with the counter-based mask of sl_dropout (same seed -> same mask: the
    backward pass calls this on the gradient).  `out` may alias x."""
    L.require_gpu(x, "x")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().sl_dropout(L.ptr(x), L.ptr(residual), L.ptr(out), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, L.dtype_code(x.dtype),
                               L.stream_ptr()), "sl_dropout")
    return out


def dropout_keep_at(idx, p: float, seed: int) -> "torch.Tensor":
    """Host restatement of the counter-based dropout mask (common.h dropout_keep) at arbitrary 64-bit element indices: bool, the shape
    of idx (a numpy array or a torch tensor of non-negative integers).  sl_dropout's index is the element's offset; the attention
    kernels' is ((query row * n_heads + head) << 16) | key."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)

    def lowbias32(v):
        v = v & m32
        v ^= v >> np.uint64(16); v = (v * np.uint64(0x7feb352d)) & m32
        v ^= v >> np.uint64(15); v = (v * np.uint64(0x846ca68b)) & m32
        v ^= v >> np.uint64(16)
        return v

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = (idx.cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)).astype(np.uint64)
    h = lowbias32((i & m32) ^ lowbias32((i >> np.uint64(32)) ^ np.uint64(seed & 0xFFFFFFFF)) ^ np.uint64(seed >> 32))
    thr = np.uint64(int(float(np.float32(p)) * 16777216.0))
    return torch.from_numpy((h >> np.uint64(8)) >= thr)


def dropout_keep_mask(n: int, p: float, seed: int) -> "torch.Tensor":
    """Host restatement of sl_dropout's mask (bool, n elements) — used by the tests' oracle to apply identical masks."""
    import numpy as np
    return dropout_keep_at(np.arange(n, dtype=np.uint64), p, seed)


def silu_mul(gu):
    M, F2 = gu.shape
    out = torch.empty((M, F2 // 2), device=gu.device, dtype=gu.dtype)
    L.check(L.lib().sl_silu_mul(L.ptr(gu), L.ptr(out), M, F2 // 2, L.dtype_code(gu.dtype), L.stream_ptr()), "sl_silu_mul")
    return out


def silu_mul_bwd(gu, dy):
    dgu = torch.empty_like(gu)
    L.check(L.lib().sl_silu_mul_bwd(L.ptr(gu), L.ptr(dy), L.ptr(dgu), gu.shape[0], gu.shape[1] // 2, L.dtype_code(gu.dtype), L.stream_ptr()),
            "sl_silu_mul_bwd")
    return dgu


def rope_inplace(x, tok_pos, cos, sin, heads, n_rot, D, inverse=False):
    L.check(L.lib().sl_rope_inplace(L.ptr(x), L.ptr(tok_pos), L.ptr(cos), L.ptr(sin), x.shape[0], heads, n_rot, D, int(inverse),
                                    L.dtype_code(x.dtype), L.stream_ptr()), "sl_rope_inplace")
    return x


_LN_WS = {}


def layernorm_bwd(x, g, b, dy, eps, dgamma=None, dbeta=None, gelu=False):
    dx = torch.empty_like(dy)
    rows = x.numel() // x.shape[-1]
    need = int(L.lib().sl_layernorm_bwd_ws_bytes(rows, x.shape[-1])) if dgamma is not None and dbeta is not None else 0
    ws = None
    if need:                                  # scratch for the blocks' dgamma / dbeta records (one buffer per device, grown on demand)
        ws = _LN_WS.get(x.device)
        if ws is None or ws.numel() < need:
            ws = _LN_WS[x.device] = torch.empty(need, dtype=torch.uint8, device=x.device)
    L.check(L.lib().sl_layernorm_bwd_ws(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(dy), L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), rows, x.shape[-1], eps,
                                        int(gelu), L.dtype_code(x.dtype), L.ptr(ws), ws.numel() if ws is not None else 0, L.stream_ptr()),
            "sl_layernorm_bwd_ws")
    return dx


def rmsnorm_bwd(x, w, dy, eps):
    dx = torch.empty_like(dy)
    rows = x.numel() // x.shape[-1]
    L.check(L.lib().sl_rmsnorm_bwd(L.ptr(x), L.ptr(w), L.ptr(dy), L.ptr(dx), rows, x.shape[-1], eps, L.dtype_code(x.dtype), L.stream_ptr()),
            "sl_rmsnorm_bwd")
    return dx


def colsum_acc(x, out_f32):
    L.check(L.lib().sl_colsum(L.ptr(x), x.stride(0), L.ptr(out_f32), x.shape[0], x.shape[1], L.dtype_code(x.dtype), L.stream_ptr()), "sl_colsum")
    return out_f32


def softmax_rows(S, n_mats, rows, cols, ld, scale, causal, dtype):
    P = torch.empty((n_mats, rows, ld), device=S.device, dtype=dtype)
    L.check(L.lib().sl_softmax_rows(L.ptr(S), L.ptr(P), n_mats, rows, cols, ld, scale, int(causal), L.dtype_code(dtype), L.stream_ptr()),
            "sl_softmax_rows")
    return P


def softmax_bwd(P, dP, cols, scale):
    dS = torch.empty_like(P)
    nrows = P.shape[0] * P.shape[1]
    L.check(L.lib().sl_softmax_bwd(L.ptr(P), L.ptr(dP), L.ptr(dS), nrows, cols, P.shape[2], scale, L.dtype_code(P.dtype), L.stream_ptr()),
            "sl_softmax_bwd")
    return dS


def softmax_rows_var(S, P, n_mats, rows_per_mat, mat_dim, ld, scale, causal, dtype):
    L.check(L.lib().sl_softmax_rows_var(L.ptr(S), L.ptr(P), n_mats, rows_per_mat, L.ptr(mat_dim), ld, scale, int(causal), L.dtype_code(dtype),
                                        L.stream_ptr()), "sl_softmax_rows_var")
    return P


def softmax_bwd_var(P, dP, dS, n_mats, rows_per_mat, mat_dim, ld, scale):
    L.check(L.lib().sl_softmax_bwd_var(L.ptr(P), L.ptr(dP), L.ptr(dS), n_mats, rows_per_mat, L.ptr(mat_dim), ld, scale, L.dtype_code(P.dtype),
                                       L.stream_ptr()), "sl_softmax_bwd_var")
    return dS


def ce_loss(logits, labels, coef, loss, dlogits=None, accumulate=False, dtype=torch.float32):
    L.check(L.lib().sl_ce_loss(L.ptr(logits), L.ptr(labels), logits.shape[0], logits.shape[1], coef, L.ptr(loss), L.ptr(dlogits),
                               int(accumulate), L.dtype_code(dtype), L.stream_ptr()), "sl_ce_loss")


def soft_ce_loss(student, teacher, coef, loss, dstudent=None, accumulate=False, dtype=torch.float32):
    L.check(L.lib().sl_soft_ce_loss(L.ptr(student), L.ptr(teacher), student.shape[0], student.shape[1], coef, L.ptr(loss), L.ptr(dstudent),
                                    int(accumulate), L.dtype_code(dtype), L.stream_ptr()), "sl_soft_ce_loss")


def mse_loss(a, b, coef, loss, da=None, accumulate=False):
    L.check(L.lib().sl_mse_loss(L.ptr(a), L.ptr(b), a.numel(), coef, L.ptr(loss), L.ptr(da), int(accumulate), L.dtype_code(a.dtype),
                                L.stream_ptr()), "sl_mse_loss")


def avgpool_bwd(dy, T, kernel, stride, out=None):
    """out (optional): the (T, H) rows of a packed buffer the gradient is written into (no temporary + copy per utterance)."""
    P, H = dy.shape
    dx = torch.empty((T, H), device=dy.device, dtype=dy.dtype) if out is None else out
    assert dx.is_contiguous() and tuple(dx.shape) == (T, H)
    L.check(L.lib().sl_avgpool_bwd(L.ptr(dy), L.ptr(dx), T, H, kernel, stride, P, L.dtype_code(dy.dtype), L.stream_ptr()), "sl_avgpool_bwd")
    return dx


def col2im(dcol, Lin, Cc, k, s, out=None):
    """out (optional): the (Lin, Cc) rows of a packed buffer the gradient is written into (no temporary + copy per utterance)."""
    dx = torch.empty((Lin, Cc), device=dcol.device, dtype=dcol.dtype) if out is None else out
    assert dx.is_contiguous() and tuple(dx.shape) == (Lin, Cc)
    L.check(L.lib().sl_col2im(L.ptr(dcol), L.ptr(dx), Lin, dcol.shape[0], Cc, k, s, L.dtype_code(dcol.dtype), L.stream_ptr()), "sl_col2im")
    return dx


def col2im_batch(dcol, out, src_rows: Sequence[int], dst_rows: Sequence[int], src_off: Sequence[int], dst_off: Sequence[int], Cc: int, k: int, s: int):
    """sl_col2im for every utterance of a packed batch in one launch: utterance u's windows are rows src_off[u] .. + src_rows[u] of dcol (k * Cc wide), its
    gradient rows dst_off[u] .. + dst_rows[u] of `out` (Cc wide)."""
    desc = L.h2d([[src_rows[u], dst_rows[u], src_off[u], dst_off[u]] for u in range(len(src_rows))], torch.int64, dcol.device)
    L.check(L.lib().sl_col2im_batch(L.ptr(dcol), L.ptr(out), desc.data_ptr(), len(src_rows), max(int(n) for n in dst_rows), Cc, k, s, L.dtype_code(dcol.dtype),
                                    L.stream_ptr()), "sl_col2im_batch")
    return out


def avgpool_bwd_batch(dy, out, P: Sequence[int], T: Sequence[int], src_off: Sequence[int], dst_off: Sequence[int], kernel: int, stride: int):
    """sl_avgpool_bwd for every utterance of a packed batch in one launch (rows src_off[u] .. + P[u] of dy -> rows dst_off[u] .. + T[u] of out)."""
    desc = L.h2d([[P[u], T[u], src_off[u], dst_off[u]] for u in range(len(P))], torch.int64, dy.device)
    L.check(L.lib().sl_avgpool_bwd_batch(L.ptr(dy), L.ptr(out), desc.data_ptr(), len(P), max(int(n) for n in T), dy.shape[1], kernel, stride,
                                         L.dtype_code(dy.dtype), L.stream_ptr()), "sl_avgpool_bwd_batch")
    return out


def hubert_conv0_bwd_batch(waves: Sequence[torch.Tensor], w, bias, gamma, beta, dy, row_offsets: Sequence[int], dw, dbias, dgamma, dbeta, k=10, stride=5,
                           eps=1e-5):
    """conv0 + LayerNorm + GELU backward of every utterance of a packed batch in ONE launch (dy rows row_offsets[u]..)."""
    dev = dy.device
    flat = torch.cat([wv.reshape(-1) for wv in waves]).contiguous()
    soff, spref = [0], [0]
    for u, wv in enumerate(waves):
        soff.append(soff[-1] + wv.numel())
        spref.append(spref[-1] + (row_offsets[u + 1] - row_offsets[u] + 23) // 24)        # strips of 24 time steps (k=10, s=5)
    desc = L.h2d([soff, list(row_offsets), spref], torch.int64, dev)
    L.check(L.lib().sl_hubert_conv0_bwd_batch(L.ptr(flat), desc[0].data_ptr(), desc[1].data_ptr(), desc[2].data_ptr(), len(waves), spref[-1], L.ptr(w),
                                              L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(dy), w.shape[0], k, stride, eps, L.ptr(dw), L.ptr(dbias),
                                              L.ptr(dgamma), L.ptr(dbeta), L.dtype_code(dy.dtype), L.stream_ptr()), "sl_hubert_conv0_bwd_batch")


def hubert_conv0_bwd(wave, w, bias, gamma, beta, dy, dw, dbias, dgamma, dbeta, k=10, stride=5, eps=1e-5):
    L.check(L.lib().sl_hubert_conv0_bwd(L.ptr(wave), wave.numel(), L.ptr(w), L.ptr(bias), L.ptr(gamma), L.ptr(beta), L.ptr(dy), w.shape[0], k,
                                        stride, eps, L.ptr(dw), L.ptr(dbias), L.ptr(dgamma), L.ptr(dbeta), L.dtype_code(dy.dtype),
                                        L.stream_ptr()), "sl_hubert_conv0_bwd")


def kd_logit_losses(student, teacher, labels, row_coef, row_slot, losses, dstudent, dtype):
    """All next-token / soft cross-entropy terms of a window in one launch (sl_kd_logit_losses)."""
    L.check(L.lib().sl_kd_logit_losses(L.ptr(student), L.ptr(teacher), L.ptr(labels), L.ptr(row_coef), L.ptr(row_slot), student.shape[0], student.shape[1],
                                       L.ptr(losses), losses.stride(0), L.ptr(dstudent), L.dtype_code(dtype), L.stream_ptr()), "sl_kd_logit_losses")


def kd_mse_rows(a, b, row_coef, row_slot, losses, loss_col, da=None):
    """Feature-distillation MSE of one tap over every utterance's tail rows in one launch (sl_kd_mse_rows)."""
    L.check(L.lib().sl_kd_mse_rows(L.ptr(a), L.ptr(b), L.ptr(row_coef), L.ptr(row_slot), a.shape[0], a.shape[1], L.ptr(losses), losses.stride(0), loss_col,
                                   L.ptr(da), L.dtype_code(a.dtype), L.stream_ptr()), "sl_kd_mse_rows")


def sample_select(logits, temperature, top_k, top_p, seed, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids) -> None:
    """sl_sample_select: HF's temperature / top-k / top-p warpers + one reproducible draw per row, then greedy_select's bookkeeping."""
    B, V = logits.shape
    choice = torch.empty(B, dtype=torch.int32, device=logits.device)
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_sample_select(L.ptr(logits), B, V, float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, eos, len(eos_ids), pad_id,
                                     int(use_eos), *state, L.ptr(choice), L.stream_ptr()), "sl_sample_select")


def sample_uniform(seed: int, row: int, step: int) -> float:
    """Host restatement of the uniform sl_sample_select draws for (seed, row, step) — the tests rebuild the inverse-CDF pick with it."""
    m32 = 0xFFFFFFFF

    def lowbias32(v):
        v &= m32
        v ^= v >> 16; v = (v * 0x7feb352d) & m32
        v ^= v >> 15; v = (v * 0x846ca68b) & m32
        v ^= v >> 16
        return v

    seed &= 0xFFFFFFFFFFFFFFFF
    h = lowbias32((step & m32) ^ lowbias32((row & m32) ^ (seed & m32)) ^ (seed >> 32))
    return (h >> 8) / 16777216.0


# ---- token log-probabilities (speechllm.h: sl_gemm_top1_lse and the _sc select entries)
def gemm_top1_lse(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, out=None):
    """gemm_top1 plus the third plane: returns (val, idx, sum), each (ceil(N / 64), M); sum[g][m] = sum over group g's columns of
    exp(v - val[g][m]).  out: optional (val, idx, sum) buffers to write into (the tests put guard bands around them)."""
    L.require_gpu(A, "A"); L.require_gpu(W, "W")
    M, K = A.shape
    N = W.shape[0]
    ng = (N + 63) // 64
    if out is None:
        out = (torch.empty((ng, M), device=A.device, dtype=torch.float32), torch.empty((ng, M), device=A.device, dtype=torch.int32),
               torch.empty((ng, M), device=A.device, dtype=torch.float32))
    val, idx, ssum = out
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = L.ptr(A), A.stride(0), L.ptr(W), W.stride(0), None, N
    a.bias = L.ptr(bias)
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.dtype, a.act, a.out_f32 = L.dtype_code(A.dtype), L.ACT_NONE, 1
    ex = L.GemmEx()
    ex.w_mod, ex.amax_val, ex.amax_idx = 1, L.ptr(val), L.ptr(idx)
    L.check(L.lib().sl_gemm_top1_lse(C.byref(a), C.byref(ex), L.ptr(ssum), L.stream_ptr()), "sl_gemm_top1_lse")
    return val, idx, ssum


def greedy_select_sc(logits, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, logprobs) -> None:
    B, V = logits.shape
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_greedy_select_sc(L.ptr(logits), B, V, eos, len(eos_ids), pad_id, int(use_eos), *state, L.ptr(logprobs), L.stream_ptr()),
            "sl_greedy_select_sc")


def greedy_select_partial_sc(val, idx, ssum, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids, logprobs,
                             advance_ctx=True) -> None:
    ng, B = val.shape
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_greedy_select_partial_sc(L.ptr(val), L.ptr(idx), L.ptr(ssum), ng, B, eos, len(eos_ids), pad_id, int(use_eos), int(advance_ctx),
                                                *state, L.ptr(logprobs), L.stream_ptr()), "sl_greedy_select_partial_sc")


def sample_select_sc(logits, temperature, top_k, top_p, seed, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids,
                     logprobs) -> None:
    B, V = logits.shape
    choice = torch.empty(B, dtype=torch.int32, device=logits.device)
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_sample_select_sc(L.ptr(logits), B, V, float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, eos, len(eos_ids),
                                        pad_id, int(use_eos), *state, L.ptr(choice), L.ptr(logprobs), L.stream_ptr()), "sl_sample_select_sc")


def sample_select_w(logits, temperature, top_k, top_p, seed, eos_ids, pad_id, use_eos, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids,
                    logprobs=None, warp=None) -> None:
    """sl_sample_select_w: sample_select_sc (logprobs None: sample_select) with HF's min_p / typical_p / epsilon_cutoff / eta_cutoff behind
    top-p.  warp: an L.WarpOpts (passed as it is, so that the library's own range checks can be reached), a dict of the four names, or None."""
    B, V = logits.shape
    choice = torch.empty(B, dtype=torch.int32, device=logits.device)
    w = warp if isinstance(warp, L.WarpOpts) else L.warp_opts(warp)
    eos, state = _select_state(eos_ids, unfinished, ctx_len, gen_count, finish_len, next_ids, out_ids)
    L.check(L.lib().sl_sample_select_w(L.ptr(logits), B, V, float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, eos, len(eos_ids),
                                       pad_id, int(use_eos), *state, L.ptr(choice), None if logprobs is None else L.ptr(logprobs), L.stream_ptr(),
                                       None if w is None else C.byref(w)), "sl_sample_select_w")


# ---- teacher-forced scoring (speechllm.h: sl_gemm_top1_lse_tgt, sl_score_*)
def gemm_top1_lse_tgt(A: torch.Tensor, W: torch.Tensor, tgt_col: torch.Tensor, bias: Optional[torch.Tensor] = None, out=None, tgt_val=None):
    """gemm_top1_lse plus the wanted column's value per row: returns (val, idx, sum, tgt_val); tgt_val[m] = the logit at (m, tgt_col[m]),
    untouched where tgt_col[m] lies outside [0, N).  out / tgt_val: optional buffers to write into (tgt_val is NOT initialised here when
    given: the caller's contents survive in the rows nobody writes)."""
    L.require_gpu(A, "A"); L.require_gpu(W, "W"); L.require_gpu(tgt_col, "tgt_col")
    M, K = A.shape
    N = W.shape[0]
    ng = (N + 63) // 64
    if tgt_col.dtype != torch.int32 or tgt_col.numel() != M:
        raise L.SpeechLLMError(f"tgt_col must hold M={M} int32 columns")
    if out is None:
        out = (torch.empty((ng, M), device=A.device, dtype=torch.float32), torch.empty((ng, M), device=A.device, dtype=torch.int32),
               torch.empty((ng, M), device=A.device, dtype=torch.float32))
    if tgt_val is None:
        tgt_val = torch.zeros(M, device=A.device, dtype=torch.float32)
    val, idx, ssum = out
    a = L.GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = L.ptr(A), A.stride(0), L.ptr(W), W.stride(0), None, N
    a.bias = L.ptr(bias)
    a.M, a.N, a.K, a.batch = M, N, K, 1
    a.dtype, a.act, a.out_f32 = L.dtype_code(A.dtype), L.ACT_NONE, 1
    ex = L.GemmEx()
    ex.w_mod, ex.amax_val, ex.amax_idx = 1, L.ptr(val), L.ptr(idx)
    L.check(L.lib().sl_gemm_top1_lse_tgt(C.byref(a), C.byref(ex), L.ptr(ssum), L.ptr(tgt_col), L.ptr(tgt_val), L.stream_ptr()), "sl_gemm_top1_lse_tgt")
    return val, idx, ssum, tgt_val


def score_finalize(val, idx, ssum, tgt_val, labels, vocab: int, logprob=None, top1=None):
    """the three planes (ceil(vocab / 64), rows) + the labels' logits -> (logprob (rows) float32, top1 (rows) int32); labels outside
    [0, vocab) are ignored: 0.0, tgt_val not read."""
    ng, rows = val.shape
    if logprob is None:
        logprob = torch.empty(rows, device=val.device, dtype=torch.float32)
    if top1 is None:
        top1 = torch.empty(rows, device=val.device, dtype=torch.int32)
    L.check(L.lib().sl_score_finalize(L.ptr(val), L.ptr(idx), L.ptr(ssum), ng, int(vocab), L.ptr(tgt_val), L.ptr(labels), rows, L.ptr(logprob), L.ptr(top1),
                                      L.stream_ptr()), "sl_score_finalize")
    return logprob, top1


def score_rows(logits: torch.Tensor, labels: torch.Tensor, logprob=None, top1=None):
    """fp32 logits (rows, V) (rows may be strided) -> (logprob, top1) as score_finalize gives them; logits[r][label] is not read for an ignored label"""
    L.require_gpu(labels, "labels")
    if logits.dtype != torch.float32 or logits.stride(1) != 1 or labels.dtype != torch.int32:
        raise L.SpeechLLMError("score_rows takes float32 logits with contiguous rows and int32 labels")
    rows, V = logits.shape
    if logprob is None:
        logprob = torch.empty(rows, device=logits.device, dtype=torch.float32)
    if top1 is None:
        top1 = torch.empty(rows, device=logits.device, dtype=torch.int32)
    L.check(L.lib().sl_score_rows(L.ptr(logits), logits.stride(0), L.ptr(labels), rows, V, L.ptr(logprob), L.ptr(top1), L.stream_ptr()), "sl_score_rows")
    return logprob, top1


def score_segment_sums(logprob, labels, top1, row_offsets, vocab: int, out=None):
    """per sequence over rows [row_offsets[s], row_offsets[s + 1]): (sum of logprob float32, counted rows int32, counted rows whose top1 is the
    label int32); ignored rows count in none"""
    nseq = row_offsets.numel() - 1
    if out is None:
        out = (torch.empty(nseq, device=logprob.device, dtype=torch.float32), torch.empty(nseq, device=logprob.device, dtype=torch.int32),
               torch.empty(nseq, device=logprob.device, dtype=torch.int32))
    ssum, cnt, hit = out
    L.check(L.lib().sl_score_segment_sums(L.ptr(logprob), L.ptr(labels), L.ptr(top1), L.ptr(row_offsets), nseq, int(vocab), L.ptr(ssum), L.ptr(cnt), L.ptr(hit),
                                          L.stream_ptr()), "sl_score_segment_sums")
    return ssum, cnt, hit


# -- stack / ctc_pool downsampling of a packed ragged batch (ref:model/audio_encoder.py:65-85) -----------------------------------
def segment_ranges_pack(ranges_per_utt, frames: Sequence[int]):
    """ctc_pool ranges as the dataset stores them (one list of (start, end) per utterance, utterance-relative) -> (packed int64 CPU tensor
    (R, 2) of {first row, end row} in packed-frame coordinates, per-utterance counts).  Pure host routine (sl_segment_ranges_host): each pair is
    clamped to its utterance's frames like a tensor slice; a pair that is empty afterwards raises SpeechLLMError naming the utterance and the range."""
    if ranges_per_utt is None or len(ranges_per_utt) != len(frames):
        raise L.SpeechLLMError(f"ctc_pool needs one list of (start, end) ranges per utterance: got {0 if ranges_per_utt is None else len(ranges_per_utt)} "
                               f"for {len(frames)} utterances")
    per = [torch.as_tensor(r, dtype=torch.int64).reshape(-1, 2) for r in ranges_per_utt]
    counts = [int(p_.shape[0]) for p_ in per]
    rel = torch.cat(per).contiguous() if per else torch.zeros((0, 2), dtype=torch.int64)
    packed = torch.empty_like(rel)
    cnt = (C.c_int32 * len(frames))(*counts)
    frm = (C.c_int64 * len(frames))(*[int(t) for t in frames])
    L.check(L.lib().sl_segment_ranges_host(rel.data_ptr(), C.cast(cnt, C.c_void_p), C.cast(frm, C.c_void_p), len(frames), packed.data_ptr()),
            "sl_segment_ranges_host")
    return packed, counts


def segment_csr(packed_ranges: torch.Tensor, n_rows: int):
    """Inverse index of a packed range table (sl_segment_csr_host, a pure host routine): (row_ptr int64 (n_rows + 1), cols int32) CPU tensors;
    frame t is covered by ranges cols[row_ptr[t]:row_ptr[t + 1]], in table order."""
    r = torch.as_tensor(packed_ranges, dtype=torch.int64).reshape(-1, 2).contiguous()
    row_ptr = torch.empty(n_rows + 1, dtype=torch.int64)
    lib = L.lib()
    L.check(lib.sl_segment_csr_host(r.data_ptr(), r.shape[0], n_rows, row_ptr.data_ptr(), None, 0), "sl_segment_csr_host")
    cols = torch.empty(int(row_ptr[n_rows]), dtype=torch.int32)
    L.check(lib.sl_segment_csr_host(r.data_ptr(), r.shape[0], n_rows, row_ptr.data_ptr(), cols.data_ptr(), cols.numel()), "sl_segment_csr_host")
    return row_ptr, cols


def segment_mean_batch(x: torch.Tensor, ranges_dev: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[r] = mean(x[first_r:end_r]) for the int64 (R, 2) device table of packed-row ranges, one launch (sl_segment_mean_batch)."""
    L.require_gpu(x, "x"); L.require_gpu(ranges_dev, "ranges")
    R, H = int(ranges_dev.shape[0]), x.shape[1]
    y = torch.empty((R, H), device=x.device, dtype=x.dtype) if out is None else out
    L.check(L.lib().sl_segment_mean_batch(L.ptr(x), L.ptr(y), L.ptr(ranges_dev), R, x.shape[0], H, L.dtype_code(x.dtype), L.stream_ptr()),
            "sl_segment_mean_batch")
    return y


def segment_mean_bwd_batch(dy: torch.Tensor, ranges_dev: torch.Tensor, row_ptr_dev: torch.Tensor, cols_dev: torch.Tensor, n_rows: int,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx[t] = sum of dy[r] / len_r over the ranges covering frame t (sl_segment_mean_bwd_batch); every one of the n_rows rows is written."""
    L.require_gpu(dy, "dy")
    H = dy.shape[1]
    dx = torch.empty((n_rows, H), device=dy.device, dtype=dy.dtype) if out is None else out
    L.check(L.lib().sl_segment_mean_bwd_batch(L.ptr(dy), L.ptr(dx), L.ptr(ranges_dev), L.ptr(row_ptr_dev), L.ptr(cols_dev), int(ranges_dev.shape[0]), n_rows, H,
                                              L.dtype_code(dy.dtype), L.stream_ptr()), "sl_segment_mean_bwd_batch")
    return dx


def stack_rows_batch(x: torch.Tensor, seqlens: Sequence[int], factor: int, out: Optional[torch.Tensor] = None):
    """`stack` downsample of every utterance of a packed batch in one launch -> (dense (sum P_u, factor * H) rows, P list), P_u = T_u // factor."""
    L.require_gpu(x, "x")
    H = x.shape[1]
    P = [int(t) // factor for t in seqlens]
    desc, row, tok = [], 0, 0
    for p_, t in zip(P, seqlens):
        desc.append([p_, tok, row, 0])
        row += p_
        tok += int(t)
    y = torch.empty((row, factor * H), device=x.device, dtype=x.dtype) if out is None else out
    if row > 0:
        desc_t = L.h2d(desc, torch.int64, x.device)
        L.check(L.lib().sl_stack_rows_batch(L.ptr(x), L.ptr(y), desc_t.data_ptr(), len(P), max(P), H, factor, L.dtype_code(x.dtype), L.stream_ptr()),
                "sl_stack_rows_batch")
    return y, P


def stack_rows_bwd_batch(dy: torch.Tensor, seqlens: Sequence[int], factor: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of stack_rows_batch: (sum P_u, factor * H) -> (sum T_u, H), zeros in the T_u % factor cropped frames (one launch, every row written)."""
    H = dy.shape[1] // factor
    P = [int(t) // factor for t in seqlens]
    desc, row, tok = [], 0, 0
    for p_, t in zip(P, seqlens):
        desc.append([p_, int(t), row, tok])
        row += p_
        tok += int(t)
    dx = torch.empty((tok, H), device=dy.device, dtype=dy.dtype) if out is None else out
    src = dy if dy.numel() else torch.empty((1, factor * H), device=dy.device, dtype=dy.dtype)      # no stacked rows at all: nothing is read
    desc_t = L.h2d(desc, torch.int64, dy.device)
    L.check(L.lib().sl_stack_rows_bwd_batch(L.ptr(src), L.ptr(dx), desc_t.data_ptr(), len(P), max(int(t) for t in seqlens), H, factor,
                                            L.dtype_code(dy.dtype), L.stream_ptr()), "sl_stack_rows_bwd_batch")
    return dx


# -- CTC word segmentation of a packed ragged batch (ref:preprocess_data/utils.py:127-188 on the device) ---------------------------
def ctc_greedy(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ids[m] = the lowest column attaining max_v (x[m] . w[v] + bias[v]): the CTC head with its argmax fused (sl_ctc_greedy_batch, one launch,
    the logits are never written).  x (n_rows, H), w (V <= 64, H), bias (V) or None, one dtype; int32 ids."""
    L.require_gpu(x, "x"); L.require_gpu(w, "w")
    if bias is not None:
        L.require_gpu(bias, "bias")
    if w.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise L.SpeechLLMError("ctc_greedy: x, w and bias must share one dtype")
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1] or (bias is not None and bias.numel() != w.shape[0]):
        raise L.SpeechLLMError(f"ctc_greedy: x {tuple(x.shape)} against w {tuple(w.shape)}")
    ids = torch.empty(x.shape[0], dtype=torch.int32, device=x.device) if out is None else out
    L.check(L.lib().sl_ctc_greedy_batch(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(ids), x.shape[0], x.shape[1], w.shape[0], L.dtype_code(x.dtype),
                                        L.stream_ptr()), "sl_ctc_greedy_batch")
    return ids


def ctc_pool_ranges(ids: torch.Tensor, row_offsets_dev: torch.Tensor, blank_id: int = 0, delim_id: int = 4, pool_range: int = 4, raw: bool = False,
                    want_words: bool = False):
    """Greedy ids of a packed batch -> (ranges int64 (capacity, 2), counts int32 (n_utt)[, words int64 (capacity, 2), word counts int32]), all on
    the device (sl_ctc_pool_ranges_batch).  The utterances' records are contiguous and in utterance order: the first sum(counts) rows of `ranges`
    are the table; packed mode (raw=False) gives {first row, end row} records in packed frame rows that sl_segment_mean_batch / sl_hubert_forward_ds
    take as they are, raw mode the reference's utterance-relative list.  Nothing is copied to the host here."""
    L.require_gpu(ids, "ids"); L.require_gpu(row_offsets_dev, "row_offsets")
    if ids.dtype != torch.int32 or row_offsets_dev.dtype != torch.int64:
        raise L.SpeechLLMError("ctc_pool_ranges: ids must be int32 and row_offsets int64")
    lib = L.lib()
    n_utt, n_rows = int(row_offsets_dev.numel()) - 1, int(ids.numel())
    cap = int(lib.sl_ctc_pool_ranges_capacity(n_rows, n_utt))
    ranges = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=ids.device)
    counts = torch.empty(max(n_utt, 1), dtype=torch.int32, device=ids.device)
    words = wcounts = None
    wcap = 0
    if want_words:
        wcap = int(lib.sl_ctc_words_capacity(n_rows, n_utt))
        words = torch.empty((max(wcap, 1), 2), dtype=torch.int64, device=ids.device)
        wcounts = torch.empty(max(n_utt, 1), dtype=torch.int32, device=ids.device)
    L.check(lib.sl_ctc_pool_ranges_batch(L.ptr(ids), L.ptr(row_offsets_dev), n_utt, n_rows, int(blank_id), int(delim_id), int(pool_range),
                                         L.CTC_RANGES_RAW if raw else L.CTC_RANGES_PACKED, L.ptr(ranges), cap, L.ptr(counts), L.ptr(words), wcap,
                                         L.ptr(wcounts), L.stream_ptr()), "sl_ctc_pool_ranges_batch")
    return (ranges, counts[:n_utt], words, wcounts[:n_utt]) if want_words else (ranges, counts[:n_utt])
