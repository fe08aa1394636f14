"""GPU: sl_attn_fwd_past — causal head_dim 128 prefill attention whose keys come in two segments, the sequence's past out of its K/V cache
slot (e4m3 bytes or 16-bit elements) and its new rows out of the packed k / v — checked per element in the style of
tests/test_kernel_edges_gpu.py, with that suite's bounds (attn_bounds / check_attn) and nothing wider.

Reference: float64 softmax attention over concat(dq8(past bytes), new rows) on the CPU.  The 16-bit cache of the format-0 cases holds the
same dequantised values (every e4m3 value is exact in bf16 and fp16), so both formats share one reference.  Cache positions >= past and the
slots no sequence uses hold +-448 (the largest e4m3 magnitude; NaN bytes do not exist in the format), the packed rows keep the suite's poison
around them: a read beyond `past`, or beyond the new rows, shows.  Format 0 must also equal sl_attn_fwd over a cache the new rows were appended
to, bit for bit."""
import ctypes as C

import pytest
import torch

from conftest import pkg
from test_kernel_edges_gpu import BIG, DEV, FILL, attn_bounds, check_attn, gauss, operand  # noqa: F401
from edge_helpers import guarded, untouched

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")

F16, BF16 = torch.float16, torch.bfloat16
F8 = torch.float8_e4m3fn
D, MAX_CTX, SLACK = 128, 200, 3
PAIRS = [(0, 5), (1, 1), (63, 2), (64, 64), (65, 70), (130, 17)]      # (past, len): boundary past zero, inside a tile, on a tile edge; len below 16 rows
# one sequence in slot 1 of 3 for every pair, and a ragged batch of three in non-consecutive slots of 5
CASES = [([p], [1], 3) for p in PAIRS] + [([(63, 2), (65, 70), (130, 17)], [4, 0, 2], 5)]
POISON8 = torch.tensor([0x7E, 0xFE], dtype=torch.uint8).repeat(D // 2)      # +448, -448, ...


def q8(x):
    return x.detach().cpu().clamp(-448, 448).to(F8).view(torch.uint8)


def dq8(b):
    return b.detach().cpu().contiguous().view(F8).double()


def _case(pairs, slots, n_slots, nkv, cls):
    """-> (k8, v8 caches (n_slots, nkv, MAX_CTX, D) bytes with poison outside the pasts, knew64 / vnew64 packed rows with SLACK poisoned rows behind
    every sequence, cu_k)"""
    k8 = POISON8.repeat(n_slots, nkv, MAX_CTX, 1).clone()
    v8 = k8.clone()
    rows = sum(n for _, n in pairs) + SLACK * len(pairs)
    knew = torch.full((rows, nkv * D), 8.0, dtype=torch.float64)
    vnew = torch.full((rows, nkv * D), 448.0, dtype=torch.float64)
    cu_k = [0]
    for i, ((past, n), slot) in enumerate(zip(pairs, slots)):
        k8[slot, :, :past] = q8(gauss((nkv, past, D), 3000 + 10 * i).float())
        o = cu_k[-1]
        knew[o:o + n] = gauss((n, nkv * D), 3001 + 10 * i)
        if cls == "G":
            v8[slot, :, :past] = q8(gauss((nkv, past, D), 3002 + 10 * i).float())
            vnew[o:o + n] = gauss((n, nkv * D), 3003 + 10 * i)
        else:      # probe: key j carries a one in column j % D, so the output is the probability row itself
            vp = torch.zeros(nkv, past + n, D)
            j = torch.arange(past + n)
            vp[:, j, j % D] = 1.0
            v8[slot, :, :past] = q8(vp[:, :past])
            vnew[o:o + n] = vp[:, past:].transpose(0, 1).reshape(n, nkv * D).double()
        cu_k.append(o + n + SLACK)
    return k8, v8, knew, vnew, cu_k


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("nh,nkv", [(4, 1), (2, 2)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_attn_fwd_past_per_element_on_both_formats(dt, nh, nkv, case):
    pairs, slots, n_slots = CASES[case]
    scale = D ** -0.5
    nq_tot = sum(n for _, n in pairs)
    q, q64 = operand(gauss((nq_tot, nh * D), 3100 + case), dt)
    lens = [n for _, n in pairs]
    cu_q = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    klen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    past = torch.tensor([p for p, _ in pairs], dtype=torch.int32, device=DEV)
    row0 = torch.tensor([s * nkv * MAX_CTX for s in slots], dtype=torch.int32, device=DEV)
    for cls in ("P", "G"):
        k8, v8, knew64, vnew64, cu_k = _case(pairs, slots, n_slots, nkv, cls)
        k, k64 = operand(knew64, dt)
        v, v64 = operand(vnew64, dt, poison=448.0)
        cu_kd = torch.tensor(cu_k[:-1], dtype=torch.int32, device=DEV)
        kw = dict(q_strides=(q.stride(0), D), k_strides=(k.stride(0), D), v_strides=(v.stride(0), D), nseq=len(pairs), max_qlen=max(lens), n_heads=nh,
                  n_kv_heads=nkv, head_dim=D, scale=scale)
        outs = {}
        for fmt in (L.KV_FP8_E4M3, L.KV_MODEL_DTYPE):
            kc = k8.to(DEV) if fmt == L.KV_FP8_E4M3 else dq8(k8).float().to(dt).to(DEV)
            vc = v8.to(DEV) if fmt == L.KV_FP8_E4M3 else dq8(v8).float().to(dt).to(DEV)
            buf, out = guarded(nq_tot, nh * D, dt)
            ops.attn_fwd_past(q, k, v, out, cu_q, cu_kd, klen, kc, vc, past, row0, o_strides=(out.stride(0), D), max_ctx=MAX_CTX, kv_format=fmt, **kw)
            assert untouched(buf, nq_tot, nh * D)
            outs[fmt] = out
            q0 = 0
            for i, ((p_, n), slot) in enumerate(zip(pairs, slots)):
                kk = torch.cat([dq8(k8[slot, :, :p_]), k64[cu_k[i]:cu_k[i] + n].view(n, nkv, D).transpose(0, 1)], 1)
                vv = torch.cat([dq8(v8[slot, :, :p_]), v64[cu_k[i]:cu_k[i] + n].view(n, nkv, D).transpose(0, 1)], 1)
                vis = torch.arange(p_ + n)[None, :] <= torch.arange(n)[:, None] + p_
                ref, tol, zero = attn_bounds(q64[q0:q0 + n].view(n, nh, D).transpose(0, 1), kk, vv, vis, scale, dt)
                check_attn(out[q0:q0 + n], ref, tol, zero, dt, f"{cls} format {fmt} sequence {i} (past {p_}, {n} new)")
                q0 += n
        # format 0 against sl_attn_fwd over the cache with the new rows appended at [past, past + len): the same bits
        kc = dq8(k8).float().to(dt)
        vc = dq8(v8).float().to(dt)
        for i, ((p_, n), slot) in enumerate(zip(pairs, slots)):
            kc[slot, :, p_:p_ + n] = k64[cu_k[i]:cu_k[i] + n].view(n, nkv, D).transpose(0, 1).float().to(dt)
            vc[slot, :, p_:p_ + n] = v64[cu_k[i]:cu_k[i] + n].view(n, nkv, D).transpose(0, 1).float().to(dt)
        kc, vc = kc.to(DEV), vc.to(DEV)
        buf, want = guarded(nq_tot, nh * D, dt)
        ops.attn_fwd(q, kc, vc, want, cu_q, row0, past + klen, q_strides=(q.stride(0), D), k_strides=(D, MAX_CTX * D), v_strides=(D, MAX_CTX * D),
                     o_strides=(want.stride(0), D), nseq=len(pairs), max_qlen=max(lens), n_heads=nh, n_kv_heads=nkv, head_dim=D, causal=True, scale=scale)
        got = outs[L.KV_MODEL_DTYPE]
        assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), f"{cls}: format 0 differs from sl_attn_fwd over the appended cache"


def test_attn_fwd_past_refusals_launch_nothing():
    nh, nkv, n = 2, 1, 4
    q = torch.zeros((n, nh * D), device=DEV, dtype=BF16)
    k = torch.zeros((n, nkv * D), device=DEV, dtype=BF16)
    out = torch.full((n, nh * D), FILL, device=DEV, dtype=BF16)
    kc = torch.zeros((1, nkv, MAX_CTX, D), device=DEV, dtype=torch.uint8)
    cu = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    one = torch.tensor([n], dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(dtype=L.SL_BF16, head_dim=D, causal=1, fmt=L.KV_FP8_E4M3):
        a = L.AttnArgs()
        a.q, a.q_row_stride, a.q_head_stride = q.data_ptr(), nh * D, D
        a.k, a.k_row_stride, a.k_head_stride = k.data_ptr(), nkv * D, D
        a.v, a.v_row_stride, a.v_head_stride = k.data_ptr(), nkv * D, D
        a.out, a.o_row_stride, a.o_head_stride = out.data_ptr(), nh * D, D
        a.cu_q, a.cu_k, a.klen = cu.data_ptr(), zero.data_ptr(), one.data_ptr()
        a.nseq, a.max_qlen, a.n_heads, a.n_kv_heads, a.head_dim, a.causal, a.dtype, a.scale = 1, n, nh, nkv, head_dim, causal, dtype, 1.0
        return L.lib().sl_attn_fwd_past(C.byref(a), kc.data_ptr(), kc.data_ptr(), zero.data_ptr(), zero.data_ptr(), MAX_CTX, fmt, L.stream_ptr())

    UNSUPPORTED, ARG = -3, -1
    assert call(dtype=L.SL_F32) == UNSUPPORTED
    assert call(head_dim=64) == UNSUPPORTED
    assert call(causal=0) == UNSUPPORTED
    assert call(fmt=2) == ARG and b"format" in L.lib().sl_last_error()
    assert call(fmt=-1) == ARG
    torch.cuda.synchronize()
    assert bool((out == FILL).all()), "a refused call wrote the output"
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == FILL).any())
