"""GPU: the kernels of teacher-forced scoring, per element — the target logit beside the lm_head epilogue's three planes
(sl_gemm_top1_lse_tgt), the two log-probability kernels (sl_score_finalize over the planes, sl_score_rows over fp32 logits) against the
fp64 restatement (tests/token_scores_ref.py) within the bounds counted there, and the per-sequence sums (sl_score_segment_sums).

The bound of a GIVEN token's log-probability, from token_scores_ref's own functions: bound_row(x, token) counts the rounding of
x[token] - m, of the final subtraction and of the row-scan log-sum-exp — that is sl_score_rows.  sl_score_finalize forms (tgt - m) -
logf(total) with total summed in the order bound_partial counts; its error is below bound_row's target terms plus bound_partial, so
bound_row + bound_partial is used (the row-scan chain in it is slack, never a missing term)."""
import numpy as np
import pytest
import torch

from conftest import pkg

import token_scores_ref as tsr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = pkg("_lib")
ops = pkg("ops")

GUARD = 12345.0
DT = [torch.float32, torch.bfloat16, torch.float16]
IGNORED = [-1, -100, None, 2 ** 30]          # None: the vocabulary size itself (the first column past the end)


def rnd(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _guarded(n, dtype, fill):
    """n elements with 64 guard words on either side -> (whole buffer, the view)"""
    buf = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
    return buf, buf[64:64 + n]


def _guards_intact(buf, n, fill):
    return bool((buf[:64] == fill).all()) and bool((buf[64 + n:] == fill).all())


# ------------------------------------------------------------------------------------------------ the target logit beside the planes
def _targets(M, N, inf_col):
    """row r -> its wanted column: the special columns in turn, every fifth row an ignored one"""
    partial = N - 1 - (N % 64) // 2 if N % 64 else N - 1                 # a column of the partial last group (N % 64 != 0)
    special = [0, N - 1, 63, min(64, N - 1), partial, inf_col]
    gen = np.random.default_rng(M * 1000 + N)
    cols = []
    for r in range(M):
        if r % 5 == 4:
            ig = IGNORED[(r // 5) % 4]
            cols.append(N if ig is None else ig)
        elif r % 5 == 3:
            cols.append(int(gen.integers(0, N)))
        else:
            cols.append(special[(r // 5 * 3 + r % 5) % len(special)])
    return cols


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M", [65, 77, 300])
@pytest.mark.parametrize("N,K", [(1000, 64), (200, 192), (64, 64)])
def test_target_logit_is_the_stored_logit_and_the_planes_do_not_move(dt, M, N, K):
    """sl_gemm_top1_lse_tgt: the three planes bit for bit those of sl_gemm_top1_lse; tgt_val[row] bit-equal to the fp32 logit the same product
    stores at (row, tgt_col[row]) with and without bias; rows whose column is -1, -100, N or 2^30 keep the guard value; guards intact."""
    A, W = rnd(M, K, seed=21 + M), rnd(N, K, seed=22 + N, std=2.0 * K ** -0.5)
    nan_row = M // 3
    A[nan_row] = float("nan")                                       # one all-NaN row: every product is NaN
    bias = rnd(N, seed=23)
    inf_col = 70 if N > 192 else 5
    bias[inf_col] = float("-inf")
    cols = _targets(M, N, inf_col)
    if cols[nan_row] < 0 or cols[nan_row] >= N:
        cols[nan_row] = 1                                           # the NaN row asks for a real column
    for want in (0, N - 1, 63, min(64, N - 1), inf_col):
        assert want in cols
    Ad, Wd = A.to(DEV, dt), W.to(DEV, dt)
    tc = torch.tensor(cols, dtype=torch.int32, device=DEV)
    ng = (N + 63) // 64
    valid = torch.tensor([0 <= c < N for c in cols])
    for b in (None, bias.to(DEV, dt)):
        logits = ops.gemm(Ad, Wd, bias=b, out_f32=True)
        val0, idx0, sum0 = ops.gemm_top1_lse(Ad, Wd, bias=b)
        bufs = [_guarded(ng * M, torch.float32, GUARD), _guarded(ng * M, torch.int32, 12345), _guarded(ng * M, torch.float32, GUARD)]
        tbuf, tv = _guarded(M, torch.float32, GUARD)
        cbuf, tcg = _guarded(M, torch.int32, 7)
        tcg.copy_(tc)
        val, idx, ssum, got = ops.gemm_top1_lse_tgt(Ad, Wd, tcg, bias=b, out=tuple(v.view(ng, M) for _, v in bufs), tgt_val=tv)
        torch.cuda.synchronize()
        assert _guards_intact(bufs[0][0], ng * M, GUARD) and _guards_intact(bufs[1][0], ng * M, 12345) and _guards_intact(bufs[2][0], ng * M, GUARD)
        assert _guards_intact(tbuf, M, GUARD) and _guards_intact(cbuf, M, 7) and torch.equal(tcg, tc)
        assert torch.equal(val.view(torch.int32), val0.view(torch.int32)) and torch.equal(idx, idx0)
        assert torch.equal(ssum.view(torch.int32), sum0.view(torch.int32))
        got, lg = got.cpu(), logits.cpu()
        assert bool((got[~valid] == GUARD).all())                   # nobody wrote them
        rows = torch.tensor([r for r in range(M) if valid[r] and r != nan_row])
        want = lg[rows, torch.tensor(cols)[rows]]
        same = got[rows].view(torch.int32) == want.view(torch.int32)
        assert bool(same.all()), [(int(rows[i]), cols[int(rows[i])], float(got[rows[i]]), float(want[i])) for i in torch.nonzero(~same)[:4, 0]]
        assert bool(torch.isnan(got[nan_row])) and bool(torch.isnan(lg[nan_row, cols[nan_row]]))
        if b is not None:
            hit = [r for r in range(M) if cols[r] == inf_col and r != nan_row]
            assert hit and all(float(got[r]) == float("-inf") for r in hit)


# ------------------------------------------------------------------------------------------------ the two log-probability kernels
def _score_case(V, B=70):
    """(logits, labels): the rows of the select-kernel tests of DESIGN 3.5 plus labels that are NOT the maximum"""
    logits = rnd(B, V, seed=V + 1) * 3.0
    logits[:, 5] = float("-inf")
    logits[3, 7] = float("nan")
    logits[4] = float("-inf")                                       # no finite maximum
    if V > 128:
        logits[5, 64:128] = float("-inf")                          # a dead group
    logits[6] += 100.0
    logits[8] = float("nan")                                        # an all-NaN row under an ignored label
    gen = np.random.default_rng(V)
    labels = [int(v) for v in gen.integers(0, V, size=B)]
    labels[0], labels[1], labels[2] = 0, V - 1, 5                   # first, last, a -inf column
    labels[3] = 7                                                   # the NaN element: counts as -inf
    labels[7] = int(torch.where(torch.isnan(logits[7]), torch.full_like(logits[7], float("-inf")), logits[7]).argmax())      # the maximum itself
    for j, r in enumerate((8, 20, 33, 69)):
        ig = IGNORED[j]
        labels[r] = V if ig is None else ig
    return logits, labels


def _planes(logits):
    """the three planes of the fused lm_head, made on the host in fp64 -> fp32 (one more rounding per group sum than the device's)"""
    B, V = logits.shape
    ng = (V + 63) // 64
    clean = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits)
    grp = torch.cat([clean, torch.full((B, ng * 64 - V), float("-inf"))], 1).view(B, ng, 64)
    gmax = grp.max(dim=2).values
    first = (grp == gmax[:, :, None]).float().argmax(dim=2) + torch.arange(ng)[None, :] * 64
    first[torch.isinf(gmax) & (gmax < 0)] = 0x7fffffff
    gsum = torch.exp(grp.double() - torch.where(torch.isinf(gmax), torch.zeros_like(gmax), gmax).double()[:, :, None]).sum(dim=2)
    gsum[torch.isinf(gmax)] = 0.0
    return gmax.T.contiguous().to(DEV), first.T.contiguous().to(torch.int32).to(DEV), gsum.T.contiguous().float().to(DEV)


def _greedy_choice(ld):
    B = ld.shape[0]
    s = dict(unfinished=torch.ones(B, dtype=torch.int32, device=DEV), ctx=torch.zeros(B, dtype=torch.int32, device=DEV),
             gen=torch.zeros(B, dtype=torch.int32, device=DEV), fin=torch.zeros(B, dtype=torch.int32, device=DEV),
             nxt=torch.zeros(B, dtype=torch.int32, device=DEV), out=torch.full((B, 1), -1, dtype=torch.int32, device=DEV))
    ops.greedy_select(ld, [], 0, False, s["unfinished"], s["ctx"], s["gen"], s["fin"], s["nxt"], s["out"])
    return s["nxt"].cpu()


_REF = {}


def _reference(V):
    """computed once per V and shared: the case, the fp64 restatement and the per-row bounds"""
    if V not in _REF:
        logits, labels = _score_case(V)
        B = logits.shape[0]
        ok = [0 <= l < V for l in labels]
        ref = tsr.transition_logprobs(logits, torch.tensor([l if o else 0 for l, o in zip(labels, ok)]))
        b_row, b_fin = [0.0] * B, [0.0] * B
        for r in range(B):
            if ok[r] and np.isfinite(float(ref[r])):
                b_row[r] = tsr.bound_row(logits[r].numpy(), labels[r])
                b_fin[r] = b_row[r] + tsr.bound_partial(logits[r].numpy()) + tsr.U * 1.01      # + the host-made third plane's rounding
        _REF[V] = (logits, labels, ok, ref, b_row, b_fin)
    return _REF[V]


@pytest.mark.parametrize("V", [1000, 777, 64, 4100])
def test_finalize_and_rows_agree_with_the_fp64_restatement(V):
    """V = 777: the scalar row scan and a last group of 9; 4 100: more than one 16-byte group per thread, 65 groups (three per stripe); 64: one
    group.  70 rows: three blocks of the finalize kernel, the last with 6 rows.  Ignored labels give exactly 0.0 — also where tgt_val holds
    NaN and where the whole logits row is NaN; top1 is sl_greedy_select's choice; a -inf / NaN target gives -inf; a row without a finite
    maximum a non-finite value."""
    logits, labels, ok, ref, b_row, b_fin = _reference(V)
    B = logits.shape[0]
    ld = logits.to(DEV)
    lab = torch.tensor(labels, dtype=torch.int32, device=DEV)
    val, idx, ssum = _planes(logits)
    clean = torch.where(torch.isnan(logits), torch.full_like(logits, float("-inf")), logits)
    tgt = torch.tensor([float(clean[r, labels[r]]) if ok[r] else float("nan") for r in range(B)], dtype=torch.float32, device=DEV)      # poison under ignored labels
    choice = _greedy_choice(ld)
    lbuf, lgv = _guarded(B * V, torch.float32, float("nan"))        # NaN beyond the last row: logits[B - 1][V] is never to be read
    lgv.copy_(ld.view(-1))
    outs = {}
    for kind in ("rows", "finalize"):
        pbuf, lp = _guarded(B, torch.float32, GUARD)
        tbuf, t1 = _guarded(B, torch.int32, 777)
        if kind == "rows":
            ops.score_rows(lgv.view(B, V), lab, logprob=lp, top1=t1)
        else:
            ops.score_finalize(val, idx, ssum, tgt, lab, V, logprob=lp, top1=t1)
        torch.cuda.synchronize()
        assert _guards_intact(pbuf, B, GUARD) and _guards_intact(tbuf, B, 777)
        outs[kind] = (lp.cpu(), t1.cpu())
    worst = {"rows": 0.0, "finalize": 0.0}
    for kind, (lp, t1) in outs.items():
        assert torch.equal(t1, choice), kind
        for r in range(B):
            got = float(lp[r])
            if not ok[r]:
                assert got == 0.0, (kind, r, got)
            elif r == 4:
                assert not np.isfinite(got), (kind, r, got)
            elif not np.isfinite(float(ref[r])):
                assert got == float("-inf"), (kind, r, got)
            else:
                bound = b_row[r] if kind == "rows" else b_fin[r]
                assert abs(got - float(ref[r])) <= bound, (kind, r, got, float(ref[r]), bound)
                worst[kind] = max(worst[kind], abs(got - float(ref[r])) / bound)
    print(f"V={V}: worst err / bound rows {worst['rows']:.3f} finalize {worst['finalize']:.3f}")


def test_rows_kernel_takes_a_pitch():
    """logits rows of pitch ld > V (V = 777: rows that are not 16-byte aligned take the scalar scan)"""
    logits, labels, ok, ref, b_row, _ = _reference(777)
    B, V, ld_ = logits.shape[0], 777, 801
    wide = torch.full((B, ld_), float("nan"), device=DEV)
    wide[:, :V] = logits.to(DEV)
    lab = torch.tensor(labels, dtype=torch.int32, device=DEV)
    lp, t1 = ops.score_rows(wide[:, :V], lab)
    lp0, t10 = ops.score_rows(logits.to(DEV), lab)
    assert torch.equal(t1, t10)
    for r in range(B):
        if ok[r] and np.isfinite(float(ref[r])) and r != 4:
            assert abs(float(lp[r]) - float(ref[r])) <= b_row[r]
        elif not ok[r]:
            assert float(lp[r]) == 0.0


# ------------------------------------------------------------------------------------------------ per-sequence sums
def test_segment_sums_against_fp64_and_exact_counts():
    """sequences of 1, 17, 5 (all ignored), 300 (more rows than the block has threads) and 77 rows; the sums within n x the per-token bound of
    the fp64 sums, the counters exact"""
    V = 777
    lens = [1, 17, 5, 300, 77]
    R = sum(lens)
    logits = rnd(R, V, seed=5) * 2.0
    gen = np.random.default_rng(6)
    labels = [int(v) for v in gen.integers(0, V, size=R)]
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    for r in range(offs[2], offs[3]):
        labels[r] = -100
    for r in (offs[1] + 3, offs[3], offs[3] + 255, offs[3] + 256, offs[4] - 1, R - 1):      # ignored rows inside, at the edges and at the thread wrap
        labels[r] = -100
    best = logits.argmax(dim=1)
    for r in range(0, R, 3):
        if labels[r] >= 0:
            labels[r] = int(best[r])                              # a third of the counted rows ARE the top-1
    lab = torch.tensor(labels, dtype=torch.int32, device=DEV)
    lp, t1 = ops.score_rows(logits.to(DEV), lab)
    obuf = [_guarded(len(lens), torch.float32, GUARD), _guarded(len(lens), torch.int32, 99), _guarded(len(lens), torch.int32, 99)]
    ssum, cnt, hit = ops.score_segment_sums(lp, lab, t1, torch.tensor(offs, dtype=torch.int32, device=DEV), V, out=tuple(v for _, v in obuf))
    torch.cuda.synchronize()
    assert _guards_intact(obuf[0][0], len(lens), GUARD) and _guards_intact(obuf[1][0], len(lens), 99) and _guards_intact(obuf[2][0], len(lens), 99)
    ok = [l >= 0 for l in labels]
    ref = tsr.transition_logprobs(logits, torch.tensor([max(l, 0) for l in labels]))
    t1c = t1.cpu()
    for s, n in enumerate(lens):
        rows = [r for r in range(offs[s], offs[s + 1]) if ok[r]]
        assert int(cnt[s]) == len(rows)
        assert int(hit[s]) == sum(int(t1c[r]) == labels[r] for r in rows)
        want = float(sum(float(ref[r]) for r in rows))
        per_token = max([tsr.bound_row(logits[r].numpy(), labels[r]) for r in rows], default=0.0)
        assert abs(float(ssum[s]) - want) <= len(rows) * per_token, (s, float(ssum[s]), want, len(rows) * per_token)
    assert float(ssum[2]) == 0.0 and int(cnt[2]) == 0 and int(hit[2]) == 0
    assert int(cnt[0]) == 1 and int(hit[0]) == 1


# ------------------------------------------------------------------------------------------------ the two paths on the same rows
@pytest.mark.parametrize("dt", DT)
def test_fused_and_rows_paths_agree_on_the_same_rows(dt):
    """300 x 1000 x 64: sl_gemm_top1_lse_tgt + sl_score_finalize against fp32 logits of the same product + sl_score_rows, within twice the
    per-token bound; the top-1 columns equal"""
    M, N, K = 300, 1000, 64
    A, W = rnd(M, K, seed=41), rnd(N, K, seed=42, std=2.0 * K ** -0.5)
    bias = rnd(N, seed=43)
    bias[70] = float("-inf")
    gen = np.random.default_rng(44)
    labels = [int(v) for v in gen.integers(0, N, size=M)]
    labels[10], labels[11], labels[299] = -100, N, -1
    lab = torch.tensor(labels, dtype=torch.int32, device=DEV)
    Ad, Wd, bd = A.to(DEV, dt), W.to(DEV, dt), bias.to(DEV, dt)
    logits = ops.gemm(Ad, Wd, bias=bd, out_f32=True)
    lp_r, t1_r = ops.score_rows(logits, lab)
    tv = torch.full((M,), float("nan"), device=DEV)
    val, idx, ssum, tv = ops.gemm_top1_lse_tgt(Ad, Wd, lab, bias=bd, tgt_val=tv)
    lp_f, t1_f = ops.score_finalize(val, idx, ssum, tv, lab, N)
    assert torch.equal(t1_r, t1_f)
    lg = logits.cpu()
    worst = 0.0
    for r in range(M):
        if not 0 <= labels[r] < N:
            assert float(lp_r[r]) == 0.0 and float(lp_f[r]) == 0.0
            continue
        if labels[r] == 70:
            assert float(lp_r[r]) == float("-inf") and float(lp_f[r]) == float("-inf")
            continue
        x = lg[r].numpy()
        bound = 2 * (tsr.bound_row(x, labels[r]) + tsr.bound_partial(x))
        d = abs(float(lp_r[r]) - float(lp_f[r]))
        assert d <= bound, (r, float(lp_r[r]), float(lp_f[r]), bound)
        worst = max(worst, d / bound)
    print(f"{dt}: worst |fused - rows| / bound {worst:.3f}")
