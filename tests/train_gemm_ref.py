"""The GEMM side of the backward pass restated in plain torch, fp64, on the CPU (a helper module of the edge suite's fourth chapter, not a
conftest; it imports neither a GPU nor the library — `keep_mask` alone loads ops.py for the one host restatement of the dropout hash).

Every `*_ref` takes the STORED (already rounded) operands in fp64 and returns a namespace of fp64 results with per-element bounds `tol_*`.
The bounds are the suite's ("Edge suite"): u = half an ulp of the stored type, E24 = 2^-24,

    product         2u |ref| + K E24 mag + E24, mag = |A|^T |W| + |b| + |R| taken term by term (any order, any K run, any atomic)
    rounding to T   u |v| for every intermediate value the epilogue rounds to the storage type before it goes on (gemm_internal.h round_as)
    multiply, add   E24 |result| each
    transcendental  train_ops_ref's TRANS (1 + |.|) and TINY through its gelu_bwd_ref / silu_mul_bwd_ref, which count their own operations
    column sums     n E24 sum |term| for n terms in any order

and an error e of an intermediate value reaches the result through the derivative of what follows (|gelu'| <= 1.13, |d dgate / d d| =
|up sg br|, ...).  No constant is a measured number.  `*_sim` restate a route in fp32 torch in the kernels' order; the planted defects of
tests/test_train_gemm_ref_cpu.py are built on them.  The case tables at the end are shared by tests/test_train_gemm_edges_gpu.py, which
runs them, and by the CPU self-check, which asks the dispatcher's dry run (SL_GEMM_LOG=2) for the plan of every one of them."""
import importlib
from types import SimpleNamespace

import torch

import train_ops_ref as R
from train_ops_ref import BF16, E24, F32, U, gelu_bwd_ref, interleave, silu_mul_bwd_ref  # noqa: F401 (interleave: used by the GPU file)

NONE, GELU = 0, 1
DROPOUT, GELU_BWD, SILU_BWD = 1, 2, 3
BK = 64               # token rows of one slab of the token-major kernels
G_MAX_K = 1024        # class G: longest reduction (one missing term stays >= 16 x the accumulation term, the first chapter's rule)


def class_g(s):
    """does the GPU file run class G on this spec?  (longer reductions are class E and Z only)"""
    return s["K"] <= G_MAX_K


def keep_mask(rows, cols, drop_ld, p, seed):
    """bool (rows, cols): ops.dropout_keep_at on the element index row * drop_ld + col, which is what the epilogues hash"""
    ops = importlib.import_module("llm-speech-summarization_amd.ops")
    idx = torch.arange(rows, dtype=torch.int64)[:, None] * drop_ld + torch.arange(cols, dtype=torch.int64)[None]
    return ops.dropout_keep_at(idx, p, seed)


def rnd(x, dt):
    return R.rnd(x, dt)


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradient: dW (No, Ni) = dW0 + dY^T X, db = db0 + colsum(dY); dY (T, No), X (T, Ni)
# ------------------------------------------------------------------------------------------------------------------------------
def wgrad_ref(dy, x, dw0, db0=None):
    T = dy.shape[0]
    dw = dw0 + dy.T @ x
    mag = dy.abs().T @ x.abs() + dw0.abs()
    r = SimpleNamespace(dw=dw, tol_dw=2 * E24 * dw.abs() + T * E24 * mag + E24)
    if db0 is not None:
        r.db = db0 + dy.sum(0)
        r.tol_db = E24 * T * dy.abs().sum(0) + E24 * r.db.abs()
    return r


def windows(x, rows, k, s):
    """implicit-GEMM conv windows: row t is x[t s : t s + k] flattened, (rows, k C)"""
    return torch.stack([x[t * s:t * s + k].reshape(-1) for t in range(rows)])


def runs_of(T, krun):
    """[t0, t1) token ranges of the K runs of `krun` slabs"""
    return [(t0, min(T, t0 + krun * BK)) for t0 in range(0, T, krun * BK)]


def wgrad_sim(dy, x, dw0, db0, krun, tiles_n=1, rng=None, defect=None):
    """fp32 restatement of the token-major route: per K run an fp32 accumulation slab by slab, the runs summed in run order on top of dW0;
    the rider from one fp32 sum per run and 64-row wave, added in a random order.  `defect` plants one of the CPU file's defects."""
    T, No = dy.shape
    dyf, xf = dy.float(), x.float()
    parts, adds = [], []
    for (t0, t1) in runs_of(T, krun):
        acc = torch.zeros(No, x.shape[1])
        accb = torch.zeros(No)
        for k0 in range(t0, t1, BK):
            a, b = dyf[k0:min(k0 + BK, t1)], xf[k0:min(k0 + BK, t1)]
            if defect == "drop_last_row" and k0 + BK >= T:
                a, b = a[:-1], b[:-1]
            rep = 2 if (defect == "first_slab_twice" and k0 == t0 and t0 > 0) else 1
            for _ in range(rep):
                acc = acc + a.T @ b
            accb = accb + a.sum(0)
        parts.append(acc)
        adds.append(accb)
    dw = dw0.float().clone()
    for p_ in parts:
        dw = dw + p_
    db = None
    if db0 is not None:
        pieces = []
        for accb in adds:
            for w0 in range(0, No, 64):
                piece = torch.zeros(No)
                piece[w0:w0 + 64] = accb[w0:w0 + 64]
                if defect == "rider_quarter" and w0 == 0:
                    piece[16:32] = 0.0            # one 16-row fragment of the first wave missing
                pieces += [piece] * (tiles_n if defect == "rider_every_column_tile" else 1)
        order = torch.randperm(len(pieces), generator=rng).tolist() if rng is not None else range(len(pieces))
        db = db0.float().clone()
        for i in order:
            db = db + pieces[i]
        db = db.double()
    return dw.double(), db


# ------------------------------------------------------------------------------------------------------------------------------
# plain product and the epilogue riders: y = A W^T (M, N), K terms
# ------------------------------------------------------------------------------------------------------------------------------
def product(a, w, bias=None):
    """a (M, K), w (N, K) -> pre = a w^T + b, and e_pre: the bound on the fp32 value the epilogue starts from"""
    K = a.shape[1]
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias
    pre = a @ w.T + b
    mag = a.abs() @ w.abs().T + b.abs()
    return SimpleNamespace(pre=pre, mag=mag, e_pre=K * E24 * mag + E24, K=K)


def plain_ref(a, w, dt, bias=None, res=None, out_f32=False):
    p = product(a, w, bias)
    r0 = torch.zeros_like(p.pre) if res is None else res
    ref = p.pre + r0
    u = U[F32] if out_f32 else U[dt]
    return SimpleNamespace(c=ref, tol_c=2 * u * ref.abs() + p.K * E24 * (p.mag + r0.abs()) + E24)


def aux_gelu_ref(a, w, bias, dt):
    """aux_out = pre (rounded to T), C = gelu(pre as computed in fp32): check_gauss's GELU bound"""
    p = product(a, w, bias)
    u = U[dt]
    c = 0.5 * p.pre * (1.0 + torch.erf(p.pre / 2.0 ** 0.5))
    return SimpleNamespace(aux=p.pre, tol_aux=2 * u * p.pre.abs() + p.e_pre, c=c,
                           tol_c=2 * u * c.abs() + 1.13 * p.K * E24 * p.mag + 2e-6 * (1 + p.pre.abs()) + E24)


def dropout_ref(a, w, bias, res, keep, p_drop, dt):
    """C = R + keep round_T(pre) / (1 - p).  Where kept: the product's bound times the scale (2u |pre| covers round_T (u) and leaves u for the
    store of a value without residual), the scale multiply and the residual add (E24 |.| each), the store (2u |ref|).  Where dropped: R."""
    p = product(a, w, bias)
    scale = 1.0 / (1.0 - p_drop)
    r0 = torch.zeros_like(p.pre) if res is None else res
    kept = keep.double()
    ref = r0 + kept * scale * p.pre
    u = U[dt]
    tol = kept * (scale * (2 * u * p.pre.abs() + p.e_pre) + 2 * E24 * (scale * p.pre.abs() + ref.abs())) + 2 * u * ref.abs() * (r0 != 0).double() * kept
    return SimpleNamespace(c=ref, tol_c=tol, pre=p.pre)


def gelu_bwd_post_ref(dyv, w, pre, keep, p_drop, dt):
    """C = gelu'(pre) dropout(dY W): d = round_T(dY W), with dropout round_T(d) / (1 - p) rounded once more; then train_ops_ref.gelu_bwd_ref"""
    p = product(dyv, w)
    u = U[dt]
    scale = 1.0 / (1.0 - p_drop) if p_drop > 0 else 1.0
    kept = torch.ones_like(p.pre) if keep is None else keep.double()
    d = kept * scale * p.pre
    e_d = kept * (scale * (u * p.pre.abs() + p.e_pre) + ((u + E24) * d.abs() if p_drop > 0 else 0.0))
    g = gelu_bwd_ref(d, pre, dt)
    return SimpleNamespace(c=g.dx, tol_c=g.tol_dx + 1.13 * e_d, d=d)


def silu_bwd_post_ref(dxv, w, g, up, dt):
    """(dgate, dup) of silu_mul_bwd on d = round_T(dX W^T): train_ops_ref.silu_mul_bwd_ref + the error of d through each output's derivative"""
    p = product(dxv, w)
    e_d = U[dt] * p.pre.abs() + p.e_pre
    r = silu_mul_bwd_ref(g, up, p.pre, dt)
    sg = torch.sigmoid(g)
    br = 1.0 + g * (1.0 - sg)
    return SimpleNamespace(dgate=r.dgate, dup=r.dup, tol_dgate=r.tol_dgate + e_d * (up * sg * br).abs(), tol_dup=r.tol_dup + e_d * (g * sg).abs())


def colsum_ref(c_stored, db0):
    """db = db0 + column sums of the STORED C (fp64 of the rounded values): M terms in any order"""
    M = c_stored.shape[0]
    db = db0 + c_stored.sum(0)
    return SimpleNamespace(db=db, tol_db=E24 * M * c_stored.abs().sum(0))


def product_sim(a, w, bias=None, nruns=1):
    """fp32 product in `nruns` K runs summed in run order, + bias"""
    a, w = a.float(), w.float()
    K = a.shape[1]
    step = (K + nruns - 1) // nruns
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, K, step):
        acc = acc + a[:, k0:k0 + step] @ w[:, k0:k0 + step].T
    return acc if bias is None else acc + bias.float()


def rt(x, dt):
    """fp32 -> stored type -> fp32 (gemm_internal.h round_as)"""
    return x.to(dt).float()


def dropout_sim(a, w, bias, res, keep, p_drop, dt):
    scale = torch.tensor(1.0 / (1.0 - p_drop), dtype=F32) if p_drop != 0.5 else torch.tensor(2.0)
    v = torch.where(keep, rt(product_sim(a, w, bias), dt) * scale, torch.zeros(()))
    if res is not None:
        v = v + res.float()
    return rt(v, dt).double()


def gelu_bwd_post_sim(dyv, w, pre, keep, p_drop, dt, on_rounded_c=False):
    v = rt(product_sim(dyv, w), dt)
    if p_drop > 0:
        v = rt(torch.where(keep, v * torch.tensor(1.0 / (1.0 - p_drop), dtype=F32), torch.zeros(())), dt)
    arg = v if on_rounded_c else pre.float()          # the defect: gelu' of the rounded product instead of the saved pre-activation
    return rt(v * R.gelu_grad32(arg), dt).double()


def silu_bwd_post_sim(dxv, w, g, up, dt, swap_block=None):
    d = rt(product_sim(dxv, w), dt)
    g, up = g.float().clone(), up.float().clone()
    if swap_block is not None:                         # the defect: gate and up exchanged in one 16-column block
        c0 = 16 * swap_block
        g[:, c0:c0 + 16], up[:, c0:c0 + 16] = up[:, c0:c0 + 16].clone(), g[:, c0:c0 + 16].clone()
    sg = 1.0 / (1.0 + torch.exp(-g))
    return rt(d * up * sg * (1.0 + g * (1.0 - sg)), dt).double(), rt(d * g * sg, dt).double()


# ------------------------------------------------------------------------------------------------------------------------------
# case tables.  A spec holds everything of a call that the dispatcher's plan depends on; `plan` is the SLPLAN line of its dry run
# (fam form grid S krun close), pinned by tests/test_train_gemm_ref_cpu.py.  Leading dimensions are the edge suite's: operand() and guarded()
# give ld_of(cols).
# ------------------------------------------------------------------------------------------------------------------------------
def ld_of(cols):
    return (cols + 7) // 8 * 8 + 16


def spec(sid, dt, M, N, K, plan, **kw):
    d = dict(id=sid, dt=dt, M=M, N=N, K=K, plan=plan, env={})
    d.update(kw)
    return d


def plan_str(fam, form, grid, S=1, krun=0, close="none"):
    return f"fam={fam} form={form} grid={grid} S={S} krun={krun} close={close}"


def slabs(K):
    return (K + BK - 1) // BK


def tt_spec(sid, M, N, K, form, grid, S=1, krun=None, wide=False, ws=False, colsum=False, env=None, dt=BF16):
    """token-major weight gradient: dY (K, M) with lda, X (K, N) with ldw, fp32 dW as residual and output"""
    krun = slabs(K) if krun is None else krun
    fam = "tt" if form in ("two_stage", "ring", "batched") else form
    return spec(sid, dt, M, N, K, plan_str(fam, form if fam == "tt" else "none", grid, S, krun if fam == "tt" else 0, "reduce" if S > 1 else "none"),
                ta=1, tw=1, lda=3 * M if wide else ld_of(M), ldw=ld_of(N), ldc=ld_of(N), ldr=ld_of(N), out_f32=1, res=1, res_f32=1, ws=int(ws),
                colsum=int(colsum), env=dict(env or {}))


TT_MN = [(128, 128), (256, 384)]
TT_TWO_STAGE_K = [128, 129, 191, 192, 193, 448]            # 2, 3, 3, 3, 4, 7 slabs: below the ring's 8; tails of 1, 63 and 0 rows
TT_RING_K = [512, 513, 575, 576, 640, 1024]                # 8, 9, 9, 9, 10, 16 slabs
# (K, switches, S, krun, last run's slabs) of 128 x 128 with a workspace
TT_RUNS = [(1537, {}, 2, 13, 12), (97 * 64 - 5, {}, 8, 13, 6), (157 * 64 - 63, dict(SL_TT_MAX_SPLITS="16"), 13, 13, 1),
           (158 * 64, dict(SL_TT_MAX_SPLITS="16"), 13, 13, 2)]
TT_RUN_VARIANTS = [("ring", {}), ("two_stage", dict(SL_TT_RING="0")), ("slots256", dict(SL_SPLITK_SLOTS="256"))]


def tiles(M, N, t=128):
    return ((M + t - 1) // t) * ((N + t - 1) // t)


def tt_cases():
    out = []
    for M, N in TT_MN:
        nt = tiles(M, N)
        for K in TT_TWO_STAGE_K:
            out.append(tt_spec(f"tt2-{M}x{N}x{K}", M, N, K, "two_stage", f"{nt},1,1", wide=M == 256))
        for K in TT_RING_K:
            out.append(tt_spec(f"ttring-{M}x{N}x{K}", M, N, K, "ring", f"{nt},1,1", wide=M == 256))
            out.append(tt_spec(f"ttring0-{M}x{N}x{K}", M, N, K, "two_stage", f"{nt},1,1", wide=M == 256, env=dict(SL_TT_RING="0")))
    for K, env, S, krun, _last in TT_RUNS:
        for name, env2 in TT_RUN_VARIANTS:
            form = "two_stage" if name == "two_stage" else "ring"
            out.append(tt_spec(f"ttruns-{name}-{K}", 128, 128, K, form, f"1,{S},1", S=S, krun=krun, ws=True, env=dict(env, **env2)))
    return out


def with_rider(s):
    return dict(s, id=s["id"] + "+db", colsum=1)


# batched form: the positional conv's strides (the plan table's tt_batched row)
TTB_LDA, TTB_LDW, TTB_SA, TTB_SW = 1024, 2048, 64, 128
TTB = [(M, b, K) for M in (64, 128) for b in (1, 2, 3) for K in (128, 130, 496)]


def ttb_spec(M, batch, K, spaced, env=None):
    """spaced: every batch's C slab takes 128 rows (M = 64: rows 64 ... 127 keep the sentinel); else the slabs lie back to back"""
    N = 128
    ldc = ld_of(N)
    sC = (128 if spaced else M) * ldc
    off = bool(env)
    if batch == 1:        # one product: the unbatched rules (M = 64 is refused there and takes the register-staged loader)
        fam, form, grid, krun = ("tt", "two_stage", "1,1,1", slabs(K)) if M == 128 else ("reg128", "none", "1,1,1", 0)      # (SL_TT_BATCHED is not read)
        if M == 128 and slabs(K) >= 8:
            form = "ring"
    elif off:
        fam, form, grid, krun = "reg128", "none", f"1,{batch},1", 0
    else:
        fam, form, grid, krun = "tt", "batched", f"1,1,{batch}", slabs(K)
    return spec(f"ttb-{M}x{batch}x{K}-{'spaced' if spaced else 'dense'}{'-off' if off else ''}", BF16, M, N, K, plan_str(fam, form, grid, 1, krun), ta=1, tw=1,
                lda=TTB_LDA, ldw=TTB_LDW, ldc=ldc, ldr=ldc, batch=batch, sA=TTB_SA, sW=TTB_SW, sC=sC, sR=sC, out_f32=1, res=1, res_f32=1, env=dict(env or {}))


def ttb_cases():
    out = []
    for M, b, K in TTB:
        for spaced in (True, False):
            out.append(ttb_spec(M, b, K, spaced))
            out.append(ttb_spec(M, b, K, spaced, env=dict(SL_TT_BATCHED="0")))
    return out


# refusals: shapes the token-major kernel must not take (they run the register-staged loader, part B)
def tt_refused_cases():
    reg = lambda M, N: plan_str("reg128", "none", f"{tiles(M, N)},1,1")
    mk = lambda sid, dt, M, N, K: spec(sid, dt, M, N, K, reg(M, N), ta=1, tw=1, lda=ld_of(M), ldw=ld_of(N), ldc=ld_of(N), ldr=ld_of(N), out_f32=1, res=1, res_f32=1)
    return [mk("ttref-m192", BF16, 192, 128, 512), mk("ttref-k127", BF16, 128, 128, 127), mk("ttref-f32", F32, 128, 128, 512),
            mk("ttref-n136", BF16, 128, 136, 512)]


# ---- B: the register-staged transposed loader
REG_MN = [(64, 70), (70, 203), (130, 64), (200, 130), (203, 200)]
REG_K = [8, 40, 64, 72, 200]
REG_K_BOTH = [1, 63, 65, 129]
REG_MODES = [("tw", 0, 1), ("ta", 1, 0), ("both", 1, 1)]


def reg_spec(dt, M, N, K, ta, tw, **kw):
    return spec(f"reg-{'ta' * ta}{'tw' * tw}-{M}x{N}x{K}", dt, M, N, K, plan_str("reg128", "none", f"{tiles(M, N)},1,1"), ta=ta, tw=tw,
                lda=ld_of(M if ta else K), ldw=ld_of(N if tw else K), ldc=ld_of(N), ldr=ld_of(N), **kw)


def reg_cases(dt):
    out = [reg_spec(dt, M, N, K, ta, tw) for _, ta, tw in REG_MODES for M, N in REG_MN for K in REG_K]
    out += [reg_spec(dt, M, N, K, 1, 1) for M, N in REG_MN[1::2] for K in REG_K_BOTH]
    return out


CONV_WINDOWS = [(23, 64, 3, 2), (101, 64, 3, 2)]       # (Lin, C, k, s); 96 output channels
CONV_C2 = 96


def conv_spec(dt, Lin, Cc, k, s):
    Lo = (Lin - k) // s + 1
    return spec(f"regconv-{Lin}", dt, CONV_C2, k * Cc, Lo, plan_str("reg128", "none", f"{tiles(CONV_C2, k * Cc)},1,1"), ta=1, tw=1, lda=ld_of(CONV_C2), ldw=s * Cc,
                ldc=ld_of(k * Cc), ldr=ld_of(k * Cc), out_f32=1, res=1, res_f32=1)


# ---- C: the training epilogue riders on every epilogue implementation.  (form, switches, M, N, K, workspace)
T256 = dict(SL_T256_MIN_TILES="1", SL_T256_MIN_K="64")
EPI_FORMS = {
    "rows128": ({}, 130, 96, 192, False),
    "direct128": ({}, 130, 203, 192, False),
    "direct128_switch": (dict(SL_DIRECT_EPILOGUE="1"), 130, 96, 192, False),
    "sw256": (dict(T256, SL_NO_SWAP_EPILOGUE="0"), 500, 200, 128, False),
    "rows256": (dict(T256, SL_NO_SWAP_EPILOGUE="1"), 500, 200, 128, False),
    "rows256_n196": (dict(T256, SL_NO_SWAP_EPILOGUE="0"), 500, 196, 128, False),
    "direct256": (dict(T256, SL_NO_SWAP_EPILOGUE="0"), 500, 203, 128, False),
    "reduce": ({}, 130, 132, 3072, True),
}
SILU_F = {"rows128": [64, 96], "direct128_switch": [64, 96], "sw256": [208], "rows256": [208], "reduce": [144]}     # F = N of the product; 96, 208, 144: no multiple of 64


def epi_spec(form, dt, feature, plan, N=None, **kw):
    env, M, N0, K, ws = EPI_FORMS[form]
    N = N0 if N is None else N
    return spec(f"epi-{form}-{feature}-{N}", dt, M, N, K, plan, feature=feature, lda=ld_of(K), ldw=ld_of(K), ldc=kw.pop("ldc", ld_of(N)), ws=int(ws), env=dict(env), **kw)


# feature -> the fields of the call; the forms that take it are listed in EPI_PLANS
def epi_feature(feature, N):
    if feature == "auxgelu":
        return dict(act=GELU, bias=1, aux=1)
    if feature == "drop":
        return dict(post=DROPOUT, bias=1, res=1, ldr=ld_of(N), drop_p=0.5, drop_ld=N + 40)
    if feature == "gbwd":
        return dict(post=GELU_BWD, post_ld=ld_of(N), drop_p=0.5, drop_ld=N + 40)
    if feature == "gbwd+db":
        return dict(post=GELU_BWD, post_ld=ld_of(N), drop_p=0.5, drop_ld=N + 40, colsum=1)
    if feature == "silubwd":
        return dict(post=SILU_BWD, post_ld=ld_of(2 * N), ldc=ld_of(2 * N))
    if feature == "db":
        return dict(colsum=1)
    raise KeyError(feature)


def _p128(fam, form, M, N):
    return plan_str(fam, form, f"{tiles(M, N)},1,1")


def _p256(form, M, N):
    return plan_str("t256", form, f"{tiles(M, N, 256)},1,1")


# (form, feature) -> plan per dtype; a form missing for a feature does not take it (the reduce pass sums no columns and keeps no copy)
def epi_plan(form, feature, dt, N):
    env, M, _, K, ws = EPI_FORMS[form]
    if form in ("rows128", "direct128", "direct128_switch"):
        return _p128("glds128", "asm", M, N)
    if form == "reduce":
        bk = 64 if dt == BF16 else 32
        nkt = K // bk
        S = min(8, nkt // 12)
        while nkt % S:
            S -= 1
        inner = "ring128" if dt == BF16 else "glds128"
        return plan_str(inner, "4" if dt == BF16 else "asm", f"{tiles(M, N)},{S},1", S, nkt // S, "reduce")
    sw = form == "sw256" and dt == BF16 and N % 8 == 0 and feature != "db"
    return _p256("phased_sw" if sw else "phased", M, N)


EPI_FEATURES = {
    "rows128": ["auxgelu", "drop", "gbwd", "gbwd+db", "silubwd", "db"],
    "direct128": ["auxgelu", "drop", "gbwd+db", "db"],
    "direct128_switch": ["auxgelu", "drop", "gbwd+db", "silubwd", "db"],
    "sw256": ["auxgelu", "drop", "gbwd+db", "silubwd", "db"],
    "rows256": ["auxgelu", "drop", "gbwd+db", "silubwd", "db"],
    "rows256_n196": ["auxgelu", "drop", "gbwd+db", "db"],
    "direct256": ["auxgelu", "drop", "gbwd+db", "db"],
    "reduce": ["drop", "gbwd", "silubwd"],
}


def epi_cases(dt):
    out = []
    for form, feats in EPI_FEATURES.items():
        for ft in feats:
            for N in (SILU_F[form] if ft == "silubwd" else [EPI_FORMS[form][2]]):
                out.append(epi_spec(form, dt, ft, epi_plan(form, ft, dt, N), N=N, **epi_feature(ft, N)))
    return out


def tt_route_cases(dt):
    """both operands transposed in bf16 at a shape the token-major kernel takes: SL_WGRAD_TR=0 sends it through the register-staged loader"""
    if dt != BF16:
        return []
    a = tt_spec("route-tt", 128, 128, 200, "two_stage", "1,1,1")
    b = dict(a, id="route-reg", plan=plan_str("reg128", "none", "1,1,1"), env=dict(SL_WGRAD_TR="0"))
    return [a, b]


# ops.wgrad_acc through sl_transpose_pad copies (M >= 256 token rows and not token-major): (tokens, Nout, Kin)
TPAD = {F32: [(257, 130, 136), (320, 130, 136)], BF16: [(257, 128, 192), (320, 128, 192)]}


def tpad_cases(dt):
    out = []
    for T, No, Ni in TPAD[dt]:
        Tp = (T + 63) // 64 * 64
        out.append(spec(f"tpad-{T}", dt, No, Ni, Tp, _p128("glds128", "asm", No, Ni), lda=Tp, ldw=Tp, ldc=ld_of(Ni), ldr=ld_of(Ni), out_f32=1, res=1, res_f32=1))
    return out


# ---- D: K runs left to the consumer (deferred_splits), 128 tile: 32 slabs are cut in two, 31 are not
def defer_cases(dt):
    bk = 64 if dt == BF16 else 32
    M, N = 130, 132
    inner, form = ("ring128", "4") if dt == BF16 else ("glds128", "asm")
    cut = spec("defer-32", dt, M, N, 32 * bk, plan_str(inner, form, f"{tiles(M, N)},2,1", 2, 16, "defer"), lda=ld_of(32 * bk), ldw=ld_of(32 * bk), ldc=ld_of(N), ws=1, defer=1)
    not_cut = spec("defer-31", dt, M, N, 31 * bk, plan_str(inner, form, f"{tiles(M, N)},1,1"), lda=ld_of(31 * bk), ldw=ld_of(31 * bk), ldc=ld_of(N), ws=1, defer=1)
    return [cut, not_cut]
