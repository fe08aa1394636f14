"""CPU: the references, bounds and case tables of tests/train_gemm_ref.py (the edge suite's fourth chapter) are right, not vacuous and
not too tight.

(a) every reference equals torch's fp64 autograd of the same operation to 1e-12: dW and db of F.linear, the conv weight gradient, GELU and
    SwiGLU backward, dropout as a fixed mask;
(b) an fp32 restatement of each route (stored inputs, fp32 accumulation per K run, runs summed in run order, the rider out of atomics in a
    random order, the epilogues' roundings to the storage type) stays inside every bound; the worst err / tol is printed;
(c) the restatement with one defect planted in it leaves the bound, or breaks the exact case that pins it;
(d) every class-G shape has a reduction of at most 1 024 terms;
(e) the dispatcher's dry run (SL_GEMM_LOG=2: plan, print, launch nothing; a child process, as tests/test_gemm_plan_cpu.py) gives every
    spec of the case tables the plan the GPU file claims for it, so that the smallest shapes select what they say.
No number here is measured."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import train_gemm_ref as G
import train_ops_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = G.BF16, G.F32
DTS = [F32, BF16]


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def worst(got, ref, tol):
    return float(((got - ref).abs() / tol).max())


def outside(got, ref, tol):
    return ~((got - ref).abs() <= tol)


def stored(x, dt):
    return G.rnd(x, dt)


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations
# ------------------------------------------------------------------------------------------------------------------------------
def test_weight_gradient_references_equal_autograd():
    T, No, Ni = 37, 12, 20
    dy, x, dw0, db0 = R.gauss((T, No), 1), R.gauss((T, Ni), 2), R.gauss((No, Ni), 3), R.gauss((1, No), 4)
    W, b = torch.zeros(No, Ni, dtype=torch.float64, requires_grad=True), torch.zeros(No, dtype=torch.float64, requires_grad=True)
    F.linear(x, W, b).backward(dy)
    r = G.wgrad_ref(dy, x, dw0, db0)
    assert close(r.dw - dw0, W.grad) and close(r.db - db0, b.grad[None])
    for Lin, Cc, k, s_ in G.CONV_WINDOWS:
        Lo, C2 = (Lin - k) // s_ + 1, 5
        xc, dyc = R.gauss((Lin, Cc), 5), R.gauss((Lo, C2), 6)
        w = torch.zeros(C2, Cc, k, dtype=torch.float64, requires_grad=True)
        F.conv1d(xc.T[None], w, stride=s_)[0].T.backward(dyc)
        r = G.wgrad_ref(dyc, G.windows(xc, Lo, k, s_), torch.zeros(C2, k * Cc, dtype=torch.float64))
        assert close(r.dw, w.grad.permute(0, 2, 1).reshape(C2, k * Cc))


def test_epilogue_references_equal_autograd():
    M, N, K = 9, 32, 24
    a, w, b, res = R.gauss((M, K), 1), R.gauss((N, K), 2), R.gauss((N,), 3), R.gauss((M, N), 4)
    keep = torch.rand(M, N, generator=torch.Generator().manual_seed(5)) > 0.25
    lin = F.linear(a, w, b)
    r = G.aux_gelu_ref(a, w, b, F32)
    assert close(r.aux, lin) and close(r.c, F.gelu(lin))
    assert close(G.dropout_ref(a, w, b, res, keep, 0.25, F32).c, res + keep.double() / 0.75 * lin)
    assert close(G.plain_ref(a, w, F32, bias=b, res=res).c, lin + res)
    # GELU backward behind the data-gradient product: upstream d = dropout(dY W)
    pre = R.gauss((M, N), 6, 2.0).requires_grad_()
    d = keep.double() / 0.75 * F.linear(a, w)
    F.gelu(pre).backward(d)
    assert close(G.gelu_bwd_post_ref(a, w, pre.detach(), keep, 0.25, F32).c, pre.grad)
    pre.grad = None
    F.gelu(pre).backward(F.linear(a, w))
    assert close(G.gelu_bwd_post_ref(a, w, pre.detach(), None, 0.0, F32).c, pre.grad)
    g, up = R.gauss((M, N), 7, 3.0).requires_grad_(), R.gauss((M, N), 8).requires_grad_()
    (F.silu(g) * up).backward(F.linear(a, w))
    r = G.silu_bwd_post_ref(a, w, g.detach(), up.detach(), F32)
    assert close(r.dgate, g.grad) and close(r.dup, up.grad)
    # the bias gradient of the stored values
    bb = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    (lin.detach() + bb).backward(torch.ones(M, N, dtype=torch.float64))
    db0 = R.gauss((1, N), 9)
    assert close(G.colsum_ref(lin.detach(), db0).db - db0, (bb.grad * lin.detach().sum(0) / M)[None])


# ------------------------------------------------------------------------------------------------------------------------------
# (b), (c) fp32 restatements stay inside the bounds; with a planted defect they leave them (or break the exact case)
# ------------------------------------------------------------------------------------------------------------------------------
WG_SHAPES = [(128, 128, K) for K in G.TT_TWO_STAGE_K + G.TT_RING_K] + [(256, 384, 193), (256, 384, 576)]


def wgrad_inputs(M, N, K, cls):
    if cls == "E":
        return R.ints((K, M), -2, 2, 1), R.ints((K, N), -2, 2, 2), 8 * R.ints((M, N), -512, 512, 3), R.ints((1, M), -8, 8, 4) + 0.0
    return stored(R.gauss((K, M), 1), BF16), stored(R.gauss((K, N), 2), BF16), stored(R.gauss((M, N), 3), F32), stored(R.gauss((1, M), 4), F32)


@pytest.mark.parametrize("M,N,K", WG_SHAPES)
def test_token_major_restatement_inside_the_bounds_and_defects_outside(M, N, K):
    rng = torch.Generator().manual_seed(K)
    dy, x, dw0, db0 = wgrad_inputs(M, N, K, "G")
    r = G.wgrad_ref(dy, x, dw0, db0)
    worst_w = worst_b = 0.0
    for krun in {G.slabs(K), 2, 1}:          # one run; runs of two slabs and of one, summed in run order
        dw, db = G.wgrad_sim(dy, x, dw0, db0[0], krun, rng=rng)
        worst_w, worst_b = max(worst_w, worst(dw, r.dw, r.tol_dw)), max(worst_b, worst(db[None], r.db, r.tol_db))
    print(f"wgrad {M} x {N} x {K}: worst err / tol dW {worst_w:.3g} db {worst_b:.3g}")
    assert worst_w <= 1.0 and worst_b <= 1.0
    e = wgrad_inputs(M, N, K, "E")
    exact = (e[2] + e[0].T @ e[1], e[3] + e[0].sum(0))

    def planted(defect, krun=G.slabs(K), **kw):
        gw, gb = G.wgrad_sim(dy, x, dw0, db0[0], krun, rng=rng, defect=defect, **kw)
        ew, eb = G.wgrad_sim(e[0], e[1], e[2], e[3][0], krun, defect=defect, **kw)
        return outside(gw, r.dw, r.tol_dw), outside(gb[None], r.db, r.tol_db), not torch.equal(ew, exact[0]), not torch.equal(eb[None], exact[1])

    ow, ob, ew, eb = planted("drop_last_row")                 # one token row dropped from the last slab
    assert float(ow.double().mean()) > 0.5 and ew, float(ow.double().mean())      # (at 1 024 tokens a product of two small values stays under the bound)
    if G.slabs(K) >= 2:
        ow, ob, ew, eb = planted("first_slab_twice", krun=1)  # a run's first slab counted twice
        assert float(ow.double().mean()) > 0.99 and ew
    ow, ob, ew, eb = planted("rider_every_column_tile", tiles_n=3)      # the rider added by every column tile
    assert float(ob.double().mean()) > 0.9 and eb and not ow.any() and not ew
    ow, ob, ew, eb = planted("rider_quarter")                 # the rider missing one 16-row fragment: the historic quarter
    assert int(ob[0, 16:32].sum()) >= 14 and int(ob.sum()) == int(ob[0, 16:32].sum()) and eb
    # the tail row K (poison) included
    poison = torch.full((1, M), 1e30, dtype=torch.float64)
    gw, gb = G.wgrad_sim(torch.cat([dy, poison]), torch.cat([x, torch.full((1, N), -1e30, dtype=torch.float64)]), dw0, db0[0], G.slabs(K + 1))
    assert outside(gw, r.dw, r.tol_dw).all() and outside(gb[None], r.db, r.tol_db).all()


def test_sentinel_checks_catch_rows_and_chunk_tails_that_must_not_be_stored():
    from edge_helpers import FILL, bad, untouched
    # rows 64 ... 127 of a 64-row batched tile written: the expected slab holds the sentinel there
    want = torch.full((192, 128), FILL)
    want[:64], want[128:] = 1.0, 2.0
    got = want.clone()
    got[64:128] = 0.0
    assert "8192 of" in bad(got, want)
    # a straddling chunk's tail stored: the element behind the extent / the row below the last
    for M, N in ((70, 203), (203, 70)):
        ld = (N + 7) // 8 * 8 + 16
        buf = torch.full((M + 2, ld), FILL)
        buf[1:M + 1, 8:8 + N] = 3.0
        assert untouched(buf, M, N)
        b2 = buf.clone()
        b2[1:M + 1, 8 + N] = 3.0              # column N of every row (N = 203: the 8-element chunk 200 ... 207)
        b3 = buf.clone()
        b3[M + 1, 8:8 + N] = 3.0              # tile row M (M = 70: the chunk 64 ... 71 of a transposed A)
        assert not untouched(b2, M, N) and not untouched(b3, M, N)


EPI_SHAPES = sorted({(M, N, K) for _, M, N, K, _ in G.EPI_FORMS.values() if K <= G.G_MAX_K and (M, N) not in ((500, 196), (500, 203))})      # (N = 203 at 130 rows)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_epilogue_restatements_inside_the_bounds_and_defects_outside(M, N, K, dt):
    a, w = stored(R.gauss((M, K), 1), dt), stored(R.gauss((N, K), 2, K ** -0.5), dt)
    b, res = stored(R.gauss((N,), 3), dt), stored(R.gauss((M, N), 4), dt)
    drop_ld, ldc, seed = N + 40, G.ld_of(N), 0x5DEECE66D1234567
    rep = {}
    # pre-activation copy + GELU
    r = G.aux_gelu_ref(a, w, b, dt)
    pre32 = G.product_sim(a, w, b)
    rep["aux"] = worst(G.rt(pre32, dt).double(), r.aux, r.tol_aux)
    rep["gelu"] = worst(G.rt(0.5 * pre32 * (1.0 + torch.erf(pre32 * 0.70710678118654752440)), dt).double(), r.c, r.tol_c)
    # dropout onto the residual
    for p_ in (0.5, 0.25):
        keep = G.keep_mask(M, N, drop_ld, p_, seed)
        r = G.dropout_ref(a, w, b, res, keep, p_, dt)
        rep[f"drop{p_}"] = worst(G.dropout_sim(a, w, b, res, keep, p_, dt), r.c, r.tol_c + 1e-300)
        wrong = G.dropout_sim(a, w, b, res, G.keep_mask(M, N, ldc, p_, seed), p_, dt)         # the mask indexed with ldc for drop_ld
        assert outside(wrong, r.c, r.tol_c).sum() > 0.2 * M * N
    # GELU backward (+ dropout), and gelu' of the rounded product instead of the saved pre-activation
    pre = stored(R.gauss((M, N), 5, 2.0), dt)
    for p_ in (0.0, 0.25):
        keep = G.keep_mask(M, N, drop_ld, p_, seed + 1) if p_ else None
        r = G.gelu_bwd_post_ref(a, w, pre, keep, p_, dt)
        rep[f"gbwd{p_}"] = worst(G.gelu_bwd_post_sim(a, w, pre, keep, p_, dt), r.c, r.tol_c)
        assert outside(G.gelu_bwd_post_sim(a, w, pre, keep, p_, dt, on_rounded_c=True), r.c, r.tol_c).sum() > 0.3 * M * N
    # SwiGLU backward, and gate / up exchanged in one 16-column block
    if N % 16 == 0:
        g, up = stored(R.gauss((M, N), 6, 2.0), dt), stored(R.gauss((M, N), 7), dt)
        r = G.silu_bwd_post_ref(a, w, g, up, dt)
        dg, du = G.silu_bwd_post_sim(a, w, g, up, dt)
        rep["silu"] = max(worst(dg, r.dgate, r.tol_dgate), worst(du, r.dup, r.tol_dup))
        blk = N // 16 - 1
        dg, du = G.silu_bwd_post_sim(a, w, g, up, dt, swap_block=blk)
        og, ou = outside(dg, r.dgate, r.tol_dgate), outside(du, r.dup, r.tol_dup)
        assert og[:, 16 * blk:].double().mean() > 0.9 and not og[:, :16 * blk].any() and ou[:, 16 * blk:].double().mean() > 0.9
    # plain product and the column sums of its stored values, summed in a random order of the rows
    r = G.plain_ref(a, w, dt, bias=b, res=res)
    rep["plain"] = worst(G.rt(G.product_sim(a, w, b, nruns=3) + res.float(), dt).double(), r.c, r.tol_c)
    c = G.rt(G.product_sim(a, w), dt)
    db0 = stored(R.gauss((1, N), 8), F32)
    rb = G.colsum_ref(c.double(), db0)
    acc = db0[0].float().clone()
    for i in torch.randperm(M, generator=torch.Generator().manual_seed(1)).tolist():
        acc = acc + c[i]
    rep["db"] = worst(acc.double()[None], rb.db, rb.tol_db)
    print(f"epilogue {M} x {N} x {K} {dt}: worst err / tol " + " ".join(f"{k} {v:.3g}" for k, v in rep.items()))
    assert max(rep.values()) <= 1.0, rep


# ------------------------------------------------------------------------------------------------------------------------------
# (d) class G keeps to reductions of at most 1 024 terms; longer ones are class E only
# ------------------------------------------------------------------------------------------------------------------------------
def test_class_g_reductions_are_short():
    assert G.G_MAX_K == 1024
    assert max(G.TT_TWO_STAGE_K + G.TT_RING_K + G.REG_K + G.REG_K_BOTH + [K for _, _, K in G.TTB]) <= G.G_MAX_K
    assert all((Lin - k) // s + 1 <= G.G_MAX_K for Lin, _, k, s in G.CONV_WINDOWS)
    assert all(s["K"] <= G.G_MAX_K for dt in DTS for s in G.epi_cases(dt) if G.class_g(s))
    long_ = [s for s in all_specs() if s["K"] > G.G_MAX_K]
    assert long_ and not any(G.class_g(s) for s in long_)
    assert {s["id"].split("-")[0] for s in long_} == {"ttruns", "epi", "defer"}


# ------------------------------------------------------------------------------------------------------------------------------
# (e) plans
# ------------------------------------------------------------------------------------------------------------------------------
def all_specs():
    out = []
    for s in G.tt_cases():
        out += [s, G.with_rider(s)]
    out += G.ttb_cases() + G.tt_refused_cases()
    for dt in DTS:
        out += G.reg_cases(dt) + [G.conv_spec(dt, *c) for c in G.CONV_WINDOWS] + G.tt_route_cases(dt) + G.tpad_cases(dt) + G.epi_cases(dt)
        out += G.defer_cases(dt)
    ids = [(s["id"], s["dt"]) for s in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def child():
    sys.path.insert(0, REPO)
    import importlib
    L = importlib.import_module("llm-speech-summarization_amd._lib")
    lib = L.lib()
    PTR = 0x7000000000      # dummy device addresses, 16-byte aligned; the dry run never reads them
    ws_bytes = lib.sl_gemm_streamk_workspace_bytes()
    cur = {}
    for i, s in enumerate(all_specs()):
        if s["env"] != cur:
            for k in cur:
                os.environ.pop(k)
            os.environ.update(s["env"])
            lib.sl_tuning_reload()
            cur = s["env"]
        g = lambda k, d=0: s.get(k, d)
        a = L.GemmArgs()
        a.M, a.N, a.K, a.batch, a.act, a.out_f32 = s["M"], s["N"], s["K"], g("batch", 1), g("act"), g("out_f32")
        a.dtype = {BF16: L.SL_BF16, F32: L.SL_F32}[s["dt"]]
        a.A, a.W, a.C = PTR, PTR + (1 << 32), PTR + (2 << 32)
        a.lda, a.ldw, a.ldc = s["lda"], s["ldw"], s["ldc"]
        a.strideA, a.strideW, a.strideC, a.strideR = g("sA"), g("sW"), g("sC"), g("sR")
        if g("bias"):
            a.bias = PTR + (3 << 32)
        if g("res"):
            a.residual, a.ldr = PTR + (2 << 32 if g("res_f32") else 4 << 32), s["ldr"]
        ex = L.GemmEx()
        ex.w_mod, ex.trans_a, ex.trans_w, ex.residual_f32 = 1, g("ta"), g("tw"), g("res_f32")
        defer = C.c_int32(-1)
        if g("ws"):
            ex.sk_ws, ex.sk_ws_bytes = PTR + (5 << 32), ws_bytes
        if g("defer"):
            ex.deferred_splits = C.addressof(defer)
        if g("aux"):
            ex.aux_out = PTR + (7 << 32)
        if g("colsum"):
            ex.colsum_out = PTR + (14 << 32)
        if g("post"):
            ex.post_op = g("post")
            ex.drop_p, ex.drop_ld = g("drop_p", 0.0), g("drop_ld")
            if ex.post_op != G.DROPOUT:
                ex.post_in, ex.post_ld = PTR + (15 << 32), s["post_ld"]
        os.write(2, f"ROW {i}\n".encode())
        rc = lib.sl_gemm_ex(C.byref(a), C.byref(ex), None)
        os.write(2, f"RC {rc} {lib.sl_last_error().decode(errors='replace') if rc else ''}\n".encode())


def run_child():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SL_")}
    env["SL_GEMM_LOG"] = "2"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    out, key, plan = {}, None, None
    for line in r.stderr.splitlines():
        if line.startswith("ROW "):
            key, plan = int(line[4:]), None
        elif line.startswith("SLPLAN ") and key is not None:
            assert plan is None, f"two plan lines for spec {key}"
            plan = " ".join(f for f in line[7:].split() if not f.startswith(("tm=", "tn=")))
        elif line.startswith("RC ") and key is not None:
            out[key] = (plan, line[3:].strip())
            key = None
    return out


def test_every_spec_of_the_case_tables_takes_the_plan_the_gpu_file_claims():
    specs = all_specs()
    got = run_child()
    assert len(got) == len(specs)
    diff = [(s["id"], str(s["dt"]), got[i][0], s["plan"], got[i][1]) for i, s in enumerate(specs) if got[i][0] != s["plan"] or got[i][1] != "0"]
    assert not diff, "plan differs from the claimed one (id, dtype, got, claimed, rc):\n" + "\n".join(map(str, diff))


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    elif sys.argv[1:] == ["--probe"]:
        for i, (plan, rc) in sorted(run_child().items()):
            s = all_specs()[i]
            print(("ok  " if plan == s["plan"] and rc == "0" else "DIFF"), s["id"], str(s["dt"])[6:], "|", plan, "|", s["plan"], "|", rc)
