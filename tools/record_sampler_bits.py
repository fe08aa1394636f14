"""Record, bit for bit, what the device sampler draws: tests/golden/sampler_bits.npz, the fixture of tests/test_sampler_bits_gpu.py.

For every launch below (256 rows, select_ref.SEED, select_ref.gen_counts()) the file holds the drawn ids (int32) and the words of the drawn
log-probabilities (the float32 viewed as int32), under "<case>__ids" and "<case>__lp":
  sc_g_<name>       every select_ref.G_NAMES row through ops.sample_select_sc
  sc_e_<form>_<V>   select_ref.E_FORMS (all eight patterns) at select_ref.E_SIZES through ops.sample_select_sc
  w_g_<name>        every warp_ref.G_NAMES row (NaN rows among them) through ops.sample_select_w with log-probabilities
  w_l_<name>        every warp_ref.LADDERS row through ops.sample_select_w
  w_e_<form>_<V>    warp_ref.E_FORMS at warp_ref.SIZES through ops.sample_select_w
Only the two public wrappers are used, so the same file runs on any build of the library:

    python tools/record_sampler_bits.py [--out tests/golden/sampler_bits.npz]

Run it on the commit whose bits are to be kept, BEFORE a change to the selection kernels, never after one to make a test pass.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import select_ref as sr  # noqa: E402
import warp_ref as wr  # noqa: E402

PKG = "llm-speech-summarization_amd"
GEN = sr.gen_counts()


def _rows(x):
    return np.repeat(np.asarray(x, dtype=np.float32)[None, :], sr.B, axis=0)


def cases():
    """-> {case: make}, make() -> (logits (256, V) fp32, parameter dict of warp_ref.params, warped: through sample_select_w?)"""
    out = {}

    def sc_g(name):
        x, T, k, p = sr.g_case(name)
        return _rows(x), wr.params(temperature=T, top_k=k, top_p=p), False

    def sc_e(V, form):
        logits, T, k, p, _ = sr.e_launch(V, form)
        return logits, wr.params(temperature=T, top_k=k, top_p=p), False

    def w_g(name):
        x, p = wr.g_case(name)
        return _rows(x), p, True

    def w_l(name):
        x, p = wr.ladder(name)
        return _rows(x), p, True

    def w_e(V, form):
        logits, p, _ = wr.e_launch(V, form)
        return logits, p, True

    for name in sr.G_NAMES:
        out[f"sc_g_{name}"] = lambda name=name: sc_g(name)
    for V in sr.E_SIZES:
        for form in sr.E_FORMS:
            out[f"sc_e_{form}_{V}"] = lambda V=V, form=form: sc_e(V, form)
    for name in wr.G_NAMES:
        out[f"w_g_{name}"] = lambda name=name: w_g(name)
    for name in wr.LADDERS:
        out[f"w_l_{name}"] = lambda name=name: w_l(name)
    for V in wr.SIZES:
        for form in wr.E_FORMS:
            out[f"w_e_{form}_{V}"] = lambda V=V, form=form: w_e(V, form)
    return out


def draw(ops, make, dev="cuda:0"):
    """one launch -> (ids (256) int32, words of the drawn log-probabilities (256) int32)"""
    logits, p, warped = make()
    rows = logits.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    st = [torch.ones(rows, **i32), torch.arange(rows, **i32), torch.tensor(GEN, **i32), torch.zeros(rows, **i32), torch.full((rows,), -7, **i32),
          torch.full((rows, sr.MAX_NEW), -1, **i32)]
    lp = torch.full((rows, sr.MAX_NEW), 7.0, dtype=torch.float32, device=dev)
    a = (torch.from_numpy(logits).to(dev), p["temperature"], p["top_k"], p["top_p"], sr.SEED, [], 0, False, *st, lp)
    if warped:
        ops.sample_select_w(*a, wr.warp_of(p))
    else:
        ops.sample_select_sc(*a)
    torch.cuda.synchronize()
    ids = st[4].cpu().numpy().astype(np.int32)
    words = lp.cpu().numpy()[np.arange(rows), np.asarray(GEN)].view(np.int32)
    return ids, words.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "sampler_bits.npz"))
    args = ap.parse_args()
    ops = importlib.import_module(PKG + ".ops")
    rec = {}
    for case, make in cases().items():
        rec[case + "__ids"], rec[case + "__lp"] = draw(ops, make)
        print(f"{case}: ids {rec[case + '__ids'][:4]} .. lp words {rec[case + '__lp'][:2]} ..", flush=True)
    np.savez_compressed(args.out, **rec)
    print(f"{len(rec) // 2} launches -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
