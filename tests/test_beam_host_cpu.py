"""CPU (no GPU): the beam-search surface — header / exports / struct mirrors, every limit of sl_beam_generate reported before any
launch, runtime_beams parsing, the Python keywords' errors, and the plain-torch restatement (tests/beam_ref.py) replayed against
what the reference class returned (tests/golden/beam_tiny.npz, written by tools/gen_beam_golden.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO, golden, pkg, t

import beam_ref

L = pkg("_lib")
cfgm = pkg("config")

CASES = ["mha_k2_eos", "mha_k3_eos_early", "mha_k3_eos_lp2", "mha_k4", "gqa_k2_eos_lp2", "gqa_k4", "mha_k3_eos_never", "mha_k3_eos_r3"]
ES = {0: False, 1: True, 2: "never"}
BEAM_EXPORTS = {"sl_beam_generate_workspace_bytes", "sl_beam_generate", "sl_beam_topk", "sl_beam_step", "sl_kv_beam_staging_bytes", "sl_kv_beam_reorder"}


def test_header_declares_the_beam_entries_and_the_abi_stays_7():
    hdr = open(os.path.join(REPO, "include", "speechllm.h")).read()
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", hdr))
    assert BEAM_EXPORTS <= declared and BEAM_EXPORTS <= set(L.EXPORTS)
    assert L.lib().sl_version() == 7
    assert "no compaction" in hdr          # the header states that done sequences keep their rows


def test_beam_struct_mirrors_match_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = [("sl_beam_opts", L.BeamOpts), ("sl_beam_state", L.BeamState)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "speechllm.h")}"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(out[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def _model(vocab=1000, dtype=L.SL_F32, reserved=0):
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, 256, 2, 2, 2, 128, 384, vocab
    m.rope_len, m.reserved = 64, reserved
    return m


def _kv(slots=64, max_ctx=48):
    kv = L.KVCache()
    kv.slots, kv.max_ctx = slots, max_ctx
    return kv


def _opts(K=4, R=1, n_eos=0, max_new=8, lp=1.0, es=0):
    o = L.BeamOpts()
    eos = (C.c_int32 * 8)(*range(2, 10))
    o.eos_ids_host, o.n_eos, o.use_eos, o.pad_id = eos, n_eos, int(n_eos > 0), 0
    o.max_new_tokens, o.check_every, o.num_beams, o.num_return_sequences, o.early_stopping, o.length_penalty = max_new, 4, K, R, es, lp
    o._keep = eos
    return o


@pytest.mark.parametrize("what,kw,nseq,kvkw,rc,needle", [
    ("num_beams 0", dict(K=0), 2, {}, -1, b"num_beams"),
    ("num_beams 9", dict(K=9), 2, {}, -1, b"num_beams"),
    ("M > 64", dict(K=8, n_eos=8), 2, {}, -3, b"candidates per step"),
    ("rows > SL_MAX_DECODE_BATCH", dict(K=8), 257, dict(slots=4096), -1, b"rows"),
    ("rows > slots", dict(K=4), 3, dict(slots=8), -1, b"cache slots"),
    ("R = 0", dict(K=4, R=0), 2, {}, -1, b"num_return_sequences"),
    ("R > K", dict(K=2, R=3), 2, {}, -1, b"num_return_sequences"),
    ("length_penalty inf", dict(lp=float("inf")), 2, {}, -1, b"finite"),
    ("length_penalty nan", dict(lp=float("nan")), 2, {}, -1, b"finite"),
    ("early_stopping 3", dict(es=3), 2, {}, -1, b"early_stopping"),
])
def test_beam_limits_are_reported_without_a_gpu(what, kw, nseq, kvkw, rc, needle):
    lib = L.lib()
    m, kv, o = _model(), _kv(**kvkw), _opts(**kw)
    assert lib.sl_beam_generate_workspace_bytes(C.byref(m), 40, nseq, C.byref(kv), C.byref(o)) == 0, what
    assert needle in lib.sl_last_error(), (what, lib.sl_last_error())
    cu = (C.c_int32 * (nseq + 1))(*[10 * i for i in range(nseq + 1)])
    got = lib.sl_beam_generate(C.byref(m), C.byref(kv), None, cu, nseq, C.byref(o), None, None, None, None, None, 0, None)
    assert got == rc and needle in lib.sl_last_error(), (what, got, lib.sl_last_error())


def test_beam_m_exceeding_the_vocabulary_and_the_context_budget_are_refused():
    lib = L.lib()
    m, kv, o = _model(vocab=6), _kv(), _opts(K=4)          # M = 8 > V = 6
    assert lib.sl_beam_generate_workspace_bytes(C.byref(m), 40, 2, C.byref(kv), C.byref(o)) == 0 and b"vocabulary" in lib.sl_last_error()
    # prompt + max_new_tokens > max_ctx: needs buffers that pass the null checks, but is refused before any launch or device call
    m, kv, o = _model(), _kv(slots=8, max_ctx=48), _opts(K=2, max_new=12)
    for f in ("layers", "embed", "lm_head", "final_norm", "rope_cos", "rope_sin"):
        setattr(m, f, C.cast(1, type(getattr(m, f))) if f == "layers" else 1)
    kv.k_cache = kv.v_cache = 1
    cu = (C.c_int32 * 3)(0, 10, 47)                         # 37 + 12 > 48
    ids, sc, ln = (C.c_int32 * 48)(), (C.c_float * 4)(), (C.c_int32 * 4)()
    rc = lib.sl_beam_generate(C.byref(m), C.byref(kv), 1, cu, 2, C.byref(o), ids, sc, ln, None, 1, 1 << 40, None)
    assert rc == -1 and b"exceeds max_ctx" in lib.sl_last_error(), lib.sl_last_error()


def test_e4m3_decode_weight_row_limit_counts_nseq_times_num_beams():
    lib = L.lib()
    rows = lib.sl_w8_max_rows()
    K = 8
    nseq = rows // K + 1                                    # nseq alone is within the e4m3 range, nseq * K is not
    assert nseq <= rows < nseq * K
    m, kv, o = _model(dtype=L.SL_BF16, reserved=L.WDEC_E4M3), _kv(slots=2048, max_ctx=48), _opts(K=K, max_new=4)
    m.dec_fused_norm = 1
    for f in ("layers", "embed", "lm_head", "final_norm", "rope_cos", "rope_sin", "lm_head_dec"):
        setattr(m, f, C.cast(1, type(getattr(m, f))) if f == "layers" else 1)
    layers = (L.LlamaLayer * 2)()
    for lay in layers:
        for f, _ in L.LlamaLayer._fields_:
            setattr(lay, f, 1)
    m.layers = layers
    kv.k_cache = kv.v_cache = 1
    cu = (C.c_int32 * (nseq + 1))(*[4 * i for i in range(nseq + 1)])
    ids, sc, ln = (C.c_int32 * (nseq * 4))(), (C.c_float * nseq)(), (C.c_int32 * nseq)()
    rc = lib.sl_beam_generate(C.byref(m), C.byref(kv), 1, cu, nseq, C.byref(o), ids, sc, ln, None, 1, 1 << 40, None)
    assert rc == -3 and b"sl_w8_max_rows" in lib.sl_last_error(), (rc, lib.sl_last_error())


# (n_tok, nseq, max_new, penalty on, x, sl_generate_workspace_bytes_sc with scores = x, sl_beam_generate_workspace_bytes_lp with num_beams = x + 1):
# the byte counts the library returned BEFORE the per-row state table and the shared decode-graph builder went in (fp32 model of _model(),
# cache of 256 slots x 48).  The layout is part of the decode-graph key through the workspace pointer, so the counts are pinned, not recomputed.
WORKSPACE_BYTES = [
    (7, 1, 1, 0, 0, 59592, 61444),
    (7, 1, 1, 0, 1, 59852, 77064),
    (7, 1, 1, 1, 0, 59852, 61956),
    (7, 1, 1, 1, 1, 60112, 77576),
    (7, 1, 6, 0, 0, 59612, 61444),
    (7, 1, 6, 0, 1, 59892, 118024),
    (7, 1, 6, 1, 0, 59892, 61956),
    (7, 1, 6, 1, 1, 60172, 118536),
    (7, 3, 1, 0, 0, 74328, 76044),
    (7, 3, 1, 0, 1, 74596, 122648),
    (7, 3, 1, 1, 0, 74596, 76556),
    (7, 3, 1, 1, 1, 74864, 123160),
    (7, 3, 6, 0, 0, 74388, 76044),
    (7, 3, 6, 0, 1, 74716, 245528),
    (7, 3, 6, 1, 0, 74716, 76556),
    (7, 3, 6, 1, 1, 75044, 246040),
    (7, 65, 1, 0, 0, 1461192, 1466628),
    (7, 65, 1, 0, 1, 1461708, 3450632),
    (7, 65, 1, 1, 0, 1461708, 1467652),
    (7, 65, 1, 1, 1, 1462224, 3452168),
    (7, 65, 6, 0, 0, 1462492, 1470468),
    (7, 65, 6, 0, 1, 1464308, 6120712),
    (7, 65, 6, 1, 0, 1464308, 1472772),
    (7, 65, 6, 1, 1, 1466124, 6124808),
    (300, 1, 1, 0, 0, 2011848, 2013700),
    (300, 1, 1, 0, 1, 2012108, 2029320),
    (300, 1, 1, 1, 0, 2012108, 2014212),
    (300, 1, 1, 1, 1, 2012368, 2029832),
    (300, 1, 6, 0, 0, 2011868, 2013700),
    (300, 1, 6, 0, 1, 2012148, 2070280),
    (300, 1, 6, 1, 0, 2012148, 2014212),
    (300, 1, 6, 1, 1, 2012428, 2070792),
    (300, 3, 1, 0, 0, 2026584, 2028300),
    (300, 3, 1, 0, 1, 2026852, 2074904),
    (300, 3, 1, 1, 0, 2026852, 2028812),
    (300, 3, 1, 1, 1, 2027120, 2075416),
    (300, 3, 6, 0, 0, 2026644, 2028300),
    (300, 3, 6, 0, 1, 2026972, 2197784),
    (300, 3, 6, 1, 0, 2026972, 2028812),
    (300, 3, 6, 1, 1, 2027300, 2198296),
    (300, 65, 1, 0, 0, 3026888, 3032324),
    (300, 65, 1, 0, 1, 3027404, 4583176),
    (300, 65, 1, 1, 0, 3027404, 3033348),
    (300, 65, 1, 1, 1, 3027920, 4584712),
    (300, 65, 6, 0, 0, 3028188, 3036164),
    (300, 65, 6, 0, 1, 3030004, 7253256),
    (300, 65, 6, 1, 0, 3030004, 3038468),
    (300, 65, 6, 1, 1, 3031820, 7257352),
]


def test_workspace_byte_counts_are_those_recorded_before_the_state_table():
    lib = L.lib()
    m, kv = _model(), _kv(slots=256, max_ctx=48)
    pen = L.LogitsOpts()
    pen.repetition_penalty = 1.3
    assert len(WORKSPACE_BYTES) == 2 * 3 * 2 * 2 * 2
    for n_tok, nseq, max_new, lp, x, gen, beam in WORKSPACE_BYTES:
        lpr = C.byref(pen) if lp else None
        o = _opts(K=x + 1, max_new=max_new)
        assert lib.sl_generate_workspace_bytes_sc(C.byref(m), n_tok, nseq, max_new, lpr, x) == gen, (n_tok, nseq, max_new, lp, x)
        assert lib.sl_beam_generate_workspace_bytes_lp(C.byref(m), n_tok, nseq, C.byref(kv), C.byref(o), lpr) == beam, (n_tok, nseq, max_new, lp, x)


def test_kernel_level_entries_check_their_arguments_without_a_gpu():
    lib = L.lib()
    assert lib.sl_beam_topk(1, 4, 100, None, 65, 1, 1, None) == -1 and b"M = 65" in lib.sl_last_error()
    assert lib.sl_beam_topk(1, 4, 10, None, 16, 1, 1, None) == -1       # M > V
    assert lib.sl_beam_topk(None, 4, 100, None, 8, 1, 1, None) == -1
    st, o = L.BeamState(), _opts(K=2)
    assert lib.sl_beam_step(C.byref(st), 1, 1, 3, 2, 4, 0, C.byref(o), None) == -1 and b"null state" in lib.sl_last_error()
    m, kv = _model(), _kv(slots=8)
    kv.k_cache = kv.v_cache = 1
    need = lib.sl_kv_beam_staging_bytes(C.byref(kv), C.byref(m), 6, 7)
    assert need == 2 * 6 * 2 * 2 * 7 * 128 * 4
    assert lib.sl_kv_beam_reorder(C.byref(kv), C.byref(m), 1, 1, 1, 6, 7, 16, need - 1, None) == -1 and b"staging" in lib.sl_last_error()
    assert lib.sl_kv_beam_reorder(C.byref(kv), C.byref(m), 1, 1, 1, 9, 7, 16, need * 2, None) == -1 and b"rows" in lib.sl_last_error()


def test_runtime_beams_parsing_and_the_shipped_yamls_default_to_greedy():
    for name in sorted(os.listdir(os.path.join(REPO, "config"))):
        if name.endswith(".yaml"):
            assert cfgm.runtime_beams(cfgm.load_config(os.path.join(REPO, "config", name))) is None, name
    assert cfgm.runtime_beams(cfgm.from_dict(dict(model={}))) is None
    assert cfgm.runtime_beams(cfgm.from_dict(dict(runtime=dict(num_beams=1, length_penalty=2.0)))) is None
    b = cfgm.runtime_beams(cfgm.from_dict(dict(runtime=dict(num_beams=4))))
    assert b == dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1)
    b = cfgm.runtime_beams(cfgm.from_dict(dict(runtime=dict(num_beams=2, length_penalty=0, early_stopping="never"))))
    assert b["length_penalty"] == 0.0 and b["early_stopping"] == "never"
    assert cfgm.runtime_beams(cfgm.from_dict(dict(runtime=dict(num_beams=3, early_stopping=True))))["early_stopping"] is True
    for bad in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=2.5), dict(num_beams=True), dict(num_beams=2, length_penalty="x"),
                dict(num_beams=2, length_penalty=float("inf")), dict(num_beams=2, early_stopping="always")):
        with pytest.raises(ValueError):
            cfgm.runtime_beams(cfgm.from_dict(dict(runtime=bad)))


def _tiny_llm():
    from oracle.golden_cfgs import TINY_MHA as LC
    weights = pkg("weights")
    larch = weights.LlamaArch(LC.hidden_size, LC.num_hidden_layers, LC.num_attention_heads, LC.num_key_value_heads, LC.head_dim,
                              LC.intermediate_size, LC.vocab_size, LC.rms_norm_eps, LC.rope_theta, LC.rope_scaling,
                              LC.tie_word_embeddings, tuple(LC.eos_token_ids), LC.pad_token_id)
    return pkg("audio_llama").AudioLlamaForCausalLM(larch, {}, torch_dtype=torch.float32, max_ctx=64)


def test_generate_keywords_raise_instead_of_decoding_greedily_in_silence():
    llm = _tiny_llm()
    g = llm.generation_config
    assert (g.num_beams, g.length_penalty, g.early_stopping, g.num_return_sequences) == (1, 1.0, False, 1)      # HF's defaults
    x = torch.zeros(1, 4, 256)
    with pytest.raises(L.SpeechLLMError, match="beam sampling"):
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_beams=3, do_sample=True)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_beams=2, num_return_sequences=3)
    with pytest.raises(L.SpeechLLMError, match="num_beams"):
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_beams=0)
    with pytest.raises(L.SpeechLLMError, match="GPU"):        # num_beams is honoured, so without a device the call fails loudly
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_beams=2)
    with pytest.raises(L.SpeechLLMError, match="early_stopping"):
        L.early_stopping_code("sometimes")
    assert [L.early_stopping_code(v) for v in (False, True, "never")] == [0, 1, 2]


def test_generate_packed_refuses_row_limits_or_sampling_with_beams():
    llm = _tiny_llm()
    llm._w = object()          # past the device check: the keyword checks come before any library call
    x = torch.zeros(8, 256)
    with pytest.raises(L.SpeechLLMError, match="row_limits"):
        llm.generate_packed(x, [4, 4], 4, row_limits=[2, 3], beams=dict(num_beams=2))
    with pytest.raises(L.SpeechLLMError, match="beam sampling"):
        llm.generate_packed(x, [4, 4], 4, sample=dict(temperature=1.0, top_k=0, top_p=1.0, seed=0), beams=dict(num_beams=2))
    with pytest.raises(L.SpeechLLMError, match="unknown keys"):
        llm.generate_packed(x, [4, 4], 4, beams=dict(num_beams=2, beam_width=3))
    with pytest.raises(L.SpeechLLMError, match="decode rows"):
        llm.generate_packed(torch.zeros(4 * 300, 256), [4] * 300, 4, beams=dict(num_beams=8))


def test_fixture_holds_the_cases_and_meets_the_gap_condition():
    g = golden("beam_tiny")
    assert list(g["cases"]) == CASES
    for name in CASES:
        assert float(g[f"{name}.min_gap"]) >= 1e-3, name
        K, R, B, n = int(g[f"{name}.K"]), int(g[f"{name}.R"]), int(g[f"{name}.batch"]), len(g[f"{name}.eos"])
        M = beam_ref.n_candidates(K, n)
        assert g[f"{name}.top_val"].shape[1:] == (B * K, M + 4) and g[f"{name}.ids"].shape == (B * R, int(g[f"{name}.max_new"]))
    assert all(v.dtype.kind in "iufbU" for v in g.values())          # data only


@pytest.mark.parametrize("name", CASES)
def test_restatement_replays_the_reference_from_the_stored_top_lists(name):
    g = golden("beam_tiny")
    K, R, B, max_new = (int(g[f"{name}.{k}"]) for k in ("K", "R", "batch", "max_new"))
    ref = beam_ref.BeamRef(B, K, max_new, g[f"{name}.eos"].tolist(), float(g[f"{name}.length_penalty"]), ES[int(g[f"{name}.early_stopping"])],
                           int(g[f"{name}.pad"]))
    val, idx = t(g[f"{name}.top_val"]), t(g[f"{name}.top_idx"]).long()
    for step in range(val.shape[0]):
        assert not ref.all_done()
        ref.step_logprobs(val[step].view(B, K, -1), idx[step].view(B, K, -1))
    assert ref.all_done()
    ids, scores, lens = ref.result(R)
    assert torch.equal(ids.view(B * R, max_new), t(g[f"{name}.ids"]).long())
    assert torch.equal(lens.view(-1), t(g[f"{name}.lens"]).long())
    want = t(g[f"{name}.scores"]).double()
    assert bool(((scores.view(-1).double() - want).abs() <= 1e-4 * want.abs().clamp(min=1.0)).all())
    assert ref.min_gap >= 1e-3
