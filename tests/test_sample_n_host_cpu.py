"""CPU (no GPU): several sampled answers per prompt — the host planner of the grouped decode attention's records, every
refusal of sl_generate_n / sl_attn_decode_grouped reported before any launch, the N = 1 workspace size, the Python keywords, and the
ctypes mirrors against the header."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import REPO, pkg

L = pkg("_lib")
ops = pkg("ops")
cfgm = pkg("config")

NEW_EXPORTS = {"sl_attn_group_plan_host", "sl_attn_decode_grouped_workspace_bytes", "sl_attn_decode_grouped", "sl_generate_workspace_bytes_n",
               "sl_generate_n", "sl_generate_last_attn_path"}


# ------------------------------------------------------------------------------------------------ the planner
def _interleaved():
    """(slot, len) = (0, 9) x 7, (1, 21) x 1, (2, 0) x 2, interleaved -> rows of each kind"""
    kinds = [0, 2, 0, 0, 1, 0, 0, 2, 0, 0]
    slot = [k for k in kinds]
    plen = [{0: 9, 1: 21, 2: 0}[k] for k in kinds]
    return kinds, slot, plen


def test_plan_groups_rows_by_slot_and_length_in_row_order():
    kinds, slot, plen = _interleaved()
    recs, n_used, raw = ops.attn_group_plan(slot, plen, rep=3)        # floor(16 / 3) = 5 rows per record
    assert len(recs) == len(kinds) == 10                              # B records are always written
    assert n_used == 3
    used, unused = recs[:n_used], recs[n_used:]
    assert all(r == (0, 0, []) for r in unused)
    assert all(int(r.reserved) == 0 for r in raw)
    a = [i for i, k in enumerate(kinds) if k == 0]
    by_key = {}
    for s, p, rows in used:
        assert rows == sorted(rows) and len(rows) >= 1
        by_key.setdefault((s, p), []).append(rows)
    assert by_key == {(0, 9): [a[:5], a[5:]], (1, 21): [[4]]}         # 5 + 2 rows, and 1 row; the len-0 rows (1, 7) are in no record
    assert not any(r in rows for _, _, rows in used for r in (1, 7))


def test_plan_rep_1_takes_16_rows_per_record_and_rep_4_takes_4():
    recs, n_used, _ = ops.attn_group_plan([3] * 19, [40] * 19, rep=1)
    assert n_used == 2 and [len(r[2]) for r in recs[:2]] == [16, 3] and recs[0][2] == list(range(16)) and recs[1][:2] == (3, 40)
    recs, n_used, _ = ops.attn_group_plan([0] * 9, [5] * 9, rep=4)
    assert n_used == 3 and [len(r[2]) for r in recs[:3]] == [4, 4, 1]
    # same slot, another length: another group
    recs, n_used, _ = ops.attn_group_plan([0, 0, 0], [5, 6, 5], rep=2)
    assert n_used == 2 and recs[0] == (0, 5, [0, 2]) and recs[1] == (0, 6, [1])


def test_plan_refuses_bad_arguments():
    lib = L.lib()
    one = (C.c_int32 * 1)(0)
    rec = (L.AttnGroup * 1)()
    n = C.c_int32(0)
    assert lib.sl_attn_group_plan_host(one, one, 1, 0, rec, C.byref(n)) == -1 and b"rep" in lib.sl_last_error()
    assert lib.sl_attn_group_plan_host(one, one, 1, 17, rec, C.byref(n)) == -1 and b"rep" in lib.sl_last_error()
    assert lib.sl_attn_group_plan_host(one, one, 0, 2, rec, C.byref(n)) == -1 and b"B" in lib.sl_last_error()
    assert lib.sl_attn_group_plan_host(None, one, 1, 2, rec, C.byref(n)) == -1 and b"prefix_slot" in lib.sl_last_error()
    assert lib.sl_attn_group_plan_host(one, one, 1, 2, rec, None) == -1 and b"n_used" in lib.sl_last_error()


# ------------------------------------------------------------------------------------------------ refusals, before any HIP call
def _model(dtype=L.SL_F32, reserved=0, fake_pointers=True):
    m = L.LlamaModel()
    m.dtype, m.hidden, m.n_layers, m.n_heads, m.n_kv_heads, m.head_dim, m.ffn, m.vocab = dtype, 256, 2, 2, 2, 128, 384, 1000
    m.rope_len, m.reserved = 64, reserved
    if fake_pointers:      # pass the null checks; every refusal below comes before anything is dereferenced on the device
        for f in ("layers", "embed", "lm_head", "final_norm", "rope_cos", "rope_sin"):
            setattr(m, f, C.cast(1, type(getattr(m, f))) if f == "layers" else 1)
    return m


def _kv(slots=64, max_ctx=48):
    kv = L.KVCache()
    kv.slots, kv.max_ctx = slots, max_ctx
    kv.k_cache = kv.v_cache = 1
    return kv


def _opts(sample=1, max_new=8):
    o = L.GenerateOpts()
    o.max_new_tokens, o.check_every, o.sample, o.temperature, o.top_k, o.top_p = max_new, 4, sample, 1.0, 0, 1.0
    return o


@pytest.mark.parametrize("what,N,nseq,sample,slots,rc,needle", [
    ("N = 0", 0, 2, 1, 64, -1, b"num_return_sequences"),
    ("N = -3", -3, 2, 1, 64, -1, b"num_return_sequences"),
    ("greedy with N = 2", 2, 2, 0, 64, -1, b"sample"),
    ("nseq * N > SL_MAX_DECODE_BATCH", 8, 257, 1, 4096, -1, b"decode rows"),
    ("slots < nseq * (N + 1)", 3, 4, 1, 15, -1, b"kv->slots"),
])
def test_generate_n_refusals_are_reported_without_a_gpu(what, N, nseq, sample, slots, rc, needle):
    lib = L.lib()
    m, kv, o = _model(), _kv(slots=slots), _opts(sample=sample)
    cu = (C.c_int32 * (nseq + 1))(*[10 * i for i in range(nseq + 1)])
    got = lib.sl_generate_n(C.byref(m), C.byref(kv), 1, cu, nseq, C.byref(o), None, None, 1, 1 << 40, None, None, None, N)
    assert got == rc and needle in lib.sl_last_error(), (what, got, lib.sl_last_error())


def test_generate_n_accepts_exactly_nseq_times_n_plus_1_slots_as_far_as_the_next_check():
    """slots = nseq * (N + 1) passes the slot check: the call goes on to the next refusal (a null output buffer)"""
    lib = L.lib()
    m, kv, o = _model(), _kv(slots=16), _opts()
    cu = (C.c_int32 * 5)(0, 10, 20, 30, 40)
    got = lib.sl_generate_n(C.byref(m), C.byref(kv), 1, cu, 4, C.byref(o), None, None, 1, 1 << 40, None, None, None, 3)
    assert got == -1 and b"kv->slots" not in lib.sl_last_error() and b"bad arguments" in lib.sl_last_error(), lib.sl_last_error()


def test_e4m3_decode_weight_row_limit_counts_nseq_times_n():
    lib = L.lib()
    rows = lib.sl_w8_max_rows()
    N = 8
    nseq = rows // N + 1                                    # nseq alone is within the e4m3 range, nseq * N is not
    assert nseq <= rows < nseq * N
    m, kv, o = _model(dtype=L.SL_BF16, reserved=L.WDEC_E4M3), _kv(slots=2048), _opts(max_new=4)
    m.dec_fused_norm = 1
    m.lm_head_dec = 1
    layers = (L.LlamaLayer * 2)()
    for lay in layers:
        for f, _ in L.LlamaLayer._fields_:
            setattr(lay, f, 1)
    m.layers = layers
    cu = (C.c_int32 * (nseq + 1))(*[4 * i for i in range(nseq + 1)])
    ids = (C.c_int32 * (nseq * N * 4))()
    args = (C.byref(m), C.byref(kv), 1, cu, nseq, C.byref(o), ids, None, 1, 1 << 40, None, None, None)
    rc = lib.sl_generate_n(*args, N)
    assert rc == -3 and b"sl_w8_max_rows" in lib.sl_last_error(), (rc, lib.sl_last_error())


@pytest.mark.parametrize("what,kw,rc,needle", [
    ("float32", dict(dtype=L.SL_F32), -3, b"float32"),
    ("D = 64", dict(D=64), -1, b"head_dim"),
    ("REP 5", dict(nh=10, nkv=2), -3, b"n_heads/n_kv"),
    ("REP 8", dict(nh=8, nkv=1), -3, b"n_heads/n_kv"),
    ("n_heads % n_kv", dict(nh=5, nkv=2), -1, b"n_heads"),
    ("format 2", dict(fmt=2), -1, b"format"),
    ("e4m3 with D = 64", dict(fmt=L.KV_FP8_E4M3, D=64), -3, b"head_dim"),
    ("B = 0", dict(B=0), -1, b"B"),
    ("row_slot0 < 0", dict(slot0=-1), -1, b"row_slot0"),
    ("null groups", dict(groups=None), -1, b"groups_dev"),
])
def test_attn_decode_grouped_refusals_are_reported_without_a_gpu(what, kw, rc, needle):
    lib = L.lib()
    a = dict(dtype=L.SL_BF16, D=128, nh=4, nkv=2, fmt=L.KV_MODEL_DTYPE, B=3, slot0=2, groups=1)
    a.update(kw)
    got = lib.sl_attn_decode_grouped(1, 512, 1, 1, 1, 1, 1, 1, a["groups"], a["B"], a["slot0"], a["nh"], a["nkv"], a["D"], 64, 0.1, a["dtype"], a["fmt"], None)
    assert got == rc and needle in lib.sl_last_error(), (what, got, lib.sl_last_error())


def test_workspace_bytes():
    lib = L.lib()
    m = _model()
    lp = L.LogitsOpts()
    lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens = 1.3, 2, 0
    for n_tok, nseq, max_new, lpr, sc in [(40, 2, 8, None, 0), (300, 7, 24, C.byref(lp), 1), (9, 1, 1, None, 1)]:
        base = lib.sl_generate_workspace_bytes_sc(C.byref(m), n_tok, nseq, max_new, lpr, sc)
        assert base > 0 and lib.sl_generate_workspace_bytes_n(C.byref(m), n_tok, nseq, max_new, lpr, sc, 1) == base
        # N > 1: at least the per-row pieces of nseq * N rows, the records and one staged logits row per prompt
        n3 = lib.sl_generate_workspace_bytes_n(C.byref(m), n_tok, nseq, max_new, lpr, sc, 3)
        assert n3 >= lib.sl_generate_workspace_bytes_sc(C.byref(m), n_tok, 3 * nseq, max_new, lpr, sc) + 3 * nseq * C.sizeof(L.AttnGroup) + \
            lib.sl_attn_decode_grouped_workspace_bytes(3 * nseq, m.n_heads) + nseq * m.vocab * 4
    assert lib.sl_generate_workspace_bytes_n(C.byref(m), 40, 2, 8, None, 0, 0) == 0 and b"num_return_sequences" in lib.sl_last_error()
    assert lib.sl_generate_workspace_bytes_n(C.byref(m), 40, 600, 8, None, 0, 4) == 0
    assert lib.sl_attn_decode_grouped_workspace_bytes(7, 6) >= 7 * 6 * 130 * 4
    assert lib.sl_attn_decode_grouped_workspace_bytes(0, 6) == 0


# ------------------------------------------------------------------------------------------------ header, mirrors, Python keywords
def test_header_declares_the_new_entries_and_the_abi_stays_7():
    hdr = open(os.path.join(REPO, "include", "speechllm.h")).read()
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", hdr))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(L.EXPORTS)
    assert L.lib().sl_version() == 7


def _c_args(decl):
    """argument list of a C declaration -> coarse kinds: 'p' pointer, 'i32', 'i64', 'f32', 'sz'"""
    inner = decl[decl.index("(") + 1:decl.rindex(")")]
    kinds = []
    for a in [x.strip() for x in inner.split(",")]:
        if a == "void":
            continue
        if "*" in a or a.startswith("sl_stream"):
            kinds.append("p")
        elif a.startswith("int64_t"):
            kinds.append("i64")
        elif a.startswith("int32_t"):
            kinds.append("i32")
        elif a.startswith("float"):
            kinds.append("f32")
        elif a.startswith("size_t"):
            kinds.append("sz")
        else:
            raise AssertionError(a)
    return kinds


def _ctypes_kind(t_):
    if t_ in (C.c_int32,):
        return "i32"
    if t_ is C.c_int64:
        return "i64"
    if t_ is C.c_float:
        return "f32"
    if t_ is C.c_size_t:
        return "sz"
    return "p"


def test_lib_binds_every_new_symbol_with_the_headers_signature():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "speechllm.h")).read(), flags=re.S)
    for name in sorted(NEW_EXPORTS):
        decl = re.search(r"(size_t|int32_t|int)\s+" + name + r"\s*\([^;]*\)\s*;", hdr)
        assert decl, name
        res, args = L._PROTOS[name]
        assert [_ctypes_kind(a) for a in args] == _c_args(decl.group(0)), name
        assert {"size_t": C.c_size_t, "int": C.c_int32, "int32_t": C.c_int32}[decl.group(1)] is res, name
        assert getattr(L.lib(), name).argtypes == args


def test_attn_group_mirror_matches_the_c_header(tmp_path):
    assert C.sizeof(L.AttnGroup) == 80 and L.AttnGroup.rows.offset == 16
    if shutil.which("gcc") is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "speechllm.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(sl_attn_group));']
    for fname, _ in L.AttnGroup._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(sl_attn_group, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.AttnGroup)
    for fname, _ in L.AttnGroup._fields_:
        assert int(out[fname]) == getattr(L.AttnGroup, fname).offset, fname


def _tiny_llm():
    from oracle.golden_cfgs import TINY_MHA as c
    weights, ri, llama_mod = pkg("weights"), pkg("random_init"), pkg("audio_llama")
    arch = weights.LlamaArch(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim, c.intermediate_size,
                             c.vocab_size, c.rms_norm_eps, c.rope_theta, c.rope_scaling, c.tie_word_embeddings, tuple(c.eos_token_ids), c.pad_token_id)
    return llama_mod.AudioLlamaForCausalLM(arch, dict(ri.llama_state_dict(c, seed=1)), torch_dtype=torch.float32, device="cpu", max_ctx=64)


def test_python_keywords():
    llm = _tiny_llm()
    x = torch.zeros(1, 4, 256)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):          # greedy with R = 2, as HF refuses it
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_return_sequences=2)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_return_sequences=0, do_sample=True)
    with pytest.raises(L.SpeechLLMError, match="GPU"):        # sampling with R = 2 is honoured, so without a device the call fails loudly
        llm.generate(inputs_embeds=x, max_new_tokens=4, num_return_sequences=2, do_sample=True)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):
        llm.generate_packed(torch.zeros(4, 256), [4], 4, num_return=2)
    with pytest.raises(L.SpeechLLMError, match="num_return_sequences"):
        llm.generate_packed(torch.zeros(4, 256), [4], 4, num_return=0)


def test_runtime_num_return_sequences_parsing():
    assert cfgm.runtime_num_return(cfgm.from_dict(dict(model=dict()))) == 1
    assert cfgm.runtime_num_return(cfgm.from_dict(dict(runtime=dict(num_return_sequences=4)))) == 4
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="num_return_sequences"):
            cfgm.runtime_num_return(cfgm.from_dict(dict(runtime=dict(num_return_sequences=bad))))
