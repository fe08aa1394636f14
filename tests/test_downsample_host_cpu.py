"""No GPU: the host side of the stack / ctc_pool downsampling — the new C exports, the argument checks of sl_hubert_forward_ds and of the four
kernels' entry points (all answered before any launch), the range clamping (sl_segment_ranges_host) and the inverse index frame -> covering
ranges (sl_segment_csr_host) against a brute-force inverse, and the refusals of the training tape that need no device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO, pkg
from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA

L = pkg("_lib")
ops = pkg("ops")
cfgm = pkg("config")
weights = pkg("weights")
enc_mod = pkg("audio_encoder")
training = pkg("training")

NEW_EXPORTS = {"sl_segment_mean_batch", "sl_segment_mean_bwd_batch", "sl_stack_rows_batch", "sl_stack_rows_bwd_batch", "sl_segment_ranges_host",
               "sl_segment_csr_host", "sl_hubert_workspace_bytes_ds", "sl_hubert_forward_ds"}
SL_ERR_ARG = -1


def test_new_symbols_are_declared_exported_and_additive():
    hdr = open(os.path.join(REPO, "include", "speechllm.h")).read()
    declared = set(re.findall(r"\b(sl_[a-z0-9_]+)\s*\(", hdr))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(L.EXPORTS)
    lib = C.CDLL(L.LIB_PATH)
    for name in sorted(NEW_EXPORTS):
        assert hasattr(lib, name), name
    assert L.lib().sl_version() == 7          # additive: no ABI bump


def test_downsample_descriptor_mirror_matches_the_header(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(REPO, "include", "speechllm.h")}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(sl_downsample_desc));']
    lines += [f'  printf("{n} %zu\\n", offsetof(sl_downsample_desc, {n}));' for n, _ in L.DownsampleDesc._fields_]
    lines += ['  printf("codes %d %d %d\\n", SL_DS_POOL, SL_DS_STACK, SL_DS_CTC_POOL);', '  return 0;', '}']
    (tmp_path / "ds.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "ds"), str(tmp_path / "ds.c")], check=True, capture_output=True)
    out = [l.split() for l in subprocess.run([str(tmp_path / "ds")], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert int(out[0][1]) == C.sizeof(L.DownsampleDesc)
    for (name, off), (fname, _) in zip(out[1:-1], L.DownsampleDesc._fields_):
        assert name == fname and int(off) == getattr(L.DownsampleDesc, fname).offset, name
    assert [int(v) for v in out[-1][1:]] == [L.DS_POOL, L.DS_STACK, L.DS_CTC_POOL]


def _model(hidden=1024, llm_dim=3072):
    m = L.HubertModel()
    m.dtype, m.n_conv, m.hidden, m.n_layers, m.n_heads, m.ffn, m.pos_k, m.pos_groups = L.SL_BF16, 7, hidden, 2, hidden // 64, 4 * hidden, 128, 16
    for i, (c, k, s) in enumerate(zip([512] * 7, [10, 3, 3, 3, 3, 2, 2], [5, 2, 2, 2, 2, 2, 2])):
        m.conv_dim[i], m.conv_kernel[i], m.conv_stride[i] = c, k, s
    m.ln_eps, m.pool_kernel, m.pool_stride, m.llm_dim = 1e-5, 1, 1, llm_dim
    return m


def test_forward_ds_argument_checks_come_back_as_sl_err_arg_without_a_device():
    lib = L.lib()
    m = _model()
    offs = (C.c_int64 * 3)(0, 16000, 48000)
    buf = (C.c_char * 256)()
    p = C.cast(buf, C.c_void_p)

    def call(ds):
        return lib.sl_hubert_forward_ds(C.byref(m), p, offs, 2, p, 3072, None, None, None if ds is None else C.byref(ds), p, 256, None)

    def expect(ds, *words):
        assert call(ds) == SL_ERR_ARG
        msg = lib.sl_last_error().decode()
        assert all(w in msg for w in words), msg
        if ds is not None:
            assert lib.sl_hubert_workspace_bytes_ds(C.byref(m), offs, 2, C.byref(ds)) == 0      # the workspace query refuses the same descriptors

    def stack():
        ds = L.DownsampleDesc()
        ds.method, ds.factor, ds.proj_in, ds.proj_w, ds.proj_b = L.DS_STACK, 4, 4 * 1024, p, p
        return ds

    expect(None, "descriptor")
    ds = stack(); ds.factor = 0
    expect(ds, "factor")
    ds = stack(); ds.proj_in = 1024                                         # a projection that is not f * H wide
    expect(ds, "stack", "4 x 1024")
    ds = stack(); ds.proj_w = None
    expect(ds, "projection")
    ds = stack(); ds.method = 7
    expect(ds, "method")
    ds = stack(); ds.method = L.DS_POOL                                     # pool keeps its own entry point
    expect(ds, "sl_hubert_forward")
    counts = (C.c_int32 * 2)(3, 2)

    def ctc():
        ds = L.DownsampleDesc()
        ds.method, ds.factor, ds.proj_in, ds.proj_w, ds.proj_b = L.DS_CTC_POOL, 4, 1024, p, p
        ds.n_ranges, ds.ranges_dev, ds.range_counts_host = 5, p, counts
        return ds

    ds = ctc(); ds.ranges_dev = None
    expect(ds, "null range table")
    ds = ctc(); ds.range_counts_host = None
    expect(ds, "null range table")
    ds = ctc(); ds.n_ranges = 6                                            # the counts add up to 5
    expect(ds, "add up to 5", "holds 6")
    ds = ctc(); ds.proj_in = 4096
    expect(ds, "ctc_pool", "4096")
    # well-formed descriptors: the workspace query answers, the forward gets as far as the workspace check (still no launch)
    for ds in (stack(), ctc()):
        need = lib.sl_hubert_workspace_bytes_ds(C.byref(m), offs, 2, C.byref(ds))
        assert need > 0
        assert call(ds) == SL_ERR_ARG and "workspace" in lib.sl_last_error().decode()
    many = ctc()
    big = (C.c_int32 * 2)(1000, 1000)
    many.range_counts_host, many.n_ranges = big, 2000                       # more ranges than frames: the range means get their own room
    assert lib.sl_hubert_workspace_bytes_ds(C.byref(m), offs, 2, C.byref(many)) > lib.sl_hubert_workspace_bytes_ds(C.byref(m), offs, 2, C.byref(ctc()))


def test_kernel_entry_points_check_their_arguments_before_launching():
    lib = L.lib()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.sl_segment_mean_batch(p, p, None, 4, 100, 128, L.SL_BF16, None) == SL_ERR_ARG               # null table
    assert lib.sl_segment_mean_batch(p, p, p, 4, 100, 130, L.SL_BF16, None) == SL_ERR_ARG                  # H not a multiple of 8
    assert lib.sl_segment_mean_batch(p, p, p, 4, 100, 6, L.SL_F32, None) == SL_ERR_ARG                     # ... of 4 in fp32
    assert lib.sl_segment_mean_batch(p, p, p, 0, 100, 128, L.SL_F16, None) == 0                            # no ranges: nothing to do
    assert lib.sl_segment_mean_bwd_batch(p, p, p, None, p, 4, 100, 128, L.SL_BF16, None) == SL_ERR_ARG     # no index
    assert lib.sl_segment_mean_bwd_batch(p, p, p, p, p, 4, 100, 132, L.SL_F16, None) == SL_ERR_ARG
    assert lib.sl_stack_rows_batch(p, p, p, 2, 10, 128, 0, L.SL_BF16, None) == SL_ERR_ARG                  # factor < 1
    assert b"factor" in lib.sl_last_error()
    assert lib.sl_stack_rows_batch(p, p, None, 2, 10, 128, 4, L.SL_BF16, None) == SL_ERR_ARG
    assert lib.sl_stack_rows_batch(p, p, p, 2, 0, 128, 4, L.SL_BF16, None) == 0                            # every utterance shorter than one row
    assert lib.sl_stack_rows_bwd_batch(p, p, p, 2, 10, 128, 0, L.SL_BF16, None) == SL_ERR_ARG
    assert lib.sl_stack_rows_bwd_batch(p, p, p, 2, 10, 130, 4, L.SL_F16, None) == SL_ERR_ARG
    assert lib.sl_stack_rows_bwd_batch(p, p, p, 2, 10, 128, 4, 9, None) == SL_ERR_ARG                      # unknown dtype


# ------------------------------------------------------------------------------------------------------------------------------
# range tables
# ------------------------------------------------------------------------------------------------------------------------------
def word_pool_ranges(words, chunk=4):
    """The ranges the reference's preprocessing derives from CTC word offsets (its get_hubert_ctc_pool_ranges, restated): the silence before the
    first word, then for every word consecutive chunks of `chunk` frames from its start until its end is covered (the last chunk may run past the
    word's end into what follows), the gap up to the next word as ONE range, and 2 * chunk frames after the last word."""
    out = [(0, words[0][0])]
    for i, (start, end) in enumerate(words):
        out += [(s, s + chunk) for s in range(start, end, chunk)]
        out.append((end, words[i + 1][0]) if i + 1 < len(words) else (end, end + 2 * chunk))
    return out


def brute_force_inverse(packed, n_rows):
    """frame -> the ranges covering it, in table order"""
    return [[r for r, (s, e) in enumerate(packed) if s <= t < e] for t in range(n_rows)]


WORDS = [(3, 9), (12, 14), (20, 31), (33, 40)]        # hand-made (start_offset, end_offset) frames of four words
TABLES = {
    "reference recipe": ([word_pool_ranges(WORDS)], [45]),      # the closing (40, 48) runs past the 45 frames and is clamped
    "unsorted": ([[(30, 40), (0, 4), (10, 12), (4, 10)]], [49]),
    "repeated": ([[(5, 9), (5, 9), (5, 9), (0, 49)]], [49]),
    "gaps": ([[(2, 3), (10, 20), (40, 41)]], [49]),
    "ends past T": ([[(40, 60), (48, 1000), (0, 49)], [(0, 9)]], [49, 5]),
    "three utterances": ([word_pool_ranges(WORDS), [(0, 1)], [(-4, 200), (1, 3)]], [49, 1, 7]),
}


def test_reference_recipe_yields_overlapping_ranges():
    r = word_pool_ranges(WORDS)
    assert r[:4] == [(0, 3), (3, 7), (7, 11), (9, 12)]                  # the word's last chunk (7, 11) runs into the gap (9, 12) that follows
    assert r[-1] == (40, 48) and (28, 32) in r and (31, 33) in r


@pytest.mark.parametrize("name", list(TABLES))
def test_csr_index_equals_brute_force_inverse(name):
    ranges, T = TABLES[name]
    packed, counts = ops.segment_ranges_pack(ranges, T)
    assert counts == [len(r) for r in ranges]
    # clamping as a tensor slice clamps, then the utterance's first packed row
    want, row0 = [], 0
    for r, t_ in zip(ranges, T):
        for s, e in r:
            idx = torch.arange(t_)[s:e]
            want.append([row0 + int(idx[0]), row0 + int(idx[-1]) + 1])
        row0 += t_
    assert packed.tolist() == want
    n_rows = sum(T)
    row_ptr, cols = ops.segment_csr(packed, n_rows)
    inv = brute_force_inverse(packed.tolist(), n_rows)
    assert row_ptr.dtype == torch.int64 and cols.dtype == torch.int32 and row_ptr.tolist()[0] == 0
    assert [cols[row_ptr[t]:row_ptr[t + 1]].tolist() for t in range(n_rows)] == inv
    assert int(row_ptr[-1]) == sum(e - s for s, e in packed.tolist())


def test_csr_builder_refuses_tables_that_leave_the_packed_rows():
    lib = L.lib()
    row_ptr = torch.empty(11, dtype=torch.int64)
    for bad_range in ([[2, 11]], [[-1, 3]], [[4, 4]], [[6, 5]]):
        r = torch.tensor(bad_range, dtype=torch.int64)
        assert lib.sl_segment_csr_host(r.data_ptr(), 1, 10, row_ptr.data_ptr(), None, 0) == SL_ERR_ARG, bad_range
    r = torch.tensor([[0, 10]], dtype=torch.int64)
    cols = torch.empty(4, dtype=torch.int32)
    assert lib.sl_segment_csr_host(r.data_ptr(), 1, 10, row_ptr.data_ptr(), cols.data_ptr(), 4) == SL_ERR_ARG        # cols too small for 10 entries


@pytest.mark.parametrize("ranges,T,utt,rng", [([[(0, 4)], [(0, 2), (5, 9)]], [49, 5], "utterance 1", "range 1 (5, 9)"),
                                              ([[(3, 3)]], [49], "utterance 0", "range 0 (3, 3)"),
                                              ([[(0, 1)], [(0, 1)], [(4, 2)]], [5, 5, 5], "utterance 2", "range 0 (4, 2)"),
                                              ([[(60, 70)]], [49], "utterance 0", "range 0 (60, 70)")])
def test_a_range_that_is_empty_after_clamping_is_refused_by_name(ranges, T, utt, rng):
    with pytest.raises(L.SpeechLLMError) as e:
        ops.segment_ranges_pack(ranges, T)
    assert utt in str(e.value) and rng in str(e.value) and "empty" in str(e.value)


def test_ranges_must_come_one_list_per_utterance():
    with pytest.raises(L.SpeechLLMError):
        ops.segment_ranges_pack([[(0, 1)]], [5, 5])
    with pytest.raises(L.SpeechLLMError):
        ops.segment_ranges_pack(None, [5])


# ------------------------------------------------------------------------------------------------------------------------------
# the training tape
# ------------------------------------------------------------------------------------------------------------------------------
def cpu_encoder(method):
    c = TINY_HUBERT
    conf = cfgm.from_dict(dict(model=dict(audio_encoder=dict(base="hubert", type="synthetic", downsample_method=method, downsample_factor=4,
                                                             pooling=dict(kernel_size=8, stride=4)),
                                          llm_embedding_channels=TINY_LLAMA.hidden_size, llm_type="meta-llama/Llama-3.2-3B-Instruct")))
    arch = weights.HubertArch(c.conv_dim, c.conv_kernel, c.conv_stride, c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size,
                              c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, c.layer_norm_eps)
    return enc_mod.AudioEncoder(conf, "cpu", dtype=torch.float32, arch=arch)


@pytest.mark.parametrize("method", ["stack", "ctc_pool"])
def test_encoder_tape_accepts_the_two_methods(method):
    tape = training.EncoderTape(cpu_encoder(method))
    assert tape.enc.downsample_method == method


def test_whisper_tape_keeps_its_refusal():
    stub = SimpleNamespace(downsample_method="stack")
    with pytest.raises(L.SpeechLLMError, match="the KD step is built for the `pool` downsample"):
        training.WhisperEncoderTape(stub)


def test_ctc_pool_without_ranges_is_refused_before_any_launch():
    enc = cpu_encoder("ctc_pool")              # no weights, no device: anything past the check would fail differently
    wave = torch.zeros(16000)
    with pytest.raises(L.SpeechLLMError, match="pool_ranges"):
        training.EncoderTape(enc).forward([wave])
    kd = SimpleNamespace(enc=enc, llm=None)
    ids = torch.arange(4)
    for ranges in (None, [None], [[(0, 4)], [(0, 4)]]):        # missing, a sample without the column, one list too many
        with pytest.raises(L.SpeechLLMError, match="micro_batch needs pool_ranges"):
            training.KDTrainer.micro_batch(kd, [wave], [ids], [ids], pool_ranges=ranges)
    for method in ("pool", "stack"):                           # ... and ranges handed to a method that would ignore them are refused too
        kd = SimpleNamespace(enc=cpu_encoder(method), llm=None)
        with pytest.raises(L.SpeechLLMError, match="ctc_pool downsample only"):
            training.KDTrainer.micro_batch(kd, [wave], [ids], [ids], pool_ranges=[[(0, 4)]])
    with pytest.raises(L.SpeechLLMError, match="ctc_pool_ranges"):      # the inference-side entry: checked after the weights, so give it some
        enc.weights = SimpleNamespace(struct=None, fold_stale=False)
        enc.encode_packed([wave])
