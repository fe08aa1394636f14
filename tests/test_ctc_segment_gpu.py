"""GPU: the CTC segmentation kernels (sl_ctc_greedy_batch, sl_ctc_pool_ranges_batch) element by element against float64 / the pure-Python
restatement tests/ctc_segment_ref.py, and the feature through the models: CTCSegmenter on the tiny HuBERT with a tiny CTC head, and
`ctc_pool` inference from waveforms alone."""
import numpy as np
import pytest
import torch

import ctc_segment_ref as ref
from conftest import golden, pkg, t
from oracle import hubert_oracle as ho
from oracle.golden_cfgs import TINY_HUBERT, TINY_LLAMA
from test_ctc_segment_host_cpu import fixture_sequences, random_ids
from test_models_gpu import DEV, StubTokenizer, hubert_arch, make_encoder, make_llama

pytestmark = pytest.mark.gpu

L = pkg("_lib")
ops = pkg("ops")
ri = pkg("random_init")
seg_mod = pkg("ctc_segmenter")
inf_mod = pkg("inference")
utils = pkg("utils")

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
ROWS = (1, 63, 64, 65, 257)
GUARD = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------------------------------------
# the head kernel
# ------------------------------------------------------------------------------------------------------------------------------
def planted(rows, H, V, dtype, seed, bias):
    """x[m] = 0.5 w[c_m] + 0.05 noise, rounded to `dtype`: the oracle (float64 on the ROUNDED operands) prefers c_m by about 0.5 |w_c|^2 ~ H / 2"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(V, H, generator=g, dtype=torch.float64).to(dtype)
    b = torch.randn(V, generator=g, dtype=torch.float64).to(dtype) if bias else None
    c = torch.randint(0, V, (rows,), generator=g)
    x = (0.5 * w.double()[c] + 0.05 * torch.randn(rows, H, generator=g, dtype=torch.float64)).to(dtype)
    return x, w, b, c


def oracle_ids(x, w, b):
    """float64 logits of the operands as the kernel gets them -> (argmax, top-2 margin, bound on the kernel's error of a logit difference).
    The operands are already rounded, and a product of two 16-bit (or fp32) values is taken exactly by the MFMA (fp32: rounded once, 2^-24), so what
    the kernel adds is the fp32 accumulation of H products and one bias add: |error of a logit| <= (H + 2) 2^-24 (sum_k |x_k w_vk| + |b_v|), in
    any order of summation; twice the largest such bound of the row covers a difference of two logits."""
    xd, wd = x.double(), w.double()
    logits = xd @ wd.T + (b.double() if b is not None else 0.0)
    mag = xd.abs() @ wd.abs().T + (b.double().abs() if b is not None else 0.0)
    top = torch.topk(logits, min(2, logits.shape[1]), dim=1)
    margin = top.values[:, 0] - top.values[:, 1] if logits.shape[1] > 1 else torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    bound = 2.0 * (x.shape[1] + 2) * 2.0 ** -24 * mag.max(dim=1).values
    return top.indices[:, 0].to(torch.int32), margin, bound


def run_head(x, w, b):
    """-> ids (CPU); the ids buffer sits between guard words, which must come back intact"""
    n = x.shape[0]
    buf = torch.full((n + 16,), GUARD, dtype=torch.int32, device=DEV)
    ops.ctc_greedy(x.to(DEV).contiguous(), w.to(DEV).contiguous(), None if b is None else b.to(DEV).contiguous(), out=buf[8:8 + n])
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:8] == GUARD).all()) and bool((got[8 + n:] == GUARD).all()), "guard words around ids were written"
    return got[8:8 + n]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("V", [5, 32, 64])
@pytest.mark.parametrize("H", [64, 1024])
def test_head_planted_rows_every_frame_compared(dtype, H, V):
    for rows in ROWS:
        for bias in (False, True):
            x, w, b, c = planted(rows, H, V, dtype, seed=rows * 7 + H + V + bias, bias=bias)
            want, margin, bound = oracle_ids(x, w, b)
            assert bool((margin > bound).all()), (rows, float(margin.min()), float(bound.max()))      # a condition on the inputs: no frame is skipped
            assert torch.equal(want.long(), c)                                                        # the planted class is the oracle's
            got = run_head(x, w, b)
            assert torch.equal(got, want), (rows, bias, (got != want).nonzero().flatten().tolist()[:8])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("H,V", [(64, 5), (72, 17), (1024, 32), (1024, 64), (2056, 33)])
def test_head_every_k_position_meets_its_own_weight_column(dtype, H, V):
    """row k is the unit vector e_k, column k of w a permutation of 0 .. V - 1: the logits are exact in every type (one non-zero product each), the
    argmax is where the permutation has V - 1, and a k offset or lane mix-up anywhere in the operand layout moves it.  H = 72 and 2056 are no
    multiples of the MFMA step (the zero-filled tail), 2056 x 33 needs more than one weight chunk in every type."""
    g = torch.Generator().manual_seed(H + V)
    w = torch.stack([torch.randperm(V, generator=g) for _ in range(H)], dim=1).to(dtype)      # (V, H)
    x = torch.eye(H, dtype=dtype)
    want = w.float().argmax(dim=0).to(torch.int32)
    assert torch.equal(run_head(x, w, None), want)
    b = (torch.arange(V, 0, -1) * 0.5).to(dtype)              # halves: the logits stay exact in every type, and exact ties between columns do occur
    logits = w.float() + b.float()[:, None]
    lowest = (logits == logits.max(dim=0).values).float().argmax(dim=0).to(torch.int32)        # the first column that attains the maximum
    assert int((logits == logits.max(dim=0).values).sum()) > H                                 # some k do have a tie
    assert torch.equal(run_head(x, w, b), lowest)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
def test_head_ties_go_to_the_lowest_column(dtype):
    H, V, rows = 256, 48, 130
    x, w, b, c = planted(rows, H, V, dtype, seed=3, bias=True)
    dup = {3: (19, 40), 7: (8,), 16: (47,)}                       # column -> its copies (same weight row, same bias), across and inside 16-column tiles
    for lo, copies in dup.items():
        for hi in copies:
            w[hi], b[hi] = w[lo], b[lo]
    c = torch.tensor([list(dup)[m % 3] if m % 2 else [19, 40, 8, 47][m % 4] for m in range(rows)])
    x = (0.5 * w.double()[c]).to(dtype)
    back = {hi: lo for lo, copies in dup.items() for hi in copies}
    want = torch.tensor([back.get(int(v), int(v)) for v in c], dtype=torch.int32)
    assert torch.equal(run_head(x, w, b), want)
    w[:] = w[0]
    b[:] = b[0]
    assert torch.equal(run_head(x, w, b), torch.zeros(rows, dtype=torch.int32))                 # every column equal: column 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16", "fp32"])
def test_head_ids_follow_their_rows_under_permutation_and_in_another_batch(dtype):
    """unplanted gaussian rows (near-ties included): whatever the kernel answers for a row, it answers it wherever the row sits"""
    g = torch.Generator().manual_seed(9)
    H, V, rows = 1024, 32, 257
    x = torch.randn(rows, H, generator=g).to(dtype)
    w = torch.randn(V, H, generator=g).to(dtype)
    b = torch.randn(V, generator=g).to(dtype)
    ids = run_head(x, w, b)
    perm = torch.randperm(rows, generator=g)
    assert torch.equal(run_head(x[perm], w, b), ids[perm])
    assert torch.equal(run_head(x[100:165], w, b), ids[100:165])
    assert torch.equal(run_head(torch.cat([x[200:], x, x[:3]]), w, b), torch.cat([ids[200:], ids, ids[:3]]))
    # 33 410 rows are 262 slabs of 128 for at most 256 blocks: some blocks walk two slabs; with V = 64 the weight image is re-staged per chunk
    w64, b64 = torch.cat([w, w.flip(0) * 0.5]), torch.cat([b, b.flip(0)])
    ids64 = run_head(x, w64, b64)
    assert torch.equal(run_head(x.to(DEV).repeat(130, 1), w64, b64), ids64.repeat(130))


# ------------------------------------------------------------------------------------------------------------------------------
# the segmentation kernel
# ------------------------------------------------------------------------------------------------------------------------------
B_, D_, A_ = 0, 4, 9            # blank, delimiter, a letter


def hand_made():
    rng = np.random.RandomState(77)
    seqs = {f"random T={T}": random_ids(rng, T, .55, .12) for T in (1, 2, 63, 64, 65, 257, 1500)}
    seqs.update({
        "all blank": [B_] * 70, "all delimiter": [D_] * 70, "one blank": [B_], "one delimiter": [D_], "one letter": [A_],
        "word at frame 0": [A_, A_, 8, B_, D_, B_, B_, 10, 10, B_, B_, B_, B_, B_, B_, B_, B_, B_, B_, B_],            # first gap (0, 0) dropped when packed
        "word ending at T": [B_, B_, D_, 7, 7, B_, 8, 8, 8],                                                          # last chunk clamped, final gap dropped
        "word lengths 3 4 5 8": [B_] + [A_] * 3 + [D_, B_] + [A_] * 4 + [D_] + [A_] * 5 + [D_, D_] + [A_] * 8 + [B_, B_],
        "word longer than a wave": [B_] * 5 + [A_, B_] * 60 + [D_] + [B_] * 9,
        "word over the 64-frame boundary": [B_] * 60 + [A_] * 10 + [D_] + [B_] * 20,
        "word over the 256-frame tile": [D_] * 250 + [A_] * 12 + [D_, B_, 7],
        "word held open by blanks over three tiles": [B_, 7] + [B_] * 700 + [8, B_, D_, B_] + [9] * 3,
        "delimiter at the tile's last frame": [A_] * 255 + [D_] + [A_] * 3,
        "letter at the tile's last frame, closed by the next tile": [B_] * 255 + [A_, D_, A_],
        "T = 255": [A_, D_] * 127 + [A_], "T = 256": [A_, D_] * 128, "alternating 257": [A_, D_] * 128 + [A_],
        "special tokens inside a word": [B_, 1, A_, 2, B_, 3, D_, 3, 3, B_, 1],                                      # <s>, </s>, <unk> count as letters
        "no word": [B_, D_, B_, B_, D_, D_, B_],
        "unknown ids": [31, 63, 1000, -5, D_, 77],
    })
    return seqs


def run_segment(seqs, raw, pool_range=4, blank=B_, delim=D_):
    """one packed batch -> per utterance (ranges, words); guard words after the capacity of both tables and after the counts must stay intact, and so
    must the table rows past the total (the kernel writes what it counts, nothing else)"""
    lib = L.lib()
    n_utt, n_rows = len(seqs), sum(len(s) for s in seqs)
    offs = np.cumsum([0] + [len(s) for s in seqs])
    ids = torch.tensor([v for s in seqs for v in s] or [0], dtype=torch.int32).to(DEV)
    offs_d = torch.tensor(offs, dtype=torch.int64).to(DEV)
    cap, wcap = int(lib.sl_ctc_pool_ranges_capacity(n_rows, n_utt)), int(lib.sl_ctc_words_capacity(n_rows, n_utt))
    table = torch.full((cap + 4, 2), -GUARD, dtype=torch.int64, device=DEV)
    words = torch.full((wcap + 4, 2), -GUARD, dtype=torch.int64, device=DEV)
    counts = torch.full((n_utt + 4,), GUARD, dtype=torch.int32, device=DEV)
    wcounts = torch.full((n_utt + 4,), GUARD, dtype=torch.int32, device=DEV)
    L.check(lib.sl_ctc_pool_ranges_batch(ids.data_ptr(), offs_d.data_ptr(), n_utt, n_rows, blank, delim, pool_range,
                                         L.CTC_RANGES_RAW if raw else L.CTC_RANGES_PACKED, table.data_ptr(), cap, counts.data_ptr(), words.data_ptr(), wcap,
                                         wcounts.data_ptr(), L.stream_ptr()), "sl_ctc_pool_ranges_batch")
    torch.cuda.synchronize()
    table, words, counts, wcounts = table.cpu(), words.cpu(), counts.cpu(), wcounts.cpu()
    assert bool((counts[n_utt:] == GUARD).all()) and bool((wcounts[n_utt:] == GUARD).all()), "guard words after the counts were written"
    cnt, wcnt = counts[:n_utt].tolist(), wcounts[:n_utt].tolist()
    assert bool((table[sum(cnt):] == -GUARD).all()) and bool((words[sum(wcnt):] == -GUARD).all()), "rows past the counted records were written"
    out, r0, w0 = [], 0, 0
    for c_, wc_ in zip(cnt, wcnt):
        out.append(([tuple(r) for r in table[r0:r0 + c_].tolist()], [tuple(w) for w in words[w0:w0 + wc_].tolist()]))
        r0, w0 = r0 + c_, w0 + wc_
    return out, offs.tolist()


def expect_segment(seqs, raw, offs, pool_range=4, blank=B_, delim=D_):
    out = []
    for s, tok0 in zip(seqs, offs):
        w = ref.words(s, blank, delim)
        out.append((ref.raw_ranges(w, len(s), pool_range) if raw else ref.packed_ranges(w, len(s), pool_range, tok0), w))
    return out


@pytest.mark.parametrize("raw", [False, True], ids=["packed", "raw"])
def test_segment_hand_made_sequences_one_by_one_and_as_one_batch(raw):
    cases = hand_made()
    for name, s in cases.items():
        got, offs = run_segment([s], raw)
        assert got == expect_segment([s], raw, offs), name
    seqs = list(cases.values())
    got, offs = run_segment(seqs, raw)
    want = expect_segment(seqs, raw, offs)
    for name, g_, w_ in zip(cases, got, want):
        assert g_ == w_, name
    # spelled out once, so that the restatement is not the only witness
    if not raw:
        got, _ = run_segment([cases["word at frame 0"], cases["word ending at T"]], raw)
        assert got[0][0] == [(0, 4), (3, 7), (7, 11), (9, 17)] and got[0][1] == [(0, 3), (7, 9)]
        assert got[1][0] == [(20, 23), (23, 27), (27, 29)] and got[1][1] == [(3, 9)]                    # rows 20 .. 28: nothing reaches past the utterance
    else:
        got, _ = run_segment([cases["word at frame 0"], cases["word ending at T"], cases["no word"]], raw)
        assert got[0][0] == [(0, 0), (0, 4), (3, 7), (7, 11), (9, 17)]
        assert got[1][0] == [(0, 3), (3, 7), (7, 11), (9, 17)] and got[2] == ([(0, 7)], [])


@pytest.mark.parametrize("raw", [False, True], ids=["packed", "raw"])
@pytest.mark.parametrize("pool_range", [4, 1, 7])
def test_segment_fixture_and_seeded_random_batch(raw, pool_range):
    seqs, blank, delim, pr = fixture_sequences()
    ids = [s[0] for s in seqs]
    got, offs = run_segment(ids, raw, pool_range, blank, delim)
    assert got == expect_segment(ids, raw, offs, pool_range, blank, delim)
    if raw and pool_range == pr:          # the recorded lists themselves: HF's word offsets and the reference's ranges
        for (s_ids, words, ranges), (g_ranges, g_words) in zip(seqs, got):
            n_frames = len(s_ids)
            assert g_words == words and g_ranges == (ranges if words else [(0, n_frames)])
    rng = np.random.RandomState(1 + pool_range)
    rnd = [random_ids(rng, int(rng.randint(1, 400)), *[(.5, .2), (.8, .1), (.1, .1), (0., .5), (.3, 0.)][i % 5], blank=2, delim=30) for i in range(60)]
    got, offs = run_segment(rnd, raw, pool_range, blank=2, delim=30)
    assert got == expect_segment(rnd, raw, offs, pool_range, blank=2, delim=30)
    if not raw:
        table = torch.tensor([r for g_ in got for r in g_[0]], dtype=torch.int64)
        for (rngs, _), tok0, s in zip(got, offs, rnd):
            assert rngs and all(tok0 <= a < b <= tok0 + len(s) for a, b in rngs)                       # non-empty, inside the utterance
        x = torch.randn(offs[-1], 64, generator=torch.Generator().manual_seed(1)).to(DEV)
        y = ops.segment_mean_batch(x, table.to(DEV))                                                    # sl_segment_mean_batch takes the table as it is
        a, b = table[17].tolist()
        assert torch.allclose(y[17].cpu(), x[a:b].mean(dim=0).cpu(), atol=1e-5)


def test_segment_an_utterance_depends_on_its_own_ids_only():
    rng = np.random.RandomState(4)
    seqs = [random_ids(rng, T, .5, .15) for T in (300, 64, 1, 257, 90)]
    base, _ = run_segment(seqs, raw=False)
    for u in range(len(seqs) - 1):                      # rewriting utterance u + 1 leaves utterance u bit-identical, in place (same length) ...
        other = list(seqs)
        other[u + 1] = [A_] * len(seqs[u + 1])
        got, _ = run_segment(other, raw=False)
        assert got[u] == base[u] and got[:u] == base[:u], u
    order = [3, 0, 4, 2, 1]                             # ... and in another order every utterance has the same ranges, relative to its first row
    got, offs = run_segment([seqs[i] for i in order], raw=False)
    _, offs0 = run_segment(seqs, raw=False)
    for pos, i in enumerate(order):
        rel = [(a - offs[pos], b - offs[pos]) for a, b in got[pos][0]]
        assert rel == [(a - offs0[i], b - offs0[i]) for a, b in base[i][0]] and got[pos][1] == base[i][1]
    raw_a, _ = run_segment(seqs, raw=True)
    raw_b, _ = run_segment([seqs[i] for i in order], raw=True)
    assert [raw_b[pos] for pos in range(5)] == [raw_a[i] for i in order]


# ------------------------------------------------------------------------------------------------------------------------------
# through the models
# ------------------------------------------------------------------------------------------------------------------------------
LENS = (9000, 16720, 24000, 16000)          # 27, 52, 74, 49 frames
CTC_SEED, CTC_V = 25, 32


def make_segmenter(dtype):
    sd = ri.hubert_ctc_state_dict(TINY_HUBERT, CTC_V, seed=CTC_SEED)
    return seg_mod.CTCSegmenter(hubert_arch(TINY_HUBERT), DEV, dtype=dtype, state_dict=sd), sd


def oracle_greedy(sd, wave):
    """CPU oracle: HubertModel.last_hidden_state -> Linear -> argmax, with the top-2 margin and the comparison bound per frame.  The fp32 kernels
    track the oracle's hidden state to a relative 1e-4 (the suite's F32_TOL: ~20 chained fp32 GEMM / LayerNorm stages of K <= 256, each good to
    about K 2^-24); by Cauchy-Schwarz a logit then moves by at most 1e-4 |h_t| |w_v|, and a difference of two logits by twice that."""
    h = ho.hubert_forward(sd, TINY_HUBERT, wave[None], prefix="hubert.")[0].double()
    w, b = sd["lm_head.weight"].double(), sd["lm_head.bias"].double()
    logits = h @ w.T + b
    top = torch.topk(logits, 2, dim=1)
    bound = 2.0 * 1e-4 * h.norm(dim=1) * w.norm(dim=1).max()
    return top.indices[:, 0].to(torch.int32), top.values[:, 0] - top.values[:, 1], bound


def test_segmenter_greedy_ids_fp32_against_the_cpu_oracle():
    """Frames whose oracle top-2 margin is within the bound are left out: 0 of the 202 frames of the four utterances with CTC_SEED = 25 (checked on
    the CPU when the seed was chosen; the cap is 5 %), and the classes blank / delimiter / letter all occur among the ids."""
    seg, sd = make_segmenter(torch.float32)
    waves = [ri.synthetic_waveform(n, seed=n) for n in LENS]
    got = [g_.cpu() for g_ in seg.greedy_ids(waves)]
    left_out = total = 0
    for w, g_ in zip(waves, got):
        want, margin, bound = oracle_greedy(sd, w)
        keep = margin > bound
        left_out += int((~keep).sum())
        total += keep.numel()
        assert g_.shape == want.shape and torch.equal(g_[keep], want[keep]), ((g_ != want) & keep).nonzero().flatten().tolist()
    print(f"left out {left_out} of {total} frames")
    assert left_out <= 0.05 * total
    # the lists are those of the restatement on these ids, in every form
    ids = [g_.tolist() for g_ in got]
    words = [ref.words(s, seg.blank_id, seg.delim_id) for s in ids]
    assert seg.word_offsets(waves) == words
    assert seg.pool_ranges(waves, raw=True) == [ref.raw_ranges(w_, len(s)) for w_, s in zip(words, ids)]
    assert seg.pool_ranges(waves) == [ref.packed_ranges(w_, len(s)) for w_, s in zip(words, ids)]
    assert seg.pool_ranges(waves, pool_range=3) == [ref.packed_ranges(w_, len(s), 3) for w_, s in zip(words, ids)]
    table, counts = seg.ranges_packed(waves)
    tok0, flat = 0, []
    for w_, s in zip(words, ids):
        flat += ref.packed_ranges(w_, len(s), 4, tok0)
        tok0 += len(s)
    assert table.is_cuda and table.dtype == torch.int64 and [tuple(r) for r in table.cpu().tolist()] == flat
    assert counts == [len(ref.packed_ranges(w_, len(s))) for w_, s in zip(words, ids)]


def test_segmenter_reads_a_hubert_for_ctc_directory(tmp_path):
    import json
    from safetensors.torch import save_file
    c = TINY_HUBERT
    sd = ri.hubert_ctc_state_dict(c, CTC_V, seed=CTC_SEED)
    (tmp_path / "config.json").write_text(json.dumps(dict(
        model_type="hubert", architectures=["HubertForCTC"], conv_dim=list(c.conv_dim), conv_kernel=list(c.conv_kernel), conv_stride=list(c.conv_stride),
        hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
        num_conv_pos_embeddings=c.num_conv_pos_embeddings, num_conv_pos_embedding_groups=c.num_conv_pos_embedding_groups, layer_norm_eps=c.layer_norm_eps,
        feat_extract_norm="layer", do_stable_layer_norm=True, vocab_size=CTC_V)))
    vocab = ["<s>", "|", "</s>", "<pad>"] + [chr(65 + i) for i in range(CTC_V - 4)]                 # <pad> = 3, | = 1: not the defaults
    (tmp_path / "vocab.json").write_text(json.dumps({tok: i for i, tok in enumerate(vocab)}))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    seg = seg_mod.CTCSegmenter(str(tmp_path), DEV, dtype=torch.float32)
    assert (seg.blank_id, seg.delim_id, seg.vocab_size) == (3, 1, CTC_V)
    mem, _ = make_segmenter(torch.float32)
    assert (mem.blank_id, mem.delim_id) == (0, 4)
    waves = [ri.synthetic_waveform(n, seed=n) for n in LENS[:2]]
    ids = [g_.cpu() for g_ in seg.greedy_ids(waves)]
    assert all(torch.equal(a, b.cpu()) for a, b in zip(ids, mem.greedy_ids(waves)))
    assert seg.word_offsets(waves) == [ref.words(s.tolist(), 3, 1) for s in ids]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ctc_pool_inference_from_waveforms_alone_equals_the_same_call_given_the_lists(dtype):
    g = golden("pipeline_tiny")
    cfg = TINY_LLAMA
    enc, _ = make_encoder(TINY_HUBERT, cfg.hidden_size, int(g["enc_seed"]), dtype, method="ctc_pool")
    llm, _ = make_llama(cfg, int(g["llm_seed"]), dtype)
    seg, _ = make_segmenter(dtype)
    tok = StubTokenizer({utils.LLAMA_PROMPT_PREFIX: t(g["prefix_ids"]), utils.LLAMA_PROMPT_SUFFIX: t(g["suffix_ids"]), "EXTRA": t(g["text_prompt_ids"])})
    inf = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, dtype=dtype, ctc_segmenter=seg)
    waves = [ri.synthetic_waveform(n, seed=n).numpy() for n in LENS]
    texts = ["", "EXTRA", "", ""]
    lists = seg.pool_ranges(waves)
    assert len({len(r) for r in lists}) > 1 and all(r for r in lists)                              # prompts of different lengths
    out = inf.generate_audio_responses(waves, texts, max_new_tokens=16)
    ids = inf.last_generate_ids.cpu()
    out_lists = inf.generate_audio_responses(waves, texts, max_new_tokens=16, ctc_pool_ranges=lists)
    assert out == out_lists and torch.equal(ids, inf.last_generate_ids.cpu()) and ids.shape[0] == 4
    # the name the reference calls: one utterance's list is its entry of the batch
    for i in (0, 2):
        assert inf.get_ctc_pool_ranges(torch.as_tensor(waves[i])[None].to(DEV)) == lists[i]
    # one utterance, no ranges given: the single-utterance entry point derives them, and explicitly given ranges still win
    inf.generate_audio_response(waves[3], max_new_tokens=16)
    alone = inf.last_generate_ids.cpu()[0]
    inf.generate_audio_response(waves[3], max_new_tokens=16, ctc_pool_ranges=lists[3])
    assert torch.equal(alone, inf.last_generate_ids.cpu()[0])
    bare = inf_mod.LLMSpeechTextInference(enc.config, None, DEV, tokenizer=tok, llm=llm, audio_encoder=enc, dtype=dtype)
    for obj in (inf, bare):
        obj.generate_audio_response(waves[3], max_new_tokens=16, ctc_pool_ranges=[(0, 49)])
    assert torch.equal(inf.last_generate_ids.cpu(), bare.last_generate_ids.cpu())
    # without a segmenter nothing changes: the reference's AttributeError
    with pytest.raises(AttributeError, match="get_ctc_pool_ranges"):
        bare.generate_audio_responses(waves, texts, max_new_tokens=16)
    with pytest.raises(AttributeError, match="get_ctc_pool_ranges"):
        bare.generate_audio_response(waves[0], max_new_tokens=16)
