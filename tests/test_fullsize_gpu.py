"""GPU parity at the sizes BASELINE.json's configs name (Spark-TTS-0.5B shape, synthetic weights), on the paths the
bench actually runs: the prefill GEMM (k_pgemm) at 32 x 128 and 8 x ~460 prompt rows, free-running bf16-KV + hipGraph
decode through the vocoder (north_star's acceptance sentence: fp32 waveform within 1e-3 of the CPU path for fixed greedy
seeds), and the 32-row padded vocoder batch.  Oracle: oracle/llm_ref.py (pinned to transformers), oracle/bicodec_ref.py
(pinned to the reference's modules), tests/golden/llm_full.npz (transformers' own tokens)."""
import os

import numpy as np
import pytest
import torch

from conftest import FULL_MAX_POS

pytestmark = pytest.mark.gpu


TIE_GAPS = []   # gaps of the accepted flips of this session (printed by the tests that bound their number)
TIE = 2e-2   # logit gap (logit std ~1.6) below which two summation orders may pick different tokens once K/V are rounded to bf16


def _llm(cfg, arena, **kw):
    from sparkmi.llm import SparkLLM
    return SparkLLM(cfg, None, "cuda:0", max_positions=FULL_MAX_POS, arena=arena, **kw)


def _assert_same_or_tie(probe, prompt, got, want, what):
    """`got` and `want` are two valid runs of one sequence (two kernels with different fp32 summation orders, or kernel vs
    CPU oracle).  With an f32 KV cache they must be identical.  With a bf16 cache an fp32 last-bit difference in a K/V
    element can move it to the neighbouring bf16 value (2^-9 relative), which may flip a NEAR-TIE arg-max; every later
    token then differs legitimately.  So: identical, or the first difference sits on a tie -- both tokens are the top two
    of the teacher-forced logits there and less than TIE apart.  Returns True when the runs were identical."""
    if got == want:
        return True
    i = next(k for k in range(min(len(got), len(want))) if got[k] != want[k])
    lg = probe.forward_logits(list(prompt) + list(want[:i]))[-1].float().cpu()
    top = torch.topk(lg, 2)
    assert {int(top.indices[0]), int(top.indices[1])} == {got[i], want[i]}, f"{what}: token {i} differs and is not a top-2 tie: {got[i]} vs {want[i]}, top {top.indices.tolist()}"
    gap = float(top.values[0] - top.values[1])
    assert gap < TIE, f"{what}: token {i} differs at a logit gap of {gap}"
    TIE_GAPS.append(gap)
    return False


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_config3_prompts_through_the_prefill_gemm(full_llm, golden_dir, kv):
    """configs[2]'s prefill: 32 prompts x 128 tokens = 4064 prompt rows -> k_pgemm in its many-row shapes (o_proj / down_proj
    summed in K segments inside the block).  Every row's tokens equal its own B = 1 run -- 127 rows: the same family in its
    few-row shapes (64-column tiles, one block per K segment + in-order combine), the same sums in the same order -- with
    EITHER cache type: the kernels a sequence's prompt runs through are chosen from its own length, so its K/V rows do not
    depend on what else the call holds (round 3 chose from the call's total rows: 27 of 32 rows survived the bf16 cache).
    Row 0 is the golden prompt and equals transformers' greedy tokens (f32 KV, like the golden)."""
    cfg, syn, arena = full_llm
    g = np.load(os.path.join(golden_dir, "llm_full.npz"))
    rng = np.random.Generator(np.random.PCG64(2024))
    prompts = [g["prompt"].tolist()] + [rng.integers(0, cfg.vocab_size, size=128).tolist() for _ in range(31)]
    assert sum(len(p) - 1 for p in prompts) >= 3072      # the k_pgemm threshold (SPARKMI_PGEMM_MIN_ROWS default)
    n = 12
    big = _llm(cfg, arena, max_slots=32, kv_dtype=kv)
    one = _llm(cfg, arena, max_slots=1, kv_dtype=kv)
    batched = big.generate_ids(prompts, n)
    for b in range(32):
        assert one.generate_ids([prompts[b]], n)[0] == batched[b], f"row {b} ({kv} KV): batch of 32 vs alone"
    if kv == "f32":
        assert batched[0] == g["greedy"][:n].tolist()


def test_a_sequence_does_not_depend_on_its_batch_with_the_bf16_cache(full_llm, monkeypatch):
    """Prompts of very different lengths in ONE call (3 .. 700 tokens: decode-kernel chunks for the short ones, the prefill GEMM
    family in its few-row or many-row shapes for the others, by each sequence's own length) against every sequence alone, bf16
    KV cache (the production setting): tokens equal, and the K rows of layer 0 / the last layer equal bit for bit.  Then the
    two forms of the segmented o_proj / down_proj sum against each other on one prompt (SPARKMI_PG_SPLIT_ROWS=0 keeps the
    in-block form at any row count)."""
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(777))
    lens = [3, 40, 65, 66, 67, 128, 130, 200, 333, 600, 17, 96]
    prompts = [rng.integers(0, cfg.vocab_size, size=L).tolist() for L in lens]
    n = 8
    mk = lambda slots: SparkLLM(cfg, None, "cuda:0", max_slots=slots, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16", diag=True)  # noqa: E731
    big = mk(len(lens))
    batched = big.generate_ids(prompts, n)
    kv_big = {b: [big.debug_get_kv(layer, b, 0, lens[b])[0] for layer in (0, cfg.num_hidden_layers - 1)] for b in range(len(lens))}
    one = mk(1)
    for b in range(len(lens)):
        assert one.generate_ids([prompts[b]], n)[0] == batched[b], f"prompt of {lens[b]} tokens: in the batch vs alone"
        for i, layer in enumerate((0, cfg.num_hidden_layers - 1)):
            assert np.array_equal(one.debug_get_kv(layer, 0, 0, lens[b])[0], kv_big[b][i]), f"{lens[b]} tokens, layer {layer}: K rows differ"
    monkeypatch.setenv("SPARKMI_PG_SPLIT_ROWS", "0")
    inblock = mk(1)
    for b in (4, 7, 9):
        assert inblock.generate_ids([prompts[b]], n)[0] == batched[b]
        assert np.array_equal(inblock.debug_get_kv(cfg.num_hidden_layers - 1, 0, 0, lens[b])[0], kv_big[b][1]), "split-K vs in-block segments"


@pytest.mark.parametrize("B", [2, 8])
def test_fused_o_proj_with_the_last_arriver_head_sum_keeps_the_bits(full_llm, monkeypatch, B):
    """The diagnostics build's opt-in form for 2 .. 8 live rows (SPARKMI_FUSE2_ROWS; measured slower than the separate o_proj launch
    and off by default, DESIGN 3.9 -- kept because it is the in-launch hand-off the review asked to be measured, and correct):
    the attention kernel also computes the o_proj and the LAST of a (row, quarter)'s 14 head blocks to arrive
    adds the heads in order and finishes the rows (k_attn<.., FUSE = 2>: sc1 partial stores, an agent-scope arrival count, sc1
    reads).  120 free-running steps of ragged contexts (uneven load: the rows' contexts differ by hundreds of tokens, so their
    head blocks finish at different times) must give the tokens -- and, teacher-forced, the residual rows -- of the separate o_proj
    kernel (SPARKMI_FUSE2_ROWS=0) bit for bit, and every row must equal its own one-row run."""
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(88 + B))
    lens = [int(v) for v in rng.integers(5, 400, size=B)]
    prompts = [rng.integers(0, cfg.vocab_size, size=L).tolist() for L in lens]
    n = 120
    mk = lambda slots: SparkLLM(cfg, None, "cuda:0", max_slots=slots, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16", diag=True)  # noqa: E731
    monkeypatch.setenv("SPARKMI_FUSE2_ROWS", "8")
    fused = mk(B)
    got = fused.generate_ids(prompts, n)
    h_fused = fused.debug_hidden()
    again = fused.generate_ids(prompts, n)            # second utterance on the same captured graphs: the counters were left at zero
    assert again == got
    monkeypatch.delenv("SPARKMI_FUSE2_ROWS")
    plain = mk(B)
    assert plain.generate_ids(prompts, n) == got
    assert np.array_equal(plain.debug_hidden(), h_fused)
    one = mk(1)
    for b in range(B):
        assert one.generate_ids([prompts[b]], n)[0] == got[b], f"row {b} of {B}"


def test_config3_ragged_batch_with_rows_retired_equals_the_padded_batch(full_llm):
    """What `bench.py --batch 32` runs (configs[2] / [3]): 32 ragged prompts (97..154 ids), per-row token budgets, rows retired on
    the device as they reach their budget (`SparkLLM.generate_ragged`: admit through the session path, cached step graph per
    live-row count, `smi_llm_retire_many`).  Every row's tokens are those of the padded static batch truncated to its budget
    -- bit for bit: rows are independent in every kernel and both paths prefill the same 4000-odd rows through k_pgemm."""
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(3030))
    prompts = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(97, 155))).tolist() for _ in range(32)]
    budgets = [int(v) for v in rng.integers(6, 23, size=32)]
    llm = _llm(cfg, arena, max_slots=32, kv_dtype="bf16")
    static = llm.generate_ids(prompts, max(budgets))
    ragged = llm.generate_ragged(prompts, budgets)
    assert ragged == [t[:n] for t, n in zip(static, budgets)]
    assert llm.generate_ragged(prompts, budgets) == ragged          # second call: every step graph comes from the cache


def test_paged_kv_cache_at_full_size_equals_contiguous_cache_and_oracle(full_llm, full_llm_oracle):
    """SURVEY 8f-4 at the 0.5B shape (the functional analogue of TensorRT-LLM's paged KV, runtime/triton_trtllm/run.sh:50-65):
    32 ragged prompts on a paged engine (64-token pages: the page size must divide max_positions = 704) give the tokens of
    the contiguous-cache engine bit for bit -- both prefill the same rows through the same kernels, only the K/V addresses
    differ -- and two rows equal the CPU oracle (f32 KV: exactly; that run is the pin, bf16 adds only the documented ties).
    The paged step's time goes to profiles/ through tools/serve_time.py."""
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(4096))
    prompts = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(97, 155))).tolist() for _ in range(32)]
    n = 10
    for kv in ("f32", "bf16"):
        paged = _llm(cfg, arena, max_slots=32, kv_dtype=kv, kv_page_tokens=64, kv_pages=104)
        flat = _llm(cfg, arena, max_slots=32, kv_dtype=kv)
        got = paged.generate_ids(prompts, n)
        assert got == flat.generate_ids(prompts, n), f"paged vs contiguous ({kv})"
        tot, free = paged.kv_pages()
        assert tot == 104 and 8 <= free <= 40            # every row holds 2-3 pages of 64 tokens, far less than the 11 a reserved slot would
        ref = full_llm_oracle
        ref.kv_dtype = kv
        for b in (3, 17):
            want = ref.generate_greedy(prompts[b], n)
            if kv == "f32":
                assert got[b] == want, f"row {b} vs oracle"
            else:
                _assert_same_or_tie(flat, prompts[b], got[b], want, f"row {b} vs oracle")
        # one sequence alone on the paged engine (the one-row kernels through the page table: k_attn<.., ONE, FUSE, PG = 1> with the
        # fused o_proj) = its row of the batch = the contiguous engine's one-row run -- with either cache type: a sequence's
        # kernels are chosen from its own length, so even the bf16 cache leaves no room for a difference
        assert paged.generate_ids([prompts[5]], n)[0] == got[5], f"paged one-row run ({kv})"
        assert _llm(cfg, arena, max_slots=1, kv_dtype=kv).generate_ids([prompts[5]], n)[0] == got[5], f"contiguous one-row run ({kv})"


def test_config5_clone_length_prompts_through_the_prefill_gemm(full_llm, full_llm_oracle):
    """configs[4]'s prefill shape: 8 voice-clone prompts of ~460 tokens (text + 32 global + ~300 semantic prompt tokens)
    = 3672+ rows -> k_pgemm with ragged lengths; every row equals its B = 1 run and two rows equal the CPU oracle."""
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(460))
    lens = [460, 441, 478, 452, 469, 447, 473, 458]
    prompts = [rng.integers(0, cfg.vocab_size, size=L).tolist() for L in lens]
    assert sum(L - 1 for L in lens) >= 3072
    n = 10
    for kv in ("f32", "bf16"):
        batched = _llm(cfg, arena, max_slots=8, kv_dtype=kv).generate_ids(prompts, n)
        one = _llm(cfg, arena, max_slots=1, kv_dtype=kv)
        for b in range(8):
            assert one.generate_ids([prompts[b]], n)[0] == batched[b], f"row {b} ({kv} KV): batch of 8 vs alone"
        ref = full_llm_oracle
        ref.kv_dtype = kv
        for b in (0, 6):
            want = ref.generate_greedy(prompts[b], n)
            if kv == "f32":
                assert want == batched[b], f"row {b} vs oracle"
            else:
                _assert_same_or_tie(one, prompts[b], batched[b], want, f"row {b} vs oracle")


def test_config2_free_running_bf16_kv_graph_to_waveform(full_llm, full_llm_oracle, full_voc, golden_dir):
    """configs[1] exactly as the bench runs it -- bf16 KV cache, decode step replayed as a hipGraph, 128-token prompt,
    150 free-running greedy tokens -> 150 frames -> 48 000 samples -- against the CPU path end to end
    (cli/SparkTTS.py:197-234): tokens equal the oracle's (bf16-KV emulation), waveform within north_star's 1e-3."""
    from oracle.bicodec_ref import BiCodecDetokRef
    from sparkmi.bicodec import BiCodecVocoder
    cfg, syn, arena = full_llm
    vcfg, sd, folded = full_voc
    g = np.load(os.path.join(golden_dir, "llm_full.npz"))
    prompt = g["prompt"].tolist()
    llm = _llm(cfg, arena, max_slots=1, kv_dtype="bf16", use_graph=True)
    toks = llm.generate_ids([prompt], 150)[0]
    again = llm.generate_ids([prompt], 150)[0]            # second utterance on the SAME captured graph
    assert toks == again and len(toks) == 150
    ref = full_llm_oracle
    ref.kv_dtype = "bf16"
    want = ref.generate_greedy(prompt, 150)
    if not _assert_same_or_tie(llm, prompt, toks, want, "bf16-KV free-running vs oracle"):
        # a near-tie was decided the other way: the waveform check below then runs on the GPU's own tokens
        # (both sequences are valid greedy runs); the teacher-forced agreement pins the rest of the sequence
        seq = list(prompt) + list(want[:-1])
        tf = llm.forward_logits(seq)[len(prompt) - 1:].argmax(-1).cpu().tolist()
        assert np.mean(np.array(tf) == np.array(want)) > 0.97
    glob = np.random.Generator(np.random.PCG64(1235)).integers(0, 4096, size=(1, 1, vcfg.spk_token_num))
    sem = torch.tensor([[t % vcfg.codebook_size for t in toks]])
    voc = BiCodecVocoder(vcfg, sd, "cuda:0", max_batch=1, max_frames=160)
    wav = voc.detokenize(sem, torch.from_numpy(glob)).cpu().numpy()
    owav = BiCodecDetokRef(vcfg, folded).detokenize(sem, torch.from_numpy(glob)).numpy()
    assert wav.shape == owav.shape == (1, 1, 48000)
    err = float(np.abs(wav - owav).max())
    assert err < 1e-3, f"waveform max |diff| {err}"       # north_star
    assert err < 3e-4, f"waveform max |diff| {err}"       # what exact-product fp32 accumulation gives


@pytest.mark.parametrize("exact", [False, True])
def test_config3_vocoder_batch_of_32_ragged_rows(full_voc, exact):
    """configs[2]'s vocoder call: 32 rows of 120..180 frames, padded to the longest (another launch plan than B <= 2:
    tile width, channel split and three-wave blocks are chosen from (B, longest row)).  Every row equals its own
    un-padded run to fp32 re-association and three rows equal the CPU oracle."""
    from oracle.bicodec_ref import BiCodecDetokRef
    from sparkmi.bicodec import BiCodecVocoder
    vcfg, sd, folded = full_voc
    rng = np.random.Generator(np.random.PCG64(3232))
    lens = [int(x) for x in rng.integers(120, 181, size=32)]
    lens[5], lens[17] = 180, 120
    B, T = 32, max(lens)
    sem = rng.integers(0, vcfg.codebook_size, size=(B, T))
    glob = rng.integers(0, 4096, size=(B, 1, vcfg.spk_token_num))
    # exact: every contraction on the exact-fp32 matrix pipe -- a row differs from its un-padded run by fp32 re-association
    # only (another tiling of the same sums).  Default (bf16-split pipe): the re-associated low bits also move hi / mid
    # roundings of later layers' operands, so the two runs differ at the size of the split itself (5e-5 on the waveform).
    row_tol = 2e-5 if exact else 1e-4
    voc = BiCodecVocoder(vcfg, sd, "cuda:0", max_batch=B, max_frames=T, exact_fp32=exact)
    wav = voc.detokenize(torch.from_numpy(sem), torch.from_numpy(glob), lengths=lens).cpu().numpy()
    again = voc.detokenize(torch.from_numpy(sem), torch.from_numpy(glob), lengths=lens).cpu().numpy()
    assert np.array_equal(wav, again)
    one = BiCodecVocoder(vcfg, None, "cuda:0", max_batch=1, max_frames=T, arena=voc.arena, exact_fp32=exact)   # the arena layout does not depend on the batch
    hop = vcfg.hop
    for b, n in enumerate(lens):
        assert not wav[b, 0, n * hop:].any(), f"row {b}: samples behind its own length"
        solo = one.detokenize(torch.from_numpy(sem[b:b + 1, :n]), torch.from_numpy(glob[b:b + 1])).cpu().numpy()
        d = float(np.abs(wav[b, 0, : n * hop] - solo[0, 0]).max())
        assert d < row_tol, f"row {b} ({n} frames) differs from its un-padded run by {d}"
    ref = BiCodecDetokRef(vcfg, folded)
    for b in (5, 17, 30):
        n = lens[b]
        o = ref.detokenize(torch.from_numpy(sem[b:b + 1, :n]), torch.from_numpy(glob[b:b + 1])).numpy()
        d = float(np.abs(wav[b, 0, : n * hop] - o[0, 0]).max())
        assert d < 3e-4, f"row {b} vs oracle: {d}"


def test_teacher_forced_logits_at_every_position_against_the_oracle(full_llm, full_llm_oracle, golden_dir):
    """forward_logits over a 160-token sequence (the golden prompt + 32 of its greedy tokens: 64-row chunks, 64 / 64 / 32 rows)
    against the fp32 oracle at EVERY position, f32 KV: all four m-tiles of the step's 64-row kernels and both 32-row k_lm32 passes
    over the 166 000-entry vocabulary are compared, not just the last row.  Per position: the oracle's top-64 logits within
    LOGIT_ATOL and the row's |logit| sum within 1e-4 of the oracle's (as the golden test does for the last position)."""
    from test_llm_gpu import LOGIT_ATOL
    cfg, syn, arena = full_llm
    g = np.load(os.path.join(golden_dir, "llm_full.npz"))
    seq = np.concatenate([g["prompt"], g["greedy"][:32]])
    got = _llm(cfg, arena, kv_dtype="f32").forward_logits(seq).cpu().numpy()
    ref = full_llm_oracle
    ref.kv_dtype = "f32"
    ref.reset()
    want = ref.forward(seq).numpy()
    ref.reset()
    assert got.shape == want.shape == (160, cfg.vocab_size)
    top = np.argpartition(-want, 64, axis=1)[:, :64]
    err = np.abs(np.take_along_axis(got, top, 1) - np.take_along_axis(want, top, 1)).max(axis=1)
    bad = np.nonzero(err >= LOGIT_ATOL)[0]
    assert bad.size == 0, f"positions {bad.tolist()[:16]}: top-64 logits off by up to {err.max():.3e}"
    sg, sw = np.abs(got.astype(np.float64)).sum(1), np.abs(want.astype(np.float64)).sum(1)
    rel = np.abs(sg - sw) / sw
    assert rel.max() < 1e-4, f"position {int(rel.argmax())}: |logit| sum off by {rel.max():.2e}"


_SESSION_CHILD = r"""
import json, sys
import numpy as np
from sparkmi import config as C, weights as W
from sparkmi.llm import SparkLLM
# the 0.5B layer widths (hidden 896, intermediate 4864: k_downC<10, .>; 14 / 2 heads), two layers and a small vocabulary
cfg = C.LLMConfig(vocab_size=4096, num_hidden_layers=2)
llm = SparkLLM(cfg, W.SyntheticLLM(cfg), "cuda:0", max_slots=64, max_positions=128, kv_dtype="bf16", use_graph=True)
rng = np.random.Generator(np.random.PCG64(3535))
llm.session_begin()
prompts, tokens, live, most = [], {}, {}, 0         # live: slot -> sequence index
for group in range(12):
    n = int(rng.integers(4, 8))                      # at most 7 prompts of at most 5 tokens: under 35 prompt rows per admission
    new = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(2, 6))).tolist() for _ in range(n)]
    if len(live) + n > 56:
        break
    for slot, p in zip(llm.admit(new), new):
        live[slot] = len(prompts)
        prompts.append(p)
    llm.decode(3)                                    # a step graph per live-row count: captured as the rows grow past 35
    most = max(most, len(live))
    if group % 3 == 2:                               # a few sequences leave: their tokens first, then their rows
        leave = list(live)[:2]
        for slot, (t, _) in zip(leave, llm.slots_tokens(leave, 128)):
            tokens[live.pop(slot)] = t
        llm.retire_many(leave)
llm.decode(6)
most = max(most, len(live))
for slot, (t, _) in zip(list(live), llm.slots_tokens(list(live), 128)):
    tokens[live[slot]] = t
llm.close()
one = SparkLLM(cfg, None, "cuda:0", max_slots=1, max_positions=128, kv_dtype="bf16", use_graph=True, arena=llm.arena)
differ = [i for i in range(len(prompts)) if one.generate_ids([prompts[i]], len(tokens[i]))[0] != tokens[i]]
print(json.dumps({"sequences": len(prompts), "most_live": most, "differ": differ}))
"""


def test_captured_decode_steps_past_35_live_rows_in_a_fresh_process():
    """A decode step of 35+ live rows at the 0.5B layer widths launches k_downC<10, 4> with more than 64 KiB of LDS; the kernel
    must be opted in to that window before ITS FIRST LAUNCH in the process, which in a session whose admissions are all small is
    a captured decode step.  A fresh child process (nothing ran before in it; one attempt, no retry) admits groups of under 35
    prompt rows, decodes between them and retires a few rows, until more than 40 rows are live; then every sequence, run
    alone, must give its session tokens."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "spark-tts_amd")]))
    r = subprocess.run([sys.executable, "-c", _SESSION_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert 40 <= out["most_live"] <= 64 and out["sequences"] >= 45, out
    assert out["differ"] == [], f"sequences whose session tokens differ from their solo run: {out['differ']}"


def _group_case(cfg, arena, prompts, kv, n=4):
    """Every sequence of one call against its solo run: tokens, and the K and V rows of layer 0 and of the last layer (prompt and
    generated positions), bit for bit."""
    from sparkmi.llm import SparkLLM
    mk = lambda slots: SparkLLM(cfg, None, "cuda:0", max_slots=slots, max_positions=FULL_MAX_POS, arena=arena, kv_dtype=kv, diag=True)  # noqa: E731
    layers = (0, cfg.num_hidden_layers - 1)
    big = mk(len(prompts))
    batched = big.generate_ids(prompts, n)
    kv_big = {b: [big.debug_get_kv(layer, b, 0, len(p) + n - 1) for layer in layers] for b, p in enumerate(prompts)}
    big.close()
    one = mk(1)
    for b, p in enumerate(prompts):
        assert one.generate_ids([p], n)[0] == batched[b], f"sequence {b} ({len(p)} tokens, {kv} KV): tokens in the call vs alone"
        for i, layer in enumerate(layers):
            k, v = one.debug_get_kv(layer, 0, 0, len(p) + n - 1)
            assert np.array_equal(k, kv_big[b][i][0]), f"sequence {b} ({kv} KV), layer {layer}: K rows differ from its solo run"
            assert np.array_equal(v, kv_big[b][i][1]), f"sequence {b} ({kv} KV), layer {layer}: V rows differ from its solo run"


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("count", [6, 7])
def test_prefill_pass_beyond_one_4096_row_group(full_llm, kv, count):
    """Prompts of 690 tokens (689 rows each, the prefill GEMM family) whose pass exceeds one 4096-row group: 6 prompts (4134 rows:
    the 6th straddles row 4096 at its own position 651, no multiple of 16, and its 38-row tail is a group of its own) and 7 (4823
    rows: the tail group holds 727 rows).  Each sequence's tokens and K / V rows equal its solo run's (include/sparkmi.h: a
    sequence's K/V rows and tokens do not depend on the rest of the call)."""
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(690 + count))
    prompts = [rng.integers(0, cfg.vocab_size, size=690).tolist() for _ in range(count)]
    assert sum(len(p) - 1 for p in prompts) > 4096
    _group_case(cfg, arena, prompts, kv)


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("lens", [(257, 257), (257, 258)], ids=["512rows", "513rows"])
def test_prefill_pass_at_the_few_row_boundary(full_llm, kv, lens):
    """Two prompts of the prefill GEMM family whose pass holds 512 rows (kPgSplitRows: the few-row shapes and split-K o_proj /
    down_proj) or 513 (the many-row shapes); alone each takes the few-row shapes.  Tokens and K / V rows equal the solo runs'."""
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(sum(lens)))
    prompts = [rng.integers(0, cfg.vocab_size, size=L).tolist() for L in lens]
    _group_case(cfg, arena, prompts, kv)
