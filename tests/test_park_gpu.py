"""Park and resume (smi_llm_slots_save / smi_llm_slots_restore; SparkLLM.save_slots / restore_slots / park): a sequence leaves its
KV slot as a snapshot in caller-owned device memory and comes back into another slot with not one bit changed.  Everything
compared here is an integer or raw bits: tokens, counts, finished flags, log-probability bit patterns, blob bytes."""
import ctypes as C

import numpy as np
import pytest

from sparkmi import _lib, config as CFG, weights as W

pytestmark = pytest.mark.gpu

MAX_POS = 160
PAGE = 16
LENS = (3, 17, 70)   # 70 prompt rows: the prefill-GEMM class (more than SMI_MAX_ROWS rows)
STEPS = 30
EINVAL, ENOMEM, ESTATE = -1, -3, -4
KINDS = [("bf16", False), ("bf16", True), ("f32", False), ("f32", True)]


@pytest.fixture(scope="module")
def tiny():
    cfg = CFG.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


_LLMS = {}


def _llm(tiny, kv="bf16", paged=False):
    """One handle per cache kind for the whole module (every test starts its own session)."""
    from sparkmi.llm import SparkLLM
    if (kv, paged) not in _LLMS:
        cfg, syn = tiny
        kw = dict(kv_page_tokens=PAGE, kv_pages=6 * MAX_POS // PAGE) if paged else {}
        _LLMS[(kv, paged)] = SparkLLM(cfg, syn, "cuda:0", max_slots=6, max_positions=MAX_POS, kv_dtype=kv, **kw)
    llm = _LLMS[(kv, paged)]
    llm.set_sampling(False)
    return llm


def _prompts(cfg, seed=3, lens=LENS):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, cfg.vocab_size, size=n).tolist() for n in lens]


def _state(llm, slots):
    """[(tokens, finished)] and the status counts of the listed slots."""
    cnt, fin = llm.status()
    return llm.slots_tokens(slots, MAX_POS), [int(cnt[s]) for s in slots], [int(fin[s]) for s in slots]


def _run(llm, prompts, sampling=None, steps=STEPS, park=None, eos=None, n_return=None, filler=None, lp=False):
    """A session over `prompts`; park = (j, k, gap): output sequence j is parked after k decode steps and restored `gap` steps
    later -- into another slot when `filler` (an unrelated prompt admitted meanwhile, which takes the freed slot) is given --
    and catches up at the end, so every sequence has run `steps` steps.  Returns (per sequence (tokens, finished), log-probs)."""
    llm.session_begin(eos)
    cur = llm.admit(prompts, sampling, n_return)
    n = len(cur)

    def read(idx):
        toks = llm.slots_tokens([cur[i] for i in idx], MAX_POS)
        lps = [llm.slots_logprobs([cur[i]], MAX_POS)[0] if lp and sampling and sampling[i] and sampling[i].get("return_log_probs")
               else None for i in idx]
        return dict(zip(idx, toks)), dict(zip(idx, lps))

    def leave(slots):   # every page is back in the pool once the last sequence has left
        llm.retire_many(slots)
        tot, free = llm.kv_pages()
        assert tot == free, "page accounting"

    if park is None:
        llm.decode(steps)
        t, l = read(list(range(n)))
        leave(cur)
        return [t[i] for i in range(n)], [l[i] for i in range(n)]
    j, k, gap = park
    llm.decode(k)
    old = cur[j]
    blob = llm.park([old])
    extra = llm.admit([filler]) if filler is not None else []
    llm.decode(gap)
    [cur[j]] = llm.restore_slots(blob)
    if filler is not None:
        assert extra == [old] and cur[j] != old, "the snapshot lands in another slot"
    llm.decode(steps - k - gap)
    others = [i for i in range(n) if i != j]
    t, l = read(others)
    llm.retire_many([cur[i] for i in others] + extra)
    llm.decode(gap)
    tj, lj = read([j])
    t.update(tj); l.update(lj)
    leave([cur[j]])
    return [t[i] for i in range(n)], [l[i] for i in range(n)]


def _same(a, b):
    assert a[0] == b[0], "tokens / finished flags differ"
    for x, y in zip(a[1], b[1]):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "log-probability bits differ"


# ------------------------------------------------------------------ snapshot = original
@pytest.mark.parametrize("kv,paged", KINDS)
def test_snapshot_continues_as_its_original(tiny, kv, paged):
    """(sequence, decode steps before the save): count 1 (straight after the admission), count 2, mid-run; with 16-token pages
    the cache length (prompt + count) straddles a page boundary (17 + 1, 70 + 13), ends exactly on one (3 + 13 = 16) and starts
    a page (3 + 14)."""
    cfg, _ = tiny
    llm = _llm(tiny, kv, paged)
    prompts = _prompts(cfg)
    other = _prompts(cfg, seed=11, lens=(9,))[0]
    for s, k in ((1, 0), (0, 1), (0, 12), (0, 13), (2, 12)):
        llm.session_begin(None)
        slots = llm.admit(prompts)
        llm.decode(k)
        nbytes = llm.slot_blob_bytes(slots[s])
        [blob] = llm.save_slots([slots[s]])
        assert blob.numel() == nbytes and blob.dtype.is_floating_point is False
        llm.decode(STEPS - k)
        orig, ocnt, ofin = _state(llm, [slots[s]])
        victim = slots[(s + 1) % 3]
        llm.retire_many([victim])
        assert llm.admit([other]) == [victim]
        [back] = llm.restore_slots([blob])
        assert back not in slots, "another slot, another row position"
        llm.decode(STEPS - k)
        got, gcnt, gfin = _state(llm, [back])
        assert got == orig and gcnt == ocnt == [STEPS + 1] and gfin == ofin, (s, k)
        # both go on with the same stream: the original, still live, has moved on by the same tokens and more
        now = llm.slots_tokens([slots[s]], MAX_POS)[0][0]
        assert now[: STEPS + 1] == orig[0][0] and len(now) == 2 * STEPS - k + 1


def test_blob_size_formula(tiny):
    """smi_llm_slot_blob_bytes against the layout of include/sparkmi.h restated: header, K/V of the written positions, history,
    and only the parts whose feature the sequence uses."""
    cfg, _ = tiny
    llm = _llm(tiny, "bf16", False)
    llm32 = _llm(tiny, "f32", True)
    prompts = _prompts(cfg)
    up16 = lambda n: (n + 15) // 16 * 16
    samp = [None, dict(repetition_penalty=1.3, no_repeat_ngram_size=3), dict(return_log_probs=True, stop_sequences=[[5, 6]])]
    for h, esz in ((llm, 2), (llm32, 4)):
        h.session_begin(None)
        slots = h.admit(prompts, samp)
        h.decode(9)
        sizes = [h.slot_blob_bytes(s) for s in slots]
        pos_bytes = cfg.num_hidden_layers * 2 * cfg.num_key_value_heads * 64 * esz
        body = [(n + 9) * pos_bytes + up16(10 * 8) for n in LENS]       # len - 1 = prompt + 9 positions written, 10 tokens
        hdr = 320                                                        # the documented header (sparkmi.h)
        assert sizes[0] == hdr + body[0]
        assert sizes[1] == hdr + body[1] + up16(cfg.vocab_size * 2) + up16(LENS[1] * 4)   # penalty history row, prompt ids
        assert sizes[2] == hdr + 1616 + body[2] + up16(10 * 4)                             # bias / stop record, log-probabilities
        h.decode(3)
        assert h.slot_blob_bytes(slots[0]) == sizes[0] + 3 * pos_bytes + up16(13 * 8) - up16(10 * 8)


# ------------------------------------------------------------------ park + resume = uninterrupted
@pytest.mark.parametrize("kv,paged", KINDS)
def test_park_and_resume_equals_uninterrupted(tiny, kv, paged):
    cfg, _ = tiny
    llm = _llm(tiny, kv, paged)
    prompts = _prompts(cfg)
    filler = _prompts(cfg, seed=12, lens=(6,))[0]
    want = _run(llm, prompts)
    for j, k in ((2, 4), (0, 12)):
        _same(_run(llm, prompts, park=(j, k, 5), filler=filler), want)
        _same(_run(llm, prompts, park=(j, k, 5)), want)     # back into the slot it left


def test_context_segment_boundary(tiny):
    """The decode attention splits the context into segments of kAttnSeg = 1024 keys (smi_llm.hip: segs_for): 1025 positions is
    the smallest context with two.  A 1010-token prompt is parked at 1017 positions and resumed to run across the boundary."""
    from sparkmi.llm import SparkLLM
    cfg, syn = tiny
    llm = SparkLLM(cfg, syn, "cuda:0", max_slots=3, max_positions=1088, kv_page_tokens=PAGE, kv_pages=3 * 1088 // PAGE)
    prompts = _prompts(cfg, seed=5, lens=(1010, 5))
    want = _run(llm, prompts, steps=40)
    assert len(want[0][0][0]) == 41 and 1010 + 41 > 1025
    _same(_run(llm, prompts, steps=40, park=(0, 6, 5), filler=[7, 8, 9]), want)
    llm.close()


def test_sampling_streams_survive(tiny):
    """Handle sampling (the seedless case: the stream is keyed by the admission number, which the blob must carry) and a
    per-request seed."""
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    filler = _prompts(cfg, seed=12, lens=(6,))[0]
    llm.set_sampling(True, 0.9, 40, 0.95, 4321)
    want = _run(llm, prompts)
    llm.set_sampling(True, 0.9, 40, 0.95, 4321)
    _same(_run(llm, prompts, park=(1, 3, 5), filler=filler), want)
    llm.set_sampling(False)
    greedy = _run(llm, prompts)
    assert greedy[0][1] != want[0][1], "sampling changed nothing"
    samp = [None, None, dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.9, seed=99)]
    want = _run(llm, prompts, samp)
    assert want[0][2] != greedy[0][2] and want[0][0] == greedy[0][0]
    _same(_run(llm, prompts, samp, park=(2, 7, 5), filler=filler), want)


@pytest.mark.parametrize("vocab", [1003, 1008])   # the penalty history row moves as u16 elements / as 16-byte pieces
def test_penalties_and_min_new_tokens(vocab):
    from sparkmi.llm import SparkLLM
    cfg = CFG.tiny_llm(vocab_size=vocab)
    llm = SparkLLM(cfg, W.SyntheticLLM(cfg), "cuda:0", max_slots=6, max_positions=MAX_POS, kv_page_tokens=PAGE, kv_pages=60)
    prompts = _prompts(cfg)
    plain = _run(llm, prompts)
    eos = [plain[0][1][0][4]]            # what sequence 1 emits fifth would stop it; min_new_tokens reaches across the park
    samp = [None, dict(repetition_penalty=1.4, presence_penalty=0.3, frequency_penalty=0.2, min_new_tokens=14), None]
    want = _run(llm, prompts, samp, eos=eos)
    assert want[0][1] != _run(llm, prompts, None, eos=eos)[0][1]
    filler = _prompts(cfg, seed=12, lens=(6,))[0]
    _same(_run(llm, prompts, samp, eos=eos, park=(1, 6, 5), filler=filler), want)
    llm.close()


def test_log_probabilities(tiny):
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    samp = [dict(return_log_probs=True), None, None]
    want = _run(llm, prompts, samp, lp=True)
    assert want[1][0] is not None and len(want[1][0]) == STEPS + 1
    got = _run(llm, prompts, samp, lp=True, park=(0, 8, 5), filler=[1, 2, 3, 4])
    _same(got, want)
    assert np.isfinite(got[1][0]).all()   # entries from before and from after the park


def test_allowed_token_ids_restricted_lm_head(tiny):
    """Every live row constrained: the restricted lm_head runs after the restore too (the union's tile list is rebuilt)."""
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    samp = [dict(allowed_token_ids=list(range(100, 180))), dict(allowed_token_ids=list(range(400, 470)) + [7]),
            dict(allowed_token_ids=list(range(150, 300)))]
    want = _run(llm, prompts, samp)
    assert all(100 <= t < 180 for t in want[0][0][0])
    _same(_run(llm, prompts, samp, park=(1, 5, 5)), want)
    _same(_run(llm, prompts, samp, park=(0, 9, 5), filler=prompts[1][:5]), want)


def test_bias_and_stop_straddle_the_park(tiny):
    """The sequence is parked right after emitting a = its token k.  A bias entry (a, X) completes, and a stop sequence (a, X)
    matches, on the first token after the restore: their prefix is in the history the blob carries."""
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    plain = _run(llm, prompts)[0][1][0]
    k = next(i for i in range(3, 20) if plain[i] not in plain[:i] and plain[i] not in prompts[1])
    a = plain[k]
    X = next(x for x in range(cfg.vocab_size) if x not in plain and x != a)
    samp = [None, dict(sequence_bias=[([a, X], 100.0)], stop_sequences=[[a, X]]), None]
    want = _run(llm, prompts, samp)
    toks, fin = want[0][1]
    assert toks[: k + 1] == plain[: k + 1] and toks[k + 1] == X and fin and len(toks) == k + 2
    got = _run(llm, prompts, samp, park=(1, k, 5), filler=[9, 8, 7])
    _same(got, want)


def test_no_repeat_ngram(tiny):
    """The banned n-gram's first occurrence starts in the prompt, and the ban first bites on the token emitted right after the
    restore: the prompt ids (pctx) and the history both have to come back.  The prompt is searched for among a few candidates
    (few distinct ids, so the tied-embedding model repeats them): A = tokens without the ban, B = with it, d = their first
    difference -- at d the ban removed A[d], which completes an n-gram of the context."""
    cfg, _ = tiny
    llm = _llm(tiny)
    base = _prompts(cfg)
    found = None
    for seed in range(120):
        rng = np.random.Generator(np.random.PCG64(100 + seed))
        alphabet = rng.integers(0, cfg.vocab_size, size=3).tolist()
        p = [alphabet[i] for i in rng.integers(0, 3, size=17)]
        prompts = [base[0], p, base[2]]
        A = _run(llm, prompts)[0][1][0]
        for n in (2, 3, 1):
            samp = [None, dict(no_repeat_ngram_size=n), None]
            want = _run(llm, prompts, samp)
            B = want[0][1][0]
            d = next((i for i in range(len(A)) if A[i] != B[i]), None)
            if d is None or d < 2 or d > 22:
                continue
            ctx = p + B[:d]
            gram = ctx[len(ctx) - (n - 1):] + [A[d]] if n > 1 else [A[d]]
            if any(ctx[i: i + n] == gram for i in range(len(p))):   # an occurrence that starts inside the prompt
                found = (prompts, samp, want, d)
                break
        if found:
            break
    assert found, "no candidate prompt makes the first ban complete an n-gram that starts in the prompt"
    prompts, samp, want, d = found
    _same(_run(llm, prompts, samp, park=(1, d - 1, 5), filler=[4, 5, 6]), want)


@pytest.mark.parametrize("paged", [False, True])
def test_forked_take(tiny, paged):
    """num_return_sequences = 2 (shared leading pages): one take parked and resumed into pages of its own, the other untouched."""
    cfg, _ = tiny
    llm = _llm(tiny, "bf16", paged)
    prompts = [_prompts(cfg)[2], _prompts(cfg)[0]]
    samp = [dict(do_sample=True, temperature=1.1, top_k=50, top_p=0.95), None]
    llm.set_sampling(False, seed=77)
    want = _run(llm, prompts, samp, n_return=[2, 1])
    assert want[0][0] != want[0][1], "two takes, two streams"
    llm.set_sampling(False, seed=77)
    _same(_run(llm, prompts, samp, n_return=[2, 1], park=(1, 6, 5), filler=[3, 2, 1]), want)
    llm.set_sampling(False, seed=77)
    _same(_run(llm, prompts, samp, n_return=[2, 1], park=(0, 6, 5)), want)   # (_run checks the page accounting at its end)


# ------------------------------------------------------------------ blob bits
@pytest.mark.parametrize("kv,paged", [("bf16", True), ("f32", False)])
def test_blob_is_slot_independent(tiny, kv, paged):
    """save -> restore (another slot) -> save: byte-identical blobs.  No field of the layout depends on the slot."""
    cfg, _ = tiny
    llm = _llm(tiny, kv, paged)
    prompts = _prompts(cfg)
    samp = [dict(repetition_penalty=1.2, return_log_probs=True, no_repeat_ngram_size=3, stop_sequences=[[1, 2, 3]]), None, None]
    llm.session_begin(None)
    slots = llm.admit(prompts, samp)
    llm.decode(11)
    blobs = llm.save_slots([slots[0], slots[2]])
    back = llm.restore_slots(blobs)
    assert not set(back) & set(slots)
    again = llm.save_slots(back)
    for x, y in zip(blobs, again):
        assert x.numel() == y.numel() and bool((x == y).all())


def test_a_finished_slot_that_is_still_busy_is_saved(tiny):
    """A sequence that has met its eos but has not been retired keeps its slot, and its row keeps stepping (pos and the row
    descriptor advance, count does not).  Its snapshot restores into a sequence that is finished too: same tokens, same count,
    same flag, and further decode steps add nothing to either; the unfinished neighbours are not disturbed."""
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    ref = _run(llm, prompts)[0]
    eos = ref[1][0][4]                                # sequence 1 ends at the first occurrence of its fifth token
    at = ref[1][0].index(eos) + 1
    assert all(eos not in ref[i][0][:16] for i in (0, 2)), "choose another eos: a neighbour would end early"
    llm.session_begin([eos])
    slots = llm.admit(prompts)
    llm.decode(8)
    orig, ocnt, ofin = _state(llm, [slots[1]])
    assert ofin == [1] and ocnt == [at] and orig[0][0] == ref[1][0][:at]
    [blob] = llm.save_slots([slots[1]])                # finished, busy, three steps past its end
    llm.decode(3)
    [blob2] = llm.save_slots([slots[1]])
    [a, b] = llm.restore_slots([blob, blob2])
    llm.decode(4)
    toks, cnt, fin = _state(llm, [a, b, slots[1]])
    assert toks == [orig[0]] * 3 and cnt == [at] * 3 and fin == [1] * 3
    rest, _, rfin = _state(llm, [slots[0], slots[2]])
    assert [t[0] for t in rest] == [ref[0][0][:16], ref[2][0][:16]] and rfin == [0, 0]
    llm.retire_many(slots + [a, b])
    assert llm.kv_pages()[0] == llm.kv_pages()[1]


# ------------------------------------------------------------------ graph cache
def test_parking_leaves_the_step_graphs_alone(tiny):
    """use_graph=1 (the default): the session that parks and resumes ends where the one that never did ends, and goes on with
    it -- the cached step graphs are reused across save / retire / restore (as tests/test_poll_gpu.py shows for poll)."""
    cfg, _ = tiny
    llm = _llm(tiny)
    prompts = _prompts(cfg)
    want = _run(llm, prompts, steps=36)
    _same(_run(llm, prompts, steps=36, park=(0, 8, 8), filler=[5, 5, 6]), want)
    _same(_run(llm, prompts, steps=36, park=(2, 16, 8), filler=[5, 5, 6]), want)


# ------------------------------------------------------------------ refusals
def _raw(llm):
    lib = llm._lib
    i32 = C.POINTER(C.c_int32)

    def save(slots, blobs, caps=None):
        a = np.asarray(slots, np.int32)
        n = len(a)
        ptrs = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in blobs])
        cap = (C.c_size_t * max(n, 1))(*(caps if caps is not None else [b.numel() for b in blobs]))
        used = (C.c_size_t * max(n, 1))()
        return lib.smi_llm_slots_save(llm._h, a.ctypes.data_as(i32), n, ptrs, cap, used, llm._stream())

    def restore(blobs, sizes=None):
        n = len(blobs)
        ptrs = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in blobs])
        nb = (C.c_size_t * max(n, 1))(*(sizes if sizes is not None else [b.numel() for b in blobs]))
        out = np.full(max(n, 1), -7, np.int32)
        return lib.smi_llm_slots_restore(llm._h, ptrs, nb, n, out.ctypes.data_as(i32), llm._stream()), out

    return save, restore


def _free_slots(llm, max_slots=6):
    """The handle's free KV slots, read directly: the size call answers for a busy slot only (host arithmetic, no device work)."""
    nb = C.c_size_t(0)
    return [s for s in range(max_slots) if llm._lib.smi_llm_slot_blob_bytes(llm._h, s, C.byref(nb)) != 0]


def _snapshot(llm, slots):
    cnt, fin = llm.status()
    return (llm.slots_tokens(slots, MAX_POS), cnt.tolist(), fin.tolist(), llm.kv_pages(), _free_slots(llm))


def test_refusals_change_nothing(tiny):
    import torch
    from sparkmi.llm import SparkLLM
    cfg, syn = tiny
    llm = _llm(tiny, "bf16", True)
    other = _llm(tiny, "f32", True)                 # another configuration
    save, restore = _raw(llm)
    prompts = _prompts(cfg)
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    # outside a session
    llm.prefill([prompts[0]])
    assert save([0], [big]) == ESTATE and restore([big])[0] == ESTATE
    llm.session_begin(None)
    slots = llm.admit(prompts)
    llm.decode(6)
    [blob] = llm.save_slots([slots[1]])
    before = _snapshot(llm, slots)
    assert before[4] == [s for s in range(6) if s not in slots] and len(before[4]) == 3

    def unchanged():
        assert _snapshot(llm, slots) == before

    free = [s for s in range(6) if s not in slots]
    need = llm.slot_blob_bytes(slots[0])
    for args in (([free[0]], [big]), ([slots[0], slots[0]], [big, big[need + 16:]]), ([64], [big]), ([-1], [big])):
        assert save(*args) == EINVAL, args
    assert save([slots[0]], [big], [need - 1]) == EINVAL
    assert not bool(big.any()), "a refused save writes nothing"
    unchanged()
    # truncated, corrupt
    assert restore([blob], [blob.numel() - 16])[0] == EINVAL
    assert restore([blob], [64])[0] == EINVAL
    bad = blob.clone(); bad[0] ^= 0xFF
    assert restore([bad])[0] == EINVAL
    bad = blob.clone(); bad[40] ^= 0x01               # a header byte under the checksum
    assert restore([bad])[0] == EINVAL
    bad = torch.cat([blob, blob[:16]])
    assert restore([bad])[0] == EINVAL
    unchanged()
    # another configuration
    other.session_begin(None)
    o = other.admit([prompts[1]])
    other.decode(6)
    [oblob] = other.save_slots(o)
    assert restore([oblob])[0] == ESTATE
    assert b"configuration" in llm._lib.smi_last_error()
    unchanged()
    # fewer free slots than snapshots
    assert restore([blob] * 4)[0] == ESTATE
    unchanged()
    # an earlier session of this handle
    llm.session_begin(None)
    assert restore([blob])[0] == ESTATE
    assert b"earlier session" in llm._lib.smi_last_error()
    assert llm.kv_pages()[0] == llm.kv_pages()[1]
    with pytest.raises(_lib.SparkMIError):
        llm.restore_slots([blob])
    with pytest.raises(_lib.SparkMIError):
        llm.save_slots([0])
    # the pool is one page short: nothing allocated
    pages = -(-(LENS[2] + 1 + 6) // PAGE)             # pages of the 70-token sequence after 6 steps: 77 positions -> 5
    small = SparkLLM(cfg, syn, "cuda:0", max_slots=4, max_positions=MAX_POS, kv_page_tokens=PAGE, kv_pages=2 * pages - 1)
    save_s, restore_s = _raw(small)
    small.session_begin(None)
    s = small.admit([prompts[2]])
    small.decode(6)
    [b] = small.save_slots(s)
    free_before = small.kv_pages()[1]
    assert free_before == pages - 1
    want = small.slots_tokens(s, MAX_POS)
    rc, out = restore_s([b])
    assert rc == ENOMEM and (out == -7).all()
    assert _free_slots(small, 4) == [t for t in range(4) if t not in s]
    assert small.kv_pages()[1] == free_before and small.slots_tokens(s, MAX_POS) == want
    small.decode(3)                                   # the session goes on
    went_on = small.slots_tokens(s, MAX_POS)[0][0]
    small.retire_many(s)
    [r] = small.restore_slots([b])                    # now it fits
    small.decode(3)
    assert small.slots_tokens([r], MAX_POS)[0][0] == went_on and len(went_on) == 10
    small.close()
