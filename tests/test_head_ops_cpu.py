"""No GPU: the table behind tests/test_head_ops_gpu.py (tests/head_cases.py) is sound at every case shape.

  * the float64 reference agrees with a second float64 statement of the head (transformers' order) inside the bound;
  * the fp32 model of the kernels' arithmetic passes the bound;
  * every corruption is rejected -- by the bound (CORRUPT_LOGITS) or by the token rule (CORRUPT_PICK);
  * the token rule excludes no row: the seeds give every row a clear float64 decision;
  * the launch forms the GPU cases name cover every form launch_one(KLM) has.

Which inputs carry which corruption: the five logits corruptions run on the seeded rows of every shape; `drop_lo` on rows whose lo terms are all positive, at
hidden 32 (from 128 on the whole lo chain is below the bound), for the bf16 kernels' lo chain and for the exact-weights kernel's rebuilt operand; `tie_high` on the planted pairs of every shape; `ignore_last_vtile` on the row whose maximum is planted alone in the last vocabulary tile;
`tail_ids` on the row whose valid logits are all negative; `mask_after_best` on restricted rows with a global maximum planted
one id past a range.
"""
import functools

import numpy as np
import pytest

import head_cases as H


@functools.lru_cache(maxsize=2)
def _group(name):
    hidden, vocab, rows, exact, tag = H.GROUPS[name]
    M = max(rows)
    W, gamma, x = H.make_inputs(hidden, vocab, exact, tag, rows=M)
    ref, A, g, r = H.head_ref(W, gamma, x)
    return W, gamma, x, ref, H.head_bound(ref, A, hidden)


@pytest.mark.parametrize("name", list(H.GROUPS))
def test_reference_model_and_logits_corruptions(name):
    hidden, vocab, rows, exact, tag = H.GROUPS[name]
    W, gamma, x, ref, bnd = _group(name)
    ok, ratio = H.accept(H.head_ref_textbook(W, gamma, x), ref, bnd)
    assert ok, f"{name}: the two float64 statements differ by {ratio:.3f} of the bound"
    ok, ratio = H.accept(H.head_model(W, gamma, x, exact=exact), ref, bnd)
    assert ok, f"{name}: the fp32 model is at {ratio:.3f} of the bound"
    print(f"{name}: fp32 model at {ratio:.3f} of the bound")
    for c in H.CORRUPT_LOGITS:
        if c == "drop_mid" and exact:
            continue                       # the exact-weights kernel has one chain on x = hi + mid + lo
        if c == "neighbour_norm" and x.shape[0] < 2:
            continue
        ok, ratio = H.accept(H.head_model(W, gamma, x, exact=exact, corrupt=c), ref, bnd)
        assert not ok and ratio > 2.0, f"{name}: corruption {c} passes the bound ({ratio:.3f})"


@pytest.mark.parametrize("name", list(H.GROUPS))
def test_token_rule_excludes_no_row_and_holds_the_models_pick(name):
    hidden, vocab, rows, exact, tag = H.GROUPS[name]
    W, gamma, x, ref, bnd = _group(name)
    ids, held = H.decision(ref, bnd)
    assert held.all(), f"{name}: rows {np.flatnonzero(~held)} have no clear float64 decision: pick another seed tag"
    got = H.head_model(W, gamma, x, exact=exact)
    ok, excluded, msg = H.token_rule(H.pick_tokens(got), ref, bnd, stored=got)
    assert ok and excluded == 0.0, msg


def _planted(name, M=24):
    hidden, vocab, rows, exact, tag = H.GROUPS[name]
    M = min(M, max(rows))
    form, grid, _, _, _ = H.expected_form(hidden, vocab, min(M, 16), exact)
    pairs, solos, neg = H.planted_plan(vocab, grid[0], form, M)
    W, gamma, x, owner, solo_at = H.planted_inputs(hidden, vocab, pairs, exact, tag, rows=M, solos=solos, negative_row=neg)
    ref, A, g, r = H.head_ref(W, gamma, x)
    return pairs, W, gamma, x, owner, ref, H.head_bound(ref, A, hidden), exact


@pytest.mark.parametrize("name", list(H.GROUPS))
def test_planted_rows_reject_the_pick_corruptions(name):
    pairs, W, gamma, x, owner, ref, bnd, exact = _planted(name)
    names = list(pairs)
    ids, held = H.decision(ref, bnd)
    assert held.all(), f"{name}: planted rows {np.flatnonzero(~held)} have no clear decision"
    for m, o in enumerate(owner):
        if o >= 0:
            a, b = pairs[names[o]]
            assert ids[m] == a and ref[m, a] == ref[m, b] == ref[m].max(), (name, m, names[o])
    got = H.head_model(W, gamma, x, exact=exact)
    for nm, (a, b) in pairs.items():
        assert np.array_equal(got[:, a].view(np.uint32), got[:, b].view(np.uint32)), f"{name}: pair {nm}: identical weight rows, different bits"
    ok, excluded, msg = H.token_rule(H.pick_tokens(got), ref, bnd, stored=got)
    assert ok and excluded == 0.0, msg
    ok, _, _ = H.token_rule(H.pick_tokens(got, corrupt="tie_high"), ref, bnd, stored=got)
    assert not ok, f"{name}: the higher index on a tie passes the token rule"
    if (owner == -1).any():
        ok, _, _ = H.token_rule(H.pick_tokens(got, corrupt="ignore_last_vtile"), ref, bnd, stored=got)
        assert not ok, f"{name}: a pick that ignores the last vocabulary tile passes the token rule"
    if (owner == -2).any() and ref.shape[1] % 16:
        m = int(np.flatnonzero(owner == -2)[0])
        assert ref[m].max() < 0, f"{name}: the all-negative row has a positive logit"
        bad = H.pick_tokens(got, corrupt="tail_ids")
        assert bad[m] >= ref.shape[1]
        ok, _, _ = H.token_rule(bad, ref, bnd, stored=got)
        assert not ok, f"{name}: a pick among the padding ids of the tail tile passes the token rule"


@pytest.mark.parametrize("hidden,rows", sorted({(h, m) for h, m, _ in H.RESTRICTED_CASES}))
def test_restricted_rows_reject_a_mask_applied_after_the_running_best(hidden, rows):
    vocab = 1000
    W, gamma, x, allow, tiles = H.restricted_inputs(hidden, vocab, rows)   # the global maximum of row 0: one id past its range
    assert len(tiles) % 2 == 1 and 3 not in tiles, "the union must have an odd number of tiles (the last group is half empty)"
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, hidden)
    assert int(np.argmax(ref[0])) == 48
    ids, held = H.decision(ref, bnd, allow)
    assert held.all()
    got = H.head_model(W, gamma, x)
    ok, excluded, msg = H.token_rule(H.pick_tokens(got, allow), ref, bnd, stored=got, allow=allow)
    assert ok and excluded == 0.0, msg
    bad = H.pick_tokens(got, allow, corrupt="mask_after_best")
    assert bad[0] == 48
    ok, _, _ = H.token_rule(bad, ref, bnd, stored=got, allow=allow)
    assert not ok, "a restricted row's mask applied after the running best passes the token rule"


def test_the_cases_reach_every_launch_form():
    forms = set()
    for name, (hidden, vocab, rows, exact, tag) in H.GROUPS.items():
        for M in rows:
            forms.add(H.expected_form(hidden, vocab, M, exact)[0])
    for M in (17, 33, 64):
        forms.add(H.expected_form(256, 1000, M, two_group=True)[0])
    for M in (2, 17, 33):
        forms.add(H.expected_form(256, 1000, M, restricted=True)[0])
    forms.add(H.expected_form(1024, 1000, 17, restricted=True)[0])
    forms.add(H.expected_form(256, 1000, 17, restricted=True, two_group=True)[0])
    assert forms == {"k_lm<1>", "k_lm32<7>", "k_lm32<8>", "k_lm<2>", "k_lm<1,RT>", "k_lm32<7,RT>", "k_lm32<8,RT>", "k_lm<2,RT>",
                     "k_gemm<1,EPI_LM>", "k_gemm<2,EPI_LM>", "k_gemm_x<EPI_LM>"}
    # the shapes of the issue's table
    assert H.expected_form(64, 16400, 1)[4] == 257 and H.expected_form(64, 16400, 17)[4] == 256
    assert H.expected_form(64, 33003, 16)[1] == (512, 1) and H.expected_form(64, 33003, 17)[1] == (256, 1)
    assert H.expected_form(32, 262200, 2, exact=True)[4] == 4097 > 16 * 256
    assert [H.ktiles(h) for h in (64, 256, 896, 928, 1024, 1056)] == [2, 8, 28, 29, 32, 33]


def test_a_dropped_lo_chain_is_rejected_where_the_bound_can_see_it():
    W, gamma, x = H.lo_inputs(H.LO_HIDDEN, H.LO_VOCAB, 17)
    hi, mid, lo = H.split3(gamma[None, :] * x)
    assert (lo > 0).all() and np.array_equal((hi + mid) + lo, x), "every lo term positive, the split exact"
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, H.LO_HIDDEN)
    ok, ratio = H.accept(H.head_model(W, gamma, x), ref, bnd)
    assert ok, f"the fp32 model is at {ratio:.3f} of the bound on the lo inputs"
    ok, ratio = H.accept(H.head_model(W, gamma, x, corrupt="drop_lo"), ref, bnd)
    assert not ok and ratio > 1.5, f"a dropped lo chain passes the bound ({ratio:.3f})"
    # the exact-weights kernel rebuilds x = (hi + mid) + lo in one line that all its epilogues share: the same inputs pin it
    ok, ratio = H.accept(H.head_model(W, gamma, x, exact=True), ref, bnd)
    assert ok, f"the exact-weights fp32 model is at {ratio:.3f} of the bound on the lo inputs"
    ok, ratio = H.accept(H.head_model(W, gamma, x, exact=True, corrupt="drop_lo"), ref, bnd)
    assert not ok and ratio > 1.5, f"an operand rebuilt without its lo term passes the bound ({ratio:.3f})"
    assert H.expected_form(H.LO_HIDDEN, H.LO_VOCAB, 17, exact=True)[:2] == ("k_gemm_x<EPI_LM>", (H.lm_cap(H.LO_VOCAB), 2))
