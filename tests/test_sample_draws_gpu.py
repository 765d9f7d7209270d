"""k_sample_scan + k_sample, draw by draw, against tests/sample_ref.py: the token of every single draw lies in the float64 chain's
``accepted`` set at the derived ``delta`` (one token for > 99 % of the draws: tests/test_sample_draws_cpu.py asserts that on the
reference alone), and the bound path and the radix path name the same token with no tolerance.  First the sampler alone
(``debug_sample``: row m draws with key = seed, token index 0, admission number m), then the sampler inside real steps of mixed
records, where the counter words are (tokens the sequence has emitted before this one; its admission number, or 0xFFFFFFFF under
a record's own seed) and the reference reads the device's own logits (after k_penalize for a penalised row)."""
import dataclasses

import numpy as np
import pytest

import sample_ref as R
from sparkmi import config as C, weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden_dir):
    return {name: (row, params, n_rows) for name, row, params, n_rows in R.alone_cases(golden_dir)}


@pytest.fixture(scope="module")
def handle():
    """One diagnostics handle per vocabulary size (the tiny model with vocab_size = len(row)), shared by the cases."""
    from sparkmi.llm import SparkLLM
    made = {}

    def get(V):
        if V not in made:
            cfg = dataclasses.replace(C.tiny_llm(), vocab_size=V)
            made[V] = SparkLLM(cfg, W.SyntheticLLM(cfg), device="cuda:0", max_slots=64, max_positions=32, diag=True)
        return made[V]

    yield get
    for llm in made.values():
        llm.close()


@pytest.mark.parametrize("name", R.ALONE_NAMES)
def test_sampler_alone_draw_by_draw(cases, handle, name):
    row, params, n_rows = cases[name]
    llm = handle(len(row))
    draws = multi = agree = 0
    worst = 0.0
    for T, k, p in params:
        delta = R.delta_for(row, T, k)
        llm.set_sampling(True, T, k, p, 0)
        for seed in R.ALONE_SEEDS:
            bound = llm.debug_sample(row, n_rows, seed, use_bound=True)
            radix = llm.debug_sample(row, n_rows, seed, use_bound=False)
            for m in range(n_rows):
                u = R.uniform24(R.philox_u32(seed, 0, m))
                acc = R.accepted(row, T, k, p, u, delta)
                what = f"{name} T {T} k {k} p {p} seed {seed:#x} row {m}: u {u!r}"
                assert int(bound[m]) in acc, f"{what}: token {bound[m]} (bound path), accepted {sorted(acc)}"
                assert int(radix[m]) in acc, f"{what}: token {radix[m]} (radix path), accepted {sorted(acc)}"
                assert bound[m] == radix[m], f"{what}: bound path {bound[m]}, radix path {radix[m]}"
                worst = max(worst, R.needed_delta(row, T, k, p, u, int(bound[m]), delta) / delta if delta else 0.0)
                draws, multi, agree = draws + 1, multi + (len(acc) > 1), agree + 1
    print(f"\n{name}: {draws} draws x 2 paths, {100.0 * multi / draws:.2f} % with more than one accepted token, bound == radix on "
          f"{agree} of {draws}, largest window a draw needed {worst:.3f} x delta")


def _argmax_lowest(x):
    return int(np.argmax(x))     # (numpy: the first of equal maxima)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("n_live", R.STEP_LIVE)
def test_sampler_inside_real_steps(n_live, paged):
    """Mixed records (greedy, inherit, own T / k / p on the handle's stream, seeded, penalised) in one session; after the admission's
    own step and after each of 12 decode steps the step's logits rows are read back and every row's new token is held to them:
    a sampling row to ``accepted`` with u from (key, token index, stream word), a greedy row to the arg-max with the lowest id.
    A throwaway sequence takes admission number 0 first, so admission number j + 1 lives in slot j."""
    from sparkmi.llm import SparkLLM
    cfg = C.tiny_llm()
    V = cfg.vocab_size
    kw = dict(kv_page_tokens=16, kv_pages=4 * n_live + 4) if paged else {}
    llm = SparkLLM(cfg, W.SyntheticLLM(cfg), device="cuda:0", max_slots=n_live, max_positions=64, diag=True, **kw)
    rng = np.random.Generator(np.random.PCG64(100 + n_live))
    prompts = [rng.integers(0, V, size=int(rng.integers(3, 21))).tolist() for _ in range(n_live)]
    recs = [R.step_record(j, n_live) for j in range(n_live)]
    llm.set_sampling(**R.STEP_HANDLE)
    llm.session_begin()
    llm.retire(llm.admit([[1, 2, 3]])[0])
    slots = llm.admit(prompts, sampling=[dict(r) if r else None for r in recs])
    assert slots == list(range(n_live))
    logits = [llm.debug_read(9).view(np.float32).reshape(n_live, V).copy()]      # the admission's own step: token index 0
    for _ in range(R.STEP_STEPS):
        llm.decode(1)
        logits.append(llm.debug_read(9).view(np.float32).reshape(n_live, V).copy())
    toks = llm.slots_tokens(slots, R.STEP_STEPS + 1)
    polled = llm.poll(slots, [R.STEP_STEPS] * n_live, 1)
    llm.close()
    draws = multi = greedy = 0
    worst = 0.0
    for j, (ids, fin) in enumerate(toks):
        assert len(ids) == R.STEP_STEPS + 1 and not fin and polled[j][0] == ids[-1:]
        samples, T, k, p, _, _ = R.step_selection(recs[j])
        for t, tok in enumerate(ids):
            z = logits[t][j]
            what = f"{n_live} live rows, row {j} ({recs[j]}), token index {t}"
            if not samples:
                assert tok == _argmax_lowest(z), f"{what}: greedy token {tok}, arg-max {_argmax_lowest(z)}"
                greedy += 1
                continue
            delta = R.delta_for(z, T, k)
            u = R.uniform24(R.step_word(recs[j], t, R.STEP_FIRST_ADMISSION + j))
            acc = R.accepted(z, T, k, p, u, delta)
            assert tok in acc, f"{what}: token {tok}, u {u!r}, accepted {sorted(acc)}"
            worst = max(worst, R.needed_delta(z, T, k, p, u, tok, delta) / delta)
            draws, multi = draws + 1, multi + (len(acc) > 1)
    assert draws >= R.STEP_STEPS + 1
    assert multi <= max(1, 0.02 * draws), f"{multi} of {draws} draws had more than one accepted token"
    print(f"\n{n_live} live rows, {'paged' if paged else 'contiguous'}: {draws} draws, {100.0 * multi / draws:.2f} % with more than one "
          f"accepted token, {greedy} greedy tokens, largest window a draw needed {worst:.3f} x delta")
