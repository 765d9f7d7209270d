"""CPU: tests/sample_ref.py on its own -- the Philox mirror against literal vectors and a second statement of Philox4x32-10, the
float64 chain against what transformers' own warpers keep (tests/golden/sampling.npz), and, with ``device_order_f32`` standing
where the kernel stands in tests/test_sample_draws_gpu.py, over the same cases and seeds: every draw inside ``accepted``, few
draws with more than one accepted token (so the GPU test cannot pass by accepting everything), and every deliberately wrong
kernel rejected."""
import os

import numpy as np
import pytest

import sample_ref as R


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "sampling.npz"))


@pytest.fixture(scope="module")
def cases(golden_dir):
    return R.alone_cases(golden_dir)


# (seed, c0, c1) -> word 0; written down from philox_u32 once it agreed with philox4x32_10, which reproduces Random123's
# known-answer vectors below
VECTORS = [
    ((1234, 0, 0), 0x8A06FB78),
    (((7 << 32) | 5, 3, 0xFFFFFFFF), 0xCE64DE6F),
    ((0, 0, 0), 0x55BE7711),
    ((0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), 0x2F05EE8C),
    ((0xDEADBEEFCAFE, 11, 33), 0x96ED89D0),
    (((3 << 32) | 77, 12, 1), 0xBB9E24B4),
]
# Random123 kat_vectors, philox4x32 10: counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_mirror():
    for ctr, key, want in KAT:
        assert tuple(R.philox4x32_10(ctr, key)) == want, "the second statement is the published Philox4x32-10"
    rng = np.random.Generator(np.random.PCG64(5))
    tried = [a for a, _ in VECTORS] + [tuple(int(x) for x in rng.integers(0, 2 ** 63, size=3) % (2 ** 64, 2 ** 32, 2 ** 32))
                                       for _ in range(200)]
    for seed, c0, c1 in tried:
        assert R.philox_u32(seed, c0, c1) == R.philox4x32_10((c0, c1, 0x5EED5EED, 0), (seed & R.M32, seed >> 32))[0]
    for args, want in VECTORS:
        assert R.philox_u32(*args) == want, f"philox_u32{args} = {R.philox_u32(*args):#010x}"
    assert R.uniform24(0xFFFFFFFF) == 1.0 - 2.0 ** -24 and R.uniform24(0xFF) == 0.0


@pytest.mark.parametrize("name,n", [("tiny", 5), ("big", 3), ("tie", 2), ("edge", 5)])
def test_survivor_sets_equal_transformers(g, name, n):
    """The float64 chain keeps exactly the ids transformers' warpers left in the fixture, wherever the cut is not within delta of
    its threshold; where it is (the ``edge`` sets are built that way), the fixture's ids are one of the accepted keeps."""
    row = R.fixture_row(g, name)
    assert len(g[f"{name}.params"]) == n
    near = 0
    for i, (t, k, p) in enumerate(g[f"{name}.params"]):
        sets = R.kept_ids(row, float(t), int(k), float(p), R.delta_for(row, float(t), int(k)))
        want = np.sort(g[f"{name}.{i}.ids"])
        assert len(sets) <= 2
        if len(sets) == 1:
            np.testing.assert_array_equal(sets[0], want, err_msg=f"{name}[{i}]")
        else:
            near += 1
            assert any(np.array_equal(s, want) for s in sets), f"{name}[{i}]: the fixture's ids are neither accepted keep"
    assert near == 0 or name == "edge"


def _case_stats(row, params, n_rows, kernel):
    """(draws, draws with more than one accepted token, draws the kernel misses) of one case"""
    draws = multi = miss = 0
    for T, k, p in params:
        delta = R.delta_for(row, T, k)
        for _, _, r in R.alone_draws(n_rows):
            acc = R.accepted(row, T, k, p, R.uniform24(r), delta)
            draws += 1
            multi += len(acc) > 1
            miss += kernel(row, T, k, p, r) not in acc
    return draws, multi, miss


@pytest.fixture(scope="module")
def stats(cases):
    return {name: _case_stats(row, params, n_rows, R.device_order_f32) for name, row, params, n_rows in cases}


def test_kernel_order_draws_are_accepted_and_few_are_ambiguous(cases, stats):
    """The ambiguity condition of the GPU test, asserted on the reference alone: per case at most 2 % of the draws have more than
    one accepted token, over all cases at least 95 % have exactly one."""
    tot = amb = 0
    for name, (draws, multi, miss) in stats.items():
        print(f"{name}: {draws} draws, {multi} with more than one accepted token ({100.0 * multi / draws:.2f} %), {miss} missed")
        assert miss == 0, f"{name}: device_order_f32 left accepted() {miss} times"
        assert multi <= 0.02 * draws, f"{name}: {multi} of {draws} draws are ambiguous"
        tot, amb = tot + draws, amb + multi
    print(f"all cases: {tot} draws, {100.0 * amb / tot:.3f} % ambiguous")
    assert tot - amb >= 0.95 * tot


def test_observed_f32_discrepancy_is_inside_delta(cases):
    """What the module docstring quotes: the largest distance ``device_order_f32`` shows from float64, against the derived bound."""
    worst = (0.0, 0.0, "")
    for name, row, params, n_rows in cases:
        for T, k, p in params:
            delta = R.delta_for(row, T, k)
            d = max(R.f32_discrepancy(row, T, k, p, r) for _, _, r in R.alone_draws(min(n_rows, 4)))
            assert d <= delta, f"{name} T {T} k {k} p {p}: {d:.3e} > delta {delta:.3e}"
            if d > worst[0]:
                worst = (d, delta, f"{name} T {T} k {k} p {p}")
    print(f"largest |f32 - f64| {worst[0]:.3e} (delta {worst[1]:.3e}) at {worst[2]}")


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_kernels_are_rejected(cases, variant):
    """Each wrong chain, run as the kernel over the GPU test's cases and seeds, leaves accepted() on at least one draw."""
    caught = []
    for name, row, params, n_rows in cases:
        if len(row) == R.BIG_V:
            continue      # (the small rows catch every variant; the big ones only cost time here)
        _, _, miss = _case_stats(row, params, n_rows, lambda *a: R.device_order_f32(*a, variant=variant))
        if miss:
            caught.append(f"{name} x{miss}")
    print(f"{variant}: rejected by {', '.join(caught)}")
    assert caught, f"no case rejects the variant {variant!r}"


def _step_misses(row, variant):
    """The in-step schedule of the GPU test (records, admission numbers, token indices) on a stand-in logits row, with the
    kernel drawing from a wrong stream: draws outside accepted()."""
    miss = 0
    for n_live in R.STEP_LIVE:
        for j in range(n_live):
            rec = R.step_record(j, n_live)
            samples, T, k, p, _, _ = R.step_selection(rec)
            if not samples:
                continue
            delta = R.delta_for(row, T, k)
            for tok in range(R.STEP_STEPS + 1):
                adm = R.STEP_FIRST_ADMISSION + j
                acc = R.accepted(row, T, k, p, R.uniform24(R.step_word(rec, tok, adm)), delta)
                miss += R.device_order_f32(row, T, k, p, R.step_word(rec, tok, adm, variant)) not in acc
    return miss


@pytest.mark.parametrize("variant", ["swapped", "seeded_on_admission"])
def test_wrong_streams_are_rejected(g, variant):
    """Counter words swapped, and a seeded row on the admission-number stream: the draws are still seeded, reproducible and
    different per seed -- and almost all of them name another token."""
    row = R.fixture_row(g, "tiny")
    assert _step_misses(row, None) == 0
    miss = _step_misses(row, variant)
    print(f"{variant}: {miss} draws rejected")
    assert miss > 0


def test_swapped_words_show_in_the_sampler_alone(g):
    """debug_sample's row m draws with (token index 0, admission number m): swapped words move every row from 1 on."""
    row = R.fixture_row(g, "tiny")
    T, k, p = 0.8, 50, 0.95
    delta = R.delta_for(row, T, k)
    wrong = sum(R.device_order_f32(row, T, k, p, R.philox_u32(seed, m, 0)) not in R.accepted(row, T, k, p, R.uniform24(r), delta)
                for seed, m, r in R.alone_draws(64))
    assert wrong > 0


def test_case_names_are_the_parametrised_ones(cases):
    assert tuple(name for name, _, _, _ in cases) == R.ALONE_NAMES
    assert {n for _, _, _, n in cases} == {1, 16, 64}
