"""Long-form synthesis, the parts that need no GPU: the text splitter, the per-sentence plan (seeds, the continuation of a created
voice), the host layout function of the assembly, and the inputs of tests/test_trim_gpu.py themselves -- the two restatements
of the bounds agree on them and no window sits near the threshold, which is what makes the exact comparison on the GPU mean
something."""
import ctypes
import random

import numpy as np
import pytest

import trim_ref as tr
from sparkmi import longform as L


# ---- split_text: fixed cases
def test_english_sentences():
    got = L.split_text("The first sentence is here. Is the second one a question? It certainly is! And then; a clause.", 300, 0)
    assert got == ["The first sentence is here.", "Is the second one a question?", "It certainly is!", "And then;", "a clause."]


def test_chinese_without_spaces():
    got = L.split_text("今天天气很好。我们去公园散步吧！你觉得怎么样？好的", 300, 0)
    assert got == ["今天天气很好。", "我们去公园散步吧！", "你觉得怎么样？", "好的"]
    assert L.width("今天天气很好。") == 21 and L.width("abc.") == 4


def test_mixed_scripts():
    got = L.split_text("He said hello. 她说你好。Then they left.", 300, 0)
    assert got == ["He said hello.", "她说你好。", "Then they left."]


def test_a_point_between_digits_ends_nothing():
    assert L.split_text("Pi is about 3.14 and e about 2.71. That is all.", 300, 0) == ["Pi is about 3.14 and e about 2.71.", "That is all."]
    assert L.split_text("Version 2. It works.", 300, 0) == ["Version 2.", "It works."]
    assert L.split_text("See example.com for more. Thanks.", 300, 0) == ["See example.com for more.", "Thanks."]


def test_closing_quotes_stay_with_the_sentence():
    got = L.split_text('"Is it done?" she asked. (It was.) He said: "Yes!"', 300, 0)
    assert got == ['"Is it done?"', "she asked.", "(It was.)", 'He said: "Yes!"']
    assert L.split_text("他说：“走吧。”然后走了。", 300, 0) == ["他说：“走吧。”", "然后走了。"]
    assert L.split_text("Wait... what?! No.", 300, 0) == ["Wait...", "what?!", "No."]


def test_paragraph_break():
    got = L.split_text("A heading without a stop\n\nThe body follows here\nwith a plain newline inside.\n \n\nLast", 300, 0)
    assert got == ["A heading without a stop", "The body follows here\nwith a plain newline inside.", "Last"]


def test_no_punctuation_at_all_is_cut_at_whitespace():
    text = " ".join(f"word{i}" for i in range(60))
    got = L.split_text(text, 50, 10)
    assert " ".join(got) == text and all(L.width(p) <= 50 for p in got) and len(got) > 5
    assert all(L.width(a + " " + b.split(" ")[0]) > 50 for a, b in zip(got, got[1:]))   # each piece is as long as the limit allows


def test_one_very_long_clause():
    text = "x" * 95
    assert L.split_text(text, 40, 5) == ["x" * 40, "x" * 40, "x" * 15]
    assert L.split_text("好" * 10, 9, 0) == ["好" * 3] * 3 + ["好"]
    got = L.split_text("alpha beta, gamma delta epsilon zeta eta theta", 24, 0)   # after the last comma inside the limit, then whitespace
    assert got == ["alpha beta,", "gamma delta epsilon zeta", "eta theta"]


def test_a_trailing_short_piece_joins_the_previous_one():
    assert L.split_text("This sentence is long enough to stand alone. Ok.", 300, 20) == ["This sentence is long enough to stand alone. Ok."]
    assert L.split_text("Hi. This sentence is long enough to stand alone.", 300, 20) == ["Hi. This sentence is long enough to stand alone."]
    assert L.split_text("This sentence is long enough to stand alone. Ok.", 45, 20) == ["This sentence is long enough to stand alone.", "Ok."]
    assert L.split_text("好。" * 3, 300, 20) == ["好。好。好。"]   # no space at a wide seam


def test_refusals():
    for bad in ("", "  \n\t ", None):
        with pytest.raises(ValueError, match="empty"):
            L.split_text(bad)
    with pytest.raises(ValueError, match="max_width"):
        L.split_text("hello", max_width=10, min_width=20)
    with pytest.raises(ValueError, match="max_width"):
        L.split_text("hello", max_width=2, min_width=0)
    with pytest.raises(ValueError, match="int"):
        L.split_text("hello", max_width=30.5)


# ---- split_text: the invariants on random strings
ALPHABET = list("abcdefg hij  klm\n\n\t.,;:!?…\"')]0123456789.。！？；，、：“”）好世界天气漢字ｗｉｄｅ") + ["\n", " ", " ", ". ", "3.14"]


def test_invariants_on_random_strings():
    rnd = random.Random(20240)
    checked = 0
    for trial in range(400):
        text = "".join(rnd.choice(ALPHABET) for _ in range(rnd.randrange(1, 400)))
        max_width = rnd.choice([3, 4, 7, 20, 50, 300])
        min_width = rnd.choice([0, 1, 5, 20, 300])
        if not text.strip() or max_width < min_width:
            with pytest.raises(ValueError):
                L.split_text(text, max_width, min_width)
            continue
        pieces = L.split_text(text, max_width, min_width)
        assert pieces and all(p and p == p.strip() for p in pieces), (text, pieces)
        assert all(L.width(p) <= max_width for p in pieces), (text, pieces)
        strip = lambda s: "".join(c for c in s if not c.isspace())   # noqa: E731
        assert strip("".join(pieces)) == strip(text), (text, pieces)     # every character once, in order
        checked += 1
    assert checked > 250


# ---- the per-sentence plan
def test_sentence_seeds():
    assert L.sentence_seeds(None, 3) == [None, None, None]
    assert L.sentence_seeds(40, 4) == [40, 41, 42, 43]
    with pytest.raises(ValueError):
        L.sentence_seeds(1.5, 2)
    with pytest.raises(ValueError):
        L.sentence_seeds(True, 2)


class _StubTokenizer:
    """the vocabulary surface ``pipeline._TokenMap`` reads, and a prompt tokenizer that keeps every <|...|> token whole"""

    def __init__(self):
        names = ["<|task_controllable_tts|>", "<|start_content|>", "<|end_content|>", "<|start_style_label|>", "<|end_style_label|>",
                 "<|gender_0|>", "<|gender_1|>", "<|start_global_token|>", "<|end_global_token|>", "<|start_semantic_token|>", "<|im_end|>"]
        names += [f"<|pitch_label_{i}|>" for i in range(5)] + [f"<|speed_label_{i}|>" for i in range(5)]
        names += [f"<|pitch_value_{i}|>" for i in range(4)] + [f"<|speed_value_{i}|>" for i in range(4)]
        names += [f"<|bicodec_global_{i}|>" for i in range(16)] + [f"<|bicodec_semantic_{i}|>" for i in range(16)]
        self.vocab = {n: 100 + i for i, n in enumerate(names)}
        self.all_special_ids = [self.vocab["<|im_end|>"]]

    def get_vocab(self):
        return dict(self.vocab)

    def __call__(self, text):
        import re
        return [self.vocab[t] if t in self.vocab else 1000 + (sum(map(ord, t)) % 50) for t in re.findall(r"<\|[^|]*\|>|[^<]+", text)]


def test_control_mode_plan_appends_what_sentence_0_decided():
    from sparkmi.pipeline import _TokenMap
    tok = _StubTokenizer()
    tm = _TokenMap(tok)
    v = tok.vocab
    glob = [5, 3, 9, 1]
    head = ([v["<|pitch_value_2|>"], v["<|speed_value_1|>"], v["<|end_style_label|>"], v["<|start_global_token|>"]]
            + [v[f"<|bicodec_global_{g}|>"] for g in glob] + [v["<|end_global_token|>"], v["<|start_semantic_token|>"]])
    sem = [v[f"<|bicodec_semantic_{s}|>"] for s in (7, 7, 2)]
    new = head + sem + [v["<|im_end|>"]]
    prefix, got = L.control_prefix(new, tm.sem, tm.glob, 4)
    assert prefix == head and got == glob
    p0 = L.control_prompt_ids(tok, "female", "low", "high", "First sentence.")
    p1 = L.control_prompt_ids(tok, "female", "low", "high", "Second one.", prefix)
    assert p0[-1] == v["<|end_style_label|>"] and v["<|gender_0|>"] in p0
    assert p1[-len(head):] == head and p1[: -len(head)] == tok(L.build_control_prompt("female", "low", "high", "Second one."))
    # a global token after the first semantic id does not count; an incomplete block is inference_batch's error
    for bad in (head[:6] + sem + [v["<|bicodec_global_0|>"]] * 2, sem, []):
        with pytest.raises(ValueError, match="global tokens generated, the speaker encoder needs 4"):
            L.control_prefix(bad, tm.sem, tm.glob, 4)
    with pytest.raises(AssertionError):
        L.control_prompt_ids(tok, "robot", "low", "high", "x")


def test_ready_run_and_trim_params():
    assert L.ready_run({0: 1, 1: 1, 3: 1}, 0, 8) == [0, 1] and L.ready_run({0: 1, 1: 1, 2: 1}, 0, 2) == [0, 1]
    assert L.ready_run({2: 1}, 1, 8) == [] and L.ready_run({2: 1, 3: 1}, 2, 8) == [2, 3]
    assert L.trim_params(16000) == (1600, 160, 3200) and L.trim_params(22050) == (2205, 220, 4410)


# ---- the host layout function against trim_ref
def test_concat_layout_matches_the_reference_formula():
    from sparkmi import _lib
    l = _lib.lib()
    rng = np.random.default_rng(3)
    i32 = lambda v: (ctypes.c_int32 * len(v))(*[int(a) for a in v])   # noqa: E731
    for trial in range(50):
        B = int(rng.integers(1, 65))
        start = rng.integers(0, 50, B)
        length = rng.integers(0, 4, B) * rng.integers(0, 900, B)
        gaps = rng.integers(0, 3, B) * rng.integers(0, 300, B)
        bounds = [(int(a), int(a + n)) for a, n in zip(start, length)]
        offs, total = tr.layout(bounds, gaps)
        got = (ctypes.c_longlong * B)()
        assert l.smi_concat_layout(i32(start), i32(start + length), i32(gaps), B, got) == total
        assert list(got) == offs
        assert l.smi_concat_layout(i32(start), i32(start + length), i32(gaps), B, None) == total
    assert l.smi_concat_layout(i32([3]), i32([2]), i32([0]), 1, None) == -1
    assert l.smi_concat_layout(i32([0]), i32([2]), i32([-1]), 1, None) == -1
    assert l.smi_concat_layout(i32([0]), i32([2]), i32([0]), 0, None) == -1
    assert l.smi_concat_layout(i32([0] * 65), i32([1] * 65), i32([0] * 65), 65, None) == -1
    # the scratch of smi_trim_rows: two int32 per tile of 64 windows and row
    assert l.smi_trim_work_len(0, 20, 2, 3) == 6 and l.smi_trim_work_len(19, 20, 2, 1) == 2
    assert l.smi_trim_work_len(20 + 2 * 63, 20, 2, 1) == 2 and l.smi_trim_work_len(20 + 2 * 64, 20, 2, 1) == 4
    assert l.smi_trim_work_len(100, 0, 2, 1) == -1 and l.smi_trim_work_len(100, 20, 2, 65) == -1


# ---- the inputs of the GPU tests
@pytest.mark.parametrize("name", sorted(tr.PARAMS))
def test_gpu_inputs_are_decided_the_same_way_by_both_restatements(name):
    W, s, m, thr = tr.PARAMS[name]
    seen = set()
    for label, x in tr.trim_cases(name):
        a, b = tr.bounds(x, W, s, thr, m), tr.bounds_reference_style(x, W, s, thr, m)
        assert a == b, (name, label, a, b)
        # fp32 evaluates a window's energy to about 1e-6 relative, fp64 to about 2e-13: 1e-4 leaves two orders of margin
        assert tr.closest_to_level(x, W, s, thr) > 1e-4, (name, label)
        seen.add((label, a[0] == 0, a[1] == len(x), a == (0, 0)))
    by = {l: rest for l, *rest in seen}
    assert by["n=W-1"][:2] == [True, True] and by["silent"][2] and by["zeros"][2] and by["n=0"][2]
    assert by["speech in the first window"][0] and not by["speech in the first window"][1]
    assert by["speech in the last window"][1] and not by["speech in the last window"][0]
    assert not any(by["speech in the middle"])
    for label in ("tile+1 windows", "tile-1 windows", "2 tiles+1 windows"):
        assert by[label][1] and not by[label][2]


@pytest.mark.parametrize("name", sorted(tr.PARAMS))
def test_equality_case_counts_as_speech(name):
    W, s, m, _ = tr.PARAMS[name]
    x, thr, i = tr.equality_case(name)
    e = tr.energies(x, W, s)
    assert e[i] == tr.level(W, thr) and (np.delete(e, i) < tr.level(W, thr)).all()     # exactly on the level, and alone there
    want = (max(0, i * s - m), min(len(x), i * s + m))
    assert tr.bounds(x, W, s, thr, m) == want == tr.bounds_reference_style(x, W, s, thr, m)


def test_fade_weights_and_middle_sample():
    p = np.ones(5, np.float32)
    assert tr.faded(p, 8).tolist() == [np.float32(1 / 3), np.float32(2 / 3), 1.0, np.float32(2 / 3), np.float32(1 / 3)]
    assert tr.faded(np.ones(4, np.float32), 8).tolist() == [np.float32(1 / 3), np.float32(2 / 3), np.float32(2 / 3), np.float32(1 / 3)]
    assert tr.faded(np.ones(1, np.float32), 8).tolist() == [1.0] and tr.faded(p, 0).tolist() == [1.0] * 5
    out, offs, total = tr.concat([np.arange(6), np.arange(6), np.arange(6)], [(1, 3), (2, 2), (0, 6)], [4, 5, 2], 0, cap=14)
    assert offs == [4, 6, 8] and total == 14 and out.tolist() == [0, 0, 0, 0, 1, 2, 0, 0, 0, 1, 2, 3, 4, 5]
