"""smi_enc_forward_rows: a ragged batch of prompts in one call, every row bit-equal to smi_enc_forward of that row alone.

The whole-encode tests compare ids and nine intermediate stages of every row with a solo run on a second handle of the same
config (np.array_equal on the raw values), in two orders and as B = 1 calls, and assert through the diagnostics that the call
was cut into several runs and that one run holds rows of different lengths.  The kernel tests (further down) run ONE launch of a
rows list on three rows written through the diagnostics and hold every row to the float64 restatement and bound tests/enc_cases.py
defines for that kernel; a fourth, unused row slot and the columns beyond each row's length must stay untouched."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

import enc_cases as ec
from oracle.tokenize_ref import get_ref_clip
from sparkmi import config as C, config_tok as T, weights as W
from sparkmi._lib import SparkMIError

pytestmark = pytest.mark.gpu

STAGES = ("input_values", "conv_feats", "hs0", "feat", "z", "mel", "ecapa_latent", "perceiver", "fsq_bounded")
CANARY = -7
SENTINEL = np.float32(12345.0)
PS = "speaker_encoder.perceiver_sampler"
SE2 = "speaker_encoder.speaker_encoder.layer2.se_res2block"


def _make(wcfg, tcfg, vcfg, **kw):
    from sparkmi.encoder import BiCodecEncoder
    wsd = W.wav2vec2_state(wcfg)
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    wf = W.fold_pos_conv_weight_norm(wsd)
    return BiCodecEncoder(wcfg, tcfg, wf, tsd, "cuda:0", diag=True, **kw), wsd, wf, tsd


# At the tiny config every row of up to 3 s (149 frames) has ONE launch plan: its widest layer, the first strided conv, has
# ceil(T1 / 64) <= 75 column tiles of one 32-channel output tile, far below the 256 blocks at which the builder widens the tile.
# A 520-frame row (T1 = 16647: 261 tiles) crosses that threshold, so the handles here admit 11 s and the call carries such a
# row next to the lengths around the kernels' tiles (2, 64, 65, 130) and the 3 s limit (149, twice).
MAX_SECONDS = 11.0
FRAMES = (130, 2, 520, 65, 149, 64, 149)
N_REF = (800, 129, 16000, 1003, 5000, 8000, 129)      # 129 = n_fft / 2 + 1, the shortest accepted


@functools.lru_cache(maxsize=None)
def _pair(exact):
    """(rows handle, solo handle) of one config"""
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), C.tiny_bicodec()
    a = _make(wcfg, tcfg, vcfg, max_seconds=MAX_SECONDS, ref_seconds=1.0, exact_fp32=exact)[0]
    b = _make(wcfg, tcfg, vcfg, max_seconds=MAX_SECONDS, ref_seconds=1.0, exact_fp32=exact)[0]
    return a, b


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(77)
    wavs = [(0.1 * rng.standard_normal(ec.samples_for(t)) + 0.01).astype(np.float32) for t in FRAMES]
    refs = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in N_REF]
    return wavs, refs


def _solo_run(enc, w, r, stages=STAGES):
    g, s = enc.tokenize_arrays(w, r)
    return dict(sem=s.cpu().numpy()[0], glob=g.cpu().numpy().reshape(-1), **{k: enc.debug_stage(k).cpu().numpy() for k in stages})


@functools.lru_cache(maxsize=None)
def _solo(exact):
    """every row alone through smi_enc_forward on the second handle: computed once, shared, never changed"""
    wavs, refs = _inputs()
    return [_solo_run(_pair(exact)[1], w, r) for w, r in zip(wavs, refs)]


def _rows_call(enc, wavs, refs, stages=STAGES, pad=5):
    """one smi_enc_forward_rows call in the given order on padded tensors; sem is pre-filled with a canary"""
    from sparkmi.encoder import pack_rows
    B = len(wavs)
    ns, nr = [len(w) for w in wavs], [len(r) for r in refs]
    order = list(range(B))
    w = torch.from_numpy(pack_rows(wavs, order, max(ns) + pad)).cuda()
    r = torch.from_numpy(pack_rows(refs, order, max(nr) + pad)).cuda()
    frames = [enc.wcfg.frames(n) for n in ns]
    sstride = max(frames) + pad
    sem = torch.full((B, sstride), CANARY, dtype=torch.int64, device="cuda")
    glob = torch.full((B, enc.tcfg.spk_token_num), CANARY, dtype=torch.int32, device="cuda")
    cns, cnr, nf = (C_.c_int32 * B)(*ns), (C_.c_int32 * B)(*nr), (C_.c_int32 * B)()
    enc._lib.check(enc._lib.smi_enc_forward_rows(enc._h, C_.c_void_p(w.data_ptr()), w.shape[1], cns, C_.c_void_p(r.data_ptr()), r.shape[1], cnr, B,
                                                 C_.c_void_p(sem.data_ptr()), sstride, C_.c_void_p(glob.data_ptr()), nf, enc._stream()),
                   "smi_enc_forward_rows")
    torch.cuda.synchronize()
    assert list(nf) == frames
    sem, glob = sem.cpu().numpy(), glob.cpu().numpy()
    out = []
    for b in range(B):
        assert (sem[b, frames[b]:] == CANARY).all(), f"row {b}: ids written beyond its {frames[b]} frames"
        out.append(dict(sem=sem[b, :frames[b]], glob=glob[b], **{k: enc.rows_debug_stage(b, k).cpu().numpy() for k in stages}))
    return out


def _same(got, want, what):
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, (what, k, got[k].shape, v.shape)
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              v.view(np.uint32) if v.dtype == np.float32 else v), f"{what}: {k} differs from the solo run"


@pytest.mark.parametrize("exact", [False, True])
def test_whole_encode_rows_equal_solo_bits(exact):
    enc = _pair(exact)[0]
    wavs, refs = _inputs()
    want = _solo(exact)
    enc.rows_reserve(len(wavs), max(len(w) for w in wavs), max(len(r) for r in refs))
    got = _rows_call(enc, wavs, refs)
    starts, launches = enc.rows_debug_runs()
    print(f"RUNS exact={exact} frames={FRAMES} run starts={starts} launches={launches}")
    # the call provably reaches run splitting and ragged rows inside one launch
    assert len(starts) >= 2, starts
    ends = starts[1:] + [len(wavs)]
    assert any(len({(FRAMES[b], N_REF[b]) for b in range(s, e)}) >= 2 for s, e in zip(starts, ends)), (starts, FRAMES)
    for b in range(len(wavs)):
        _same(got[b], want[b], f"row {b} ({FRAMES[b]} frames)")
    # another order
    perm = [4, 6, 0, 3, 2, 5, 1]
    got2 = _rows_call(enc, [wavs[i] for i in perm], [refs[i] for i in perm])
    for j, i in enumerate(perm):
        _same(got2[j], want[i], f"permuted row {j} (was {i})")
    # each row alone as a B = 1 rows call
    for b in range(len(wavs)):
        _same(_rows_call(enc, [wavs[b]], [refs[b]])[0], want[b], f"B=1 rows call of row {b}")


def test_limits_are_refused_before_any_launch():
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), C.tiny_bicodec()
    enc = _make(wcfg, tcfg, vcfg, max_seconds=41.0, ref_seconds=1.0)[0]
    rng = np.random.default_rng(5)
    w = [(0.1 * rng.standard_normal(ec.samples_for(t))).astype(np.float32) for t in (9, 30)]
    r = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (400, 129)]
    with pytest.raises(SparkMIError, match=r"code -1.*no rows workspace"):
        _rows_call(enc, w, r, stages=())
    enc.rows_reserve(2, ec.samples_for(30), 400)
    with pytest.raises(SparkMIError, match=r"code -1.*B=3"):
        _rows_call(enc, w + [w[0]], r + [r[0]], stages=())
    long_row = np.zeros(ec.samples_for(31), np.float32)
    with pytest.raises(SparkMIError, match=r"code -1.*n_samples"):
        _rows_call(enc, [w[0], long_row], r, stages=())
    with pytest.raises(SparkMIError, match=r"code -1.*n_ref=128"):                       # n_fft / 2
        _rows_call(enc, w, [r[0], np.zeros(128, np.float32)], stages=())
    with pytest.raises(SparkMIError, match=r"code -1"):                                 # beyond the config's own limits
        enc.rows_reserve(2, enc.max_samples + 1, 400)
    enc.rows_reserve(2, ec.samples_for(2041), 400)
    with pytest.raises(SparkMIError, match=r"code -1.*2041 frames"):
        _rows_call(enc, [w[0], np.zeros(ec.samples_for(2041), np.float32)], r, stages=())
    assert enc.rows_debug_runs() == ([], 0)                                             # nothing was built, nothing launched
    with pytest.raises(ValueError):                                                     # the Python entry: before any device call
        enc.tokenize_rows([np.zeros(enc.max_samples + 1, np.float32)], [r[0]])
    # a valid call on the same handle afterwards
    solo = _make(wcfg, tcfg, vcfg, max_seconds=41.0, ref_seconds=1.0)[0]
    got = _rows_call(enc, w, r, stages=("feat",))
    for b in range(2):
        _same(got[b], _solo_run(solo, w[b], r[b], ("feat",)), f"row {b} after the refusals")


def test_solo_path_is_undisturbed_by_a_rows_call():
    enc, other = _pair(False)
    wavs, refs = _inputs()
    w, r = wavs[3], refs[3]
    first = _solo_run(enc, w, r, ("feat",))          # eager
    second = _solo_run(enc, w, r, ("feat",))         # captured and replayed
    enc.rows_reserve(len(wavs), max(len(x) for x in wavs), max(len(x) for x in refs))
    rows = _rows_call(enc, wavs[:5], refs[:5], ("feat",))
    third = _solo_run(enc, w, r, ("feat",))          # replayed again, after the rows call
    _same(second, first, "replay")
    _same(third, first, "solo after rows")
    _same(rows[3], first, "rows row 3")
    for b in range(5):
        _same(rows[b], {k: _solo(False)[b][k] for k in ("sem", "glob", "feat")}, f"rows row {b}")


def test_solo_list_is_the_one_row_rows_list():
    """build-only: smi_enc_forward's list is the rows builder's list of that one row, launch record by launch record"""
    enc = _pair(False)[0]
    wavs, refs = _inputs()
    enc.rows_reserve(len(wavs), max(len(w) for w in wavs), max(len(r) for r in refs))
    for t, r in zip(FRAMES, N_REF):
        n = ec.samples_for(t)
        frames, count = enc.debug_build(n, r)
        solo = enc.debug_launches()
        rframes, rcount, starts = enc.rows_debug_build([n], [r])
        rows = enc.rows_debug_launches()
        assert (frames, count, starts) == (t, rcount, [0]) and rframes == [t] and len(solo) == len(rows) == count > 0
        for a, b in zip(solo, rows):
            for field in ("index", "name", "kind", "grid", "block", "lds", "cpt"):
                assert a[field] == b[field], (t, r, field, a, b)
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), C.tiny_bicodec()
    long_enc = _make(wcfg, tcfg, vcfg, max_seconds=41.0, ref_seconds=1.0)[0]
    with pytest.raises(SparkMIError, match=r"code -1.*2041 frames"):
        long_enc.debug_build(ec.samples_for(2041), 200)
    assert long_enc.launches() == 0 and long_enc.debug_launches() == []                # refused before anything was built


def test_graph_cache_round_robin():
    """Ten (samples, reference samples) keys on one handle that caches eight graphs, each encoded three times in round-robin
    order.  Round one runs every key eagerly; round two captures every key, and the ninth and tenth captures evict the two least
    recently used graphs; round three finds its key evicted every time (ten keys through eight entries, oldest first), so it
    captures again and evicts in turn; a last pass over the eight keys then cached replays them.  A rows call sits between rounds
    two and three.  Every result (sem, glob, feat) carries the bits of its key's first."""
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), C.tiny_bicodec()
    enc = _make(wcfg, tcfg, vcfg, max_seconds=1.0, ref_seconds=1.0)[0]
    rng = np.random.default_rng(19)
    keys = [(ec.samples_for(2 + i), 129 + i) for i in range(10)]
    wavs = [(0.1 * rng.standard_normal(n) + 0.01).astype(np.float32) for n, _ in keys]
    refs = [(0.2 * rng.standard_normal(r)).astype(np.float32) for _, r in keys]
    first = [_solo_run(enc, w, r, ("feat",)) for w, r in zip(wavs, refs)]
    for i, f in enumerate(first):
        assert f["sem"].shape == (2 + i,)
    for rnd in (2, 3):
        if rnd == 3:
            enc.rows_reserve(3, max(len(w) for w in wavs), max(len(r) for r in refs))
            for j, got in zip((9, 0, 4), _rows_call(enc, [wavs[j] for j in (9, 0, 4)], [refs[j] for j in (9, 0, 4)], ("feat",))):
                _same(got, first[j], f"rows call, key {j}")
        for i in range(10):
            _same(_solo_run(enc, wavs[i], refs[i], ("feat",)), first[i], f"round {rnd}, key {i}")
    for i in range(2, 10):
        _same(_solo_run(enc, wavs[i], refs[i], ("feat",)), first[i], f"replay, key {i}")


def test_tokenize_rows_returns_the_callers_order():
    enc = _pair(False)[0]
    wavs, refs = _inputs()
    out = enc.tokenize_rows(list(wavs), list(refs))
    torch.cuda.synchronize()
    for b, (g, s) in enumerate(out):
        assert g.shape == (1, 1, enc.tcfg.spk_token_num) and g.dtype == torch.int32 and s.shape == (1, FRAMES[b]) and s.dtype == torch.int64
        assert np.array_equal(s.cpu().numpy()[0], _solo(False)[b]["sem"]) and np.array_equal(g.cpu().numpy().reshape(-1), _solo(False)[b]["glob"])
    res = enc._rows_reserved
    enc.tokenize_rows(list(wavs[:2]), list(refs[:2]))                                  # fits: no new reservation
    assert enc._rows_reserved == res


def test_full_size_rows_equal_solo_bits():
    """xlsr-53 and the 0.5B BiCodec: 1.0, 2.9, 3.0 and 6.0 s in one call"""
    wcfg, tcfg, vcfg = T.xlsr53(), T.spark_0p5b_tok(), C.spark_0p5b_bicodec()
    from sparkmi.encoder import BiCodecEncoder
    wsd = W.wav2vec2_state(wcfg)
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", max_seconds=6.0, ref_seconds=6.0, diag=True)
    solo = BiCodecEncoder(wcfg, tcfg, None, None, "cuda:0", max_seconds=6.0, ref_seconds=6.0, arena=enc.arena, diag=True)
    rng = np.random.default_rng(3)
    wavs = [(0.1 * rng.standard_normal(int(16000 * s))).astype(np.float32) for s in (1.0, 2.9, 3.0, 6.0)]
    refs = [get_ref_clip(w.astype(np.float64), 16000, 6.0, tcfg.hop_length).astype(np.float32) for w in wavs]
    enc.rows_reserve(4, 96000, max(len(r) for r in refs))
    got = _rows_call(enc, wavs, refs, ("feat",))
    print(f"RUNS full size run starts={enc.rows_debug_runs()[0]} launches={enc.rows_debug_runs()[1]}")
    for b in range(4):
        _same(got[b], _solo_run(solo, wavs[b], refs[b], ("feat",)), f"row {b}")


def _write_wav(path, x, sr=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())


def test_pipeline_prompt_encode_rows_equals_streams(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_rows")
    synthetic.make_model_dir(d)
    paths = []
    for i, (f0, secs) in enumerate(((150.0, 1.3), (210.0, 2.1))):
        t = np.arange(int(16000 * secs)) / 16000.0
        x = 0.3 * np.sin(2 * np.pi * f0 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.0 * t)) + 0.01 * np.random.default_rng(i).standard_normal(len(t))
        p = d / f"prompt{i}.wav"
        _write_wav(p, x)
        paths.append(str(p))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    reqs = [dict(text="First speaker.", prompt_speech_path=paths[0], prompt_text="one"),
            dict(text="Second speaker, a little longer.", prompt_speech_path=paths[1], prompt_text=None)]
    for (g, s), (g1, s1) in zip(tts.audio_tokenizer.tokenize_rows(paths), tts.audio_tokenizer.tokenize_many(paths)):
        assert torch.equal(g, g1) and torch.equal(s, s1)
    a = tts.inference_batch(reqs, do_sample=False, max_new_tokens=30, prompt_encode="rows")
    b = tts.inference_batch(reqs, do_sample=False, max_new_tokens=30, prompt_encode="streams")
    c = tts.inference_batch(reqs, do_sample=False, max_new_tokens=30)
    for x, y, z in zip(a, b, c):
        assert x.shape == y.shape and np.array_equal(x, y) and np.array_equal(y, z)
    with pytest.raises(ValueError, match="prompt_encode"):
        tts.inference_batch(reqs, do_sample=False, max_new_tokens=30, prompt_encode="x")


# ------------------------------------------------------------------------------------------------------------------------
# Each small kernel in its batched form: ONE launch of a rows list over three rows, against the float64 restatements and
# bounds of tests/enc_cases.py.  The rows are written through the diagnostics with the row stride the launch uses (the longest
# row of the run); columns beyond a row's own length hold a sentinel on both sides of the launch -- an input the kernel must
# not read (it would show in the result) and an output it must not write -- and so does the whole of a fourth, unused row slot.
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ktiny(spk=8):
    wcfg, tcfg, vcfg = ec.tiny_cfgs(spk_token_num=spk, perceiver_heads=2)
    return _make(wcfg, tcfg, vcfg, max_seconds=6.0, ref_seconds=1.5) + (wcfg, tcfg)


def _build3(enc, ns, nr):
    """the rows list of three rows in a workspace of four; all three must share one run (one launch of every kernel)"""
    enc.rows_reserve(4, max(ns), max(nr))
    frames, _, starts = enc.rows_debug_build(ns, nr)
    assert starts == [0], starts
    return frames


def _put(enc, row, buf, arr, ext=None, offset=0):
    """arr [C][T] into row `row`'s buffer at row stride ext, sentinel beyond T"""
    arr = np.asarray(arr, np.float32)
    if arr.ndim == 1 or ext is None:
        enc.rows_debug_io(row, buf, arr, offset=offset)
        return
    full = np.full((arr.shape[0], ext), SENTINEL)
    full[:, : arr.shape[1]] = arr
    enc.rows_debug_io(row, buf, full, offset=offset)


def _blank(enc, buf, n, rows=4):
    for r in range(rows):
        enc.rows_debug_io(r, buf, np.full(n, SENTINEL))


def _get(enc, row, buf, C_, T_, ext, offset=0):
    """row `row`'s [C_][T_] block of a buffer of row stride ext; the columns beyond T_ must still hold the sentinel"""
    a = enc.rows_debug_io(row, buf, count=C_ * ext, offset=offset).reshape(C_, ext)
    assert (a[:, T_:] == SENTINEL).all(), f"{buf} row {row}: columns beyond {T_} were written"
    return a[:, :T_]


def _untouched(enc, buf, n):
    assert (enc.rows_debug_io(3, buf, count=n) == SENTINEL).all(), f"{buf}: the unused fourth row slot was written"


def _rl(enc, name):
    """runs the one launch of that name once; every small kernel's grid z is the three rows"""
    hits = [l for l in enc.rows_debug_launches() if l["name"] == name]
    assert len(hits) == 1 and hits[0]["kind"] == 9 and hits[0]["grid"][2] == 3, (name, hits)
    enc.rows_debug_run(hits[0]["index"])
    return hits[0]


def _accept(kernel, case, got, ref, bnd):
    ok, r = ec.accept(got, ref, bnd)
    print(f"RATIO rows {kernel} {case} worst error/bound {r:.4f}")
    assert ok, f"{kernel} {case}: worst |got - ref| / bound = {r}"


def test_rows_wavnorm_and_conv0():
    enc, _, wf, _, wcfg, _ = _ktiny()
    names = ("n720", "n1025", "n32123")
    xs = [ec.wavnorm_inputs(n) for n in names]
    ns = [len(x) for x in xs]
    assert ns == [720, 1025, 32123]
    _build3(enc, ns, [200] * 3)
    _blank(enc, "wavn", max(ns) + 8)
    for r, x in enumerate(xs):
        _put(enc, r, "in_wav", np.concatenate([x, np.full(8, SENTINEL)]))
    l = _rl(enc, "w2v.normalize")
    assert l["grid"] == (1, 1, 3) and l["block"] == 1024
    for r, x in enumerate(xs):
        got = enc.rows_debug_io(r, "wavn", count=len(x) + 8)
        assert (got[len(x):] == SENTINEL).all()
        _accept("k_wavnorm", names[r], got[: len(x)], ec.wavnorm_ref(x), ec.wavnorm_bound(x))
    _untouched(enc, "wavn", max(ns) + 8)
    # k_conv0: T0 = 255, 256, 591
    T0s = [255, 256, 591]
    ns = [5 * (t - 1) + 10 for t in T0s]
    _build3(enc, ns, [200] * 3)
    CD, ext = wcfg.conv_dim[0], max(T0s)
    _blank(enc, "cf0", CD * ext)
    xs = [ec.normal(f"conv0.rows.{t}", n) for t, n in zip(T0s, ns)]
    for r, x in enumerate(xs):
        _put(enc, r, "wavn", np.concatenate([x, np.full(8, SENTINEL)]))
    l = _rl(enc, "w2v.conv0")
    assert l["grid"] == ((ext + 255) // 256, CD, 3) and l["block"] == 256
    for r, (x, t) in enumerate(zip(xs, T0s)):
        ref, mag = ec.conv0_ref(x, wf["feature_extractor.conv_layers.0.conv.weight"][:, 0], wf["feature_extractor.conv_layers.0.conv.bias"], 5, t)
        _accept("k_conv0", f"T0={t}", _get(enc, r, "cf0", CD, t, ext), ref, ec.conv0_bound(mag, 10))
    _untouched(enc, "cf0", CD * ext)


def test_rows_posconv_and_tap():
    enc, _, wf, _, wcfg, _ = _ktiny()
    H = wcfg.hidden_size
    Ts = [2, 64, 65]
    _build3(enc, [ec.samples_for(t) for t in Ts], [200] * 3)
    ext = 65
    xs = [ec.normal(f"posconv.rows.{t}", (H, t)) for t in Ts]
    _blank(enc, "h", H * ext)
    for r, x in enumerate(xs):
        _put(enc, r, "x", x, ext)
    l = _rl(enc, "w2v.pos_conv+gelu+res")
    assert l["grid"] == (2, H // 16, 3) and l["lds"] == ec.posconv_lds(32, 16)
    Wp, bp = wf["encoder.pos_conv_embed.conv.weight"], wf["encoder.pos_conv_embed.conv.bias"]
    for r, (x, t) in enumerate(zip(xs, Ts)):
        ref, pre, mag = ec.posconv_ref(x, Wp, bp, wcfg.num_conv_pos_embedding_groups)
        _accept("k_posconv", f"T={t}", _get(enc, r, "h", H, t, ext), ref, ec.posconv_bound(x, pre, mag, 32 * 16))
    _untouched(enc, "h", H * ext)
    # k_tap, three modes, T = 2, 9, 65: the row stride (65) is not the row's own T
    Ts = [2, 9, 65]
    _build3(enc, [ec.samples_for(t) for t in Ts], [200] * 3)
    a, b, c = wcfg.taps
    hs = [ec.normal(f"tap.rows.h.{t}", (H, t)) for t in Ts]
    accs = [ec.normal(f"tap.rows.acc.{t}", (H, t), 2.0) for t in Ts]
    _blank(enc, "acc", H * ext); _blank(enc, "feat", H * ext); _blank(enc, "h", H * ext)
    for r in range(3):
        _put(enc, r, "h", hs[r], ext)
    l = _rl(enc, f"w2v.tap{a}")
    assert l["grid"] == (1, H, 3) and l["block"] == 256
    for r, t in enumerate(Ts):
        assert ec.accept_equal(_get(enc, r, "acc", H, t, ext), hs[r])
    for r in range(3):
        _put(enc, r, "acc", accs[r], ext)
    _rl(enc, f"w2v.tap{b}")
    for r, t in enumerate(Ts):
        _accept("k_tap", f"mode 1 T={t}", _get(enc, r, "acc", H, t, ext), ec.tap_ref(hs[r], accs[r], 1), ec.tap_bound(hs[r], accs[r], 1))
    for r in range(3):
        _put(enc, r, "acc", accs[r], ext)
    _rl(enc, f"w2v.tap{c}")
    for r, t in enumerate(Ts):
        _accept("k_tap", f"mode 2 T={t}", _get(enc, r, "feat", H, t, ext), ec.tap_ref(hs[r], accs[r], 2), ec.tap_bound(hs[r], accs[r], 2))
        assert ec.accept_equal(_get(enc, r, "acc", H, t, ext), accs[r])
    for buf in ("acc", "feat"):
        _untouched(enc, buf, H * ext)


def test_rows_mha_self_attention():
    enc = _ktiny()[0]
    Ts = [9, 65, 257]
    _build3(enc, [ec.samples_for(t) for t in Ts], [200] * 3)
    ext = 257
    _blank(enc, "att", 128 * ext)
    qkv = [ec.mha_inputs(f"rows.self.{t}", 2, t, t)[:3] for t in Ts]
    for r, (q, k, v) in enumerate(qkv):
        _put(enc, r, "wide", np.concatenate([q, k, v], axis=0), ext)
    l = _rl(enc, "w2v.encoder.layers.0.attention")
    assert l["grid"] == ((ext + 7) // 8, 2, 3) and l["block"] == 256 and l["lds"] == ec.mha_lds(ext)   # LDS sized by the longest row
    for r, ((q, k, v), t) in enumerate(zip(qkv, Ts)):
        ref, _, bnd = ec.mha_ref(q, k, v, 2)
        _accept("k_mha", f"self T={t}", _get(enc, r, "att", 128, t, ext), ref, bnd)
    _untouched(enc, "att", 128 * ext)


def test_rows_mha_cross_attention():
    Nt, heads = 5, 2
    enc = _ktiny(Nt)[0]
    Tks = [11, 73, 269]
    nr = [ec.REF_HOP * (tk - Nt - 1) + 5 for tk in Tks]
    _build3(enc, [ec.samples_for(2)] * 3, nr)
    ext, inner = 269, heads * 64
    _blank(enc, "po", inner * Nt)
    qkv = [ec.mha_inputs(f"rows.cross.{tk}", heads, Nt, tk)[:3] for tk in Tks]
    for r, (q, k, v) in enumerate(qkv):
        _put(enc, r, "pq", q.reshape(-1))
        _put(enc, r, "pkv", np.concatenate([k, v], axis=0), ext)
    l = _rl(enc, PS + ".layers.0.0.attend")
    assert l["grid"] == (1, heads, 3) and l["lds"] == ec.mha_lds(ext)
    for r, ((q, k, v), tk) in enumerate(zip(qkv, Tks)):
        ref, _, bnd = ec.mha_ref(q, k, v, heads)
        _accept("k_mha", f"cross Nt={Nt} Tk={tk}", enc.rows_debug_io(r, "po", count=inner * Nt).reshape(inner, Nt), ref, bnd)
    _untouched(enc, "po", inner * Nt)


def test_rows_frames_magnitude_rowmean_se():
    enc, _, _, _, _, tcfg = _ktiny()
    nfft, hop, nf = tcfg.n_fft, tcfg.hop_length, tcfg.n_fft // 2 + 1
    nr = [129, 800, 1003]
    Tms = [n // hop + 1 for n in nr]
    assert Tms == [2, 11, 13]
    _build3(enc, [ec.samples_for(2)] * 3, nr)
    ext = 13
    _blank(enc, "frames", nfft * ext); _blank(enc, "mag", nf * ext)
    xs = [ec.normal(f"frames.rows.{n}", n, 0.2) for n in nr]
    Ds = [ec.normal(f"mag.rows.{t}", (2 * nf, t), 3.0) for t in Tms]
    for r in range(3):
        _put(enc, r, "in_ref", np.concatenate([xs[r], np.full(8, SENTINEL)]))
        _put(enc, r, "dft", Ds[r], ext)
    l = _rl(enc, "mel.frames")
    assert l["grid"] == (1, nfft, 3)
    _rl(enc, "mel.magnitude")
    for r, t in enumerate(Tms):
        assert ec.accept_equal(_get(enc, r, "frames", nfft, t, ext), ec.frames_ref(xs[r], nfft, hop))
        _accept("k_mag", f"Tm={t}", _get(enc, r, "mag", nf, t, ext), ec.mag_ref(Ds[r]), ec.mag_bound(Ds[r]))
    _untouched(enc, "frames", nfft * ext); _untouched(enc, "mag", nf * ext)
    # k_rowmean / k_se: Tm = 3, 64, 65
    Tms = [3, 64, 65]
    _build3(enc, [ec.samples_for(2)] * 3, [hop * (t - 1) + 5 for t in Tms])
    ext, C_ = 65, tcfg.ecapa_channels
    ys = [ec.normal(f"rowmean.rows.{t}", (C_, t), 1.0, 0.3) for t in Tms]
    xins = [ec.normal(f"se.rows.x.{t}", (C_, t)) for t in Tms]
    ss = [ec.normal(f"se.rows.s.{t}", C_, 0.2, 0.5) for t in Tms]
    _blank(enc, "ec_vec", 4 * (C_ + 128)); _blank(enc, "ec_cat", 3 * C_ * ext)
    for r in range(3):
        _put(enc, r, "ec_b", ys[r], ext)
        _put(enc, r, "ec_a", xins[r], ext)
    l = _rl(enc, SE2 + ".3.mean")
    assert l["grid"] == ((C_ + 3) // 4, 1, 3)
    for r, t in enumerate(Tms):
        vec = enc.rows_debug_io(r, "ec_vec", count=4 * (C_ + 128))
        assert (vec[C_:] == SENTINEL).all()
        _accept("k_rowmean", f"Tm={t}", vec[:C_], ec.rowmean_ref(ys[r]), ec.rowmean_bound(ys[r]))
        _put(enc, r, "ec_vec", ss[r], offset=C_ + 128)
    _untouched(enc, "ec_vec", 4 * (C_ + 128))
    l = _rl(enc, SE2 + ".3.scale+res")
    assert l["grid"] == (1, C_, 3)
    for r, t in enumerate(Tms):
        _accept("k_se", f"Tm={t}", _get(enc, r, "ec_cat", C_, t, ext), ec.se_ref(xins[r], ys[r], ss[r]), ec.se_bound(xins[r], ys[r], ss[r]))
    _untouched(enc, "ec_cat", 3 * C_ * ext)


def test_rows_geglu_rmsnorm_and_fsq():
    Nt, levels = 8, [4] * 6
    wcfg, tcfg, vcfg = ec.tiny_cfgs(spk_token_num=Nt, fsq_levels=list(levels))
    Ld, nd, FI = tcfg.spk_latent_dim, len(levels), tcfg.ff_inner
    Wp, bp = ec.fsq_weights("rows", levels, Ld)
    from sparkmi.encoder import BiCodecEncoder
    wsd = W.wav2vec2_state(wcfg)
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    tsd.update({"speaker_encoder.quantizer.project_in.weight": Wp, "speaker_encoder.quantizer.project_in.bias": bp})
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", diag=True, max_seconds=1.0, ref_seconds=1.0)
    nr = [200, 800, 1003]
    _build3(enc, [ec.samples_for(2), ec.samples_for(3), ec.samples_for(2)], nr)
    Tks = [Nt + n // ec.REF_HOP + 1 for n in nr]
    ext = max(Tks)
    Xs = [ec.normal(f"geglu.rows.{r}", (2 * FI, Nt), 1.5) for r in range(3)]
    ctxs = [ec.normal(f"rmsn.rows.{r}", (Ld, tk), 2.0) for r, tk in enumerate(Tks)]
    _blank(enc, "pg", FI * Nt); _blank(enc, "pout", Ld * Nt)
    for r in range(3):
        _put(enc, r, "pff", Xs[r].reshape(-1))
        _put(enc, r, "pctx", ctxs[r], ext)
    l = _rl(enc, PS + ".layers.0.1.geglu")
    assert l["grid"] == (1, FI, 3) and l["block"] == 64
    l = _rl(enc, PS + ".norm")
    assert l["grid"] == (1, 1, 3) and l["block"] == 64
    g = tsd[PS + ".norm.gamma"]
    for r in range(3):
        _accept("k_geglu", f"row {r}", enc.rows_debug_io(r, "pg", count=FI * Nt).reshape(FI, Nt), ec.geglu_ref(Xs[r], FI), ec.geglu_bound(Xs[r], FI))
        _accept("k_rmsn", f"row {r} Tk={Tks[r]}", enc.rows_debug_io(r, "pout", count=Ld * Nt).reshape(Ld, Nt), ec.rmsn_ref(ctxs[r][:, :Nt], g),
                ec.rmsn_bound(ctxs[r][:, :Nt], g))
    _untouched(enc, "pg", FI * Nt); _untouched(enc, "pout", Ld * Nt)
    # k_fsq_quant: the existing test's checks (tests/test_enc_ops_gpu.py), row by row
    fx = [ec.fsq_inputs(f"rows.{r}", levels, Ld, Nt) for r in range(3)]
    _blank(enc, "fsqb", Nt * 8)
    for r in range(4):
        enc.rows_debug_io(r, "out_glob", np.full(Nt, CANARY, dtype=np.int32))
    for r in range(3):
        _put(enc, r, "pout", fx[r][0].reshape(-1))
    l = _rl(enc, "speaker_encoder.quantizer")
    assert l["grid"] == (1, 1, 3) and l["block"] == 64
    for r, (X, cand) in enumerate(fx):
        got_bd = enc.rows_debug_io(r, "fsqb", count=Nt * nd).reshape(Nt, nd)
        got = enc.rows_debug_io(r, "out_glob", count=Nt, dtype=np.int32)
        exact = np.zeros((Nt, nd), bool)
        for t in cand:
            exact[t, 0] = got_bd[t, 0] == np.float32(-0.5)
        assert exact.any(), f"no probe landed on -0.5: {got_bd[cand, 0]!r}"
        ids, bd, bnd, margin = ec.fsq_ref(X, Wp, bp, levels, exact_half=exact)
        _accept("k_fsq_quant", f"bounded row {r}", got_bd, bd, bnd)
        planted = exact.any(axis=1)
        keep = np.ones(Nt, bool)
        keep[[t for t in cand if not planted[t]]] = False
        ok, excl = ec.accept_ids(got[keep], ids[keep], margin[keep], planted[keep])
        assert ok, f"row {r}: ids differ from the float64 decision (excluded {excl}): {got[keep]} vs {ids[keep]}"
        own = ((np.rint(got_bd.astype(np.float64)) + 2) * 4 ** np.arange(nd)).sum(axis=1).astype(np.int32)
        np.testing.assert_array_equal(got, own)
    assert (enc.rows_debug_io(3, "fsqb", count=Nt * 8) == SENTINEL).all()
    assert (enc.rows_debug_io(3, "out_glob", count=Nt, dtype=np.int32) == CANARY).all()


def test_rows_vq_argmax_ties_and_ragged_codebook():
    ncode, D = 300, 5
    pairs = ec.vq_dup_pairs(ncode)
    cb = ec.vq_codebook("rows", ncode, D, pairs)
    wcfg, tcfg, vcfg = ec.tiny_cfgs(codebook_size=ncode, codebook_dim=D)
    from sparkmi.encoder import BiCodecEncoder
    wsd = W.wav2vec2_state(wcfg)
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    tsd["quantizer.codebook.weight"] = cb
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", diag=True, max_seconds=2.0, ref_seconds=1.0)
    Ts = [2, 9, 65]
    _build3(enc, [ec.samples_for(t) for t in Ts], [200] * 3)
    ext = 65
    Zs = [np.ascontiguousarray(ec.vq_inputs(f"rows.{t}", cb, max(t, 8), pairs)[:, :t]) for t in Ts]   # (vq_inputs plants 1 + 3 frames)
    for r in range(4):
        enc.rows_debug_io(r, "out_sem", np.full(ext, CANARY, dtype=np.int64))
    for r in range(3):
        _put(enc, r, "e0", Zs[r], ext)
    l = _rl(enc, "quantizer.argmax")
    assert l["grid"] == (ext, 1, 3) and l["block"] == 256
    n = len(pairs)
    for r, t in enumerate(Ts):
        got = enc.rows_debug_io(r, "out_sem", count=2 * ext, dtype=np.int64)
        assert (got[t:] == CANARY).all()
        got = got[:t]
        ids, margin, tie = ec.vq_ref(Zs[r], cb)
        assert 0 <= got[0] < ncode
        m = min(n, t - 1)                                        # the duplicated rows the row is long enough to point at
        assert tie[1:1 + m].all() and got[1:1 + m].tolist() == [i for i, _ in pairs][:m], (got[1:1 + m], pairs)   # lowest index of every tie
        ok, excl = ec.accept_ids(got[1:], ids[1:], margin[1:])
        assert ok, f"row {r}: ids differ from the float64 decision (excluded {excl})"
    assert (enc.rows_debug_io(3, "out_sem", count=2 * ext, dtype=np.int64) == CANARY).all()
