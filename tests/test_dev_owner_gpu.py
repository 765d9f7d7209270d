"""Every device allocation of the library has one owner (DevBuf, spark-tts_amd/csrc/smi_common.h), and the owners keep two
process-wide counters -- live buffers, live bytes -- that smi_debug_dev_memory (diagnostics library) reads.  A handle that is
created, driven through every buffer it grows on demand and destroyed must leave both counters where they were: a counter
that does not return is a buffer that bypassed the owner or was never freed."""
import ctypes as C

import numpy as np
import pytest
import torch

from sparkmi import _lib, audio, config as Cf, config_tok as T, weights as W

pytestmark = pytest.mark.gpu

MAX_SLOTS, MAX_POS = 6, 1152


def _counters():
    live, nbytes = C.c_longlong(-1), C.c_longlong(-1)
    assert _lib.diag().smi_debug_dev_memory(C.byref(live), C.byref(nbytes)) == 0
    return live.value, nbytes.value


@pytest.fixture(scope="module")
def tiny_llm():
    """(cfg, weights, arena): one packed arena for every handle of this module (the layout does not depend on the paging)."""
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    cfg = Cf.tiny_llm()
    syn = W.SyntheticLLM(cfg)
    arena = torch.from_numpy(pack_llm_arena(cfg, syn, llm_cfg_struct(cfg, MAX_SLOTS, MAX_POS, "bf16", True))).to("cuda:0")
    return cfg, syn, arena


def _drive_llm(tiny_llm, paged):
    """Create, grow every on-demand buffer, close.  Returns the counters while the handle was live."""
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = tiny_llm
    kw = dict(kv_page_tokens=16, kv_pages=128) if paged else {}
    llm = SparkLLM(cfg, syn, "cuda:0", max_slots=MAX_SLOTS, max_positions=MAX_POS, kv_dtype="bf16", arena=arena, diag=True, **kw)
    rng = np.random.Generator(np.random.PCG64(7))
    prompt = lambda n: rng.integers(0, cfg.vocab_size, size=n).tolist()   # noqa: E731
    llm.session_begin()
    slots = llm.admit([prompt(70)])       # 69 prompt rows in one pass: the big workspace, the split-K slab, the plan, the tiles
    slots += llm.admit([prompt(200)])     # ... and all of them again, larger
    slots += llm.admit([prompt(1030)])    # past one 1024-token attention segment:
    llm.decode(2)                         # the steps' attention runs in segments (the partials buffer)
    slots += llm.admit([prompt(9)], [dict(repetition_penalty=1.3)])   # a penalised admission: its prompt ids' index list
    llm.decode(1)
    toks = llm.slots_tokens(slots, 8)
    assert len(toks) == 4 and all(1 <= len(t) <= 4 for t, _ in toks)   # (a sequence that met its stop id early has fewer)
    if not paged:   # (smi_llm_debug_layer needs a contiguous cache) one temporary of a debug entry point
        hidden = rng.standard_normal((2, cfg.hidden_size)).astype(np.float32)
        out = llm.debug_layer(0, [(0, 0), (1, 0)], hidden, 0)
        assert np.isfinite(out["q"]).all()
    live = _counters()
    llm.close()
    return live


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged16"])
def test_llm_handle_returns_every_buffer(tiny_llm, paged):
    start = _counters()
    for _ in range(2):   # and once more: the second cycle starts from what the first left
        live = _drive_llm(tiny_llm, paged)
        # counted while it lived: the 35 buffers of smi_llm_create (the page table too when paged) and all eleven on-demand ones --
        # the big workspace's six, the split-K slab, the plan, the tiles, the attention partials, the penalty prompt ids
        print(f"paged={paged}: live buffers {live[0] - start[0]}, bytes {live[1] - start[1]}")
        assert live[0] - start[0] >= 35 + int(paged) + 11 and live[1] > start[1], (start, live)
        assert _counters() == start, (start, _counters())


def _vocoder():
    from sparkmi.bicodec import BiCodecVocoder
    vcfg = Cf.tiny_bicodec()
    voc = BiCodecVocoder(vcfg, W.bicodec_detok_state(vcfg), "cuda:0", max_frames=32, diag=True)
    rng = np.random.Generator(np.random.PCG64(2))
    sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 24)))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    assert torch.isfinite(voc.detokenize(sem, glob)).all()
    return voc


def _encoder():
    from sparkmi.encoder import BiCodecEncoder
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), Cf.tiny_bicodec()
    wsd = W.wav2vec2_state(wcfg)
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", max_seconds=1.0, ref_seconds=0.5, diag=True)
    rng = np.random.Generator(np.random.PCG64(3))
    wav = (0.1 * rng.standard_normal(8000)).astype(np.float32)
    n_ref = int(tcfg.sample_rate * 0.25) // tcfg.hop_length * tcfg.hop_length
    glob, sem = enc.tokenize_arrays(wav, wav[:n_ref])
    assert sem.shape[1] == wcfg.frames(8000) and glob.shape[-1] == tcfg.spk_token_num
    return enc


def _resampler():
    a = audio.DeviceAudio("cuda:0", diag=True)
    x = torch.linspace(-1, 1, 4000, device="cuda:0").reshape(1, 4000).contiguous()
    y, n_out = a.resample_rows(x, [4000], [2], [3])
    assert n_out == [audio.out_len(4000, 2, 3)] and torch.isfinite(y).all()
    return a


def _joiner():
    j = audio.StreamJoiner(2, 4000, 5, diag=True)
    x = torch.linspace(-1, 1, 4000, device="cuda:0").reshape(1, 4000).contiguous()
    out, lens = j.push(x, [("a", 4000, True)])
    assert lens == [4000] and torch.isfinite(out).all()
    return j


@pytest.mark.parametrize("make", [_vocoder, _encoder, _resampler, _joiner], ids=["smi_voc", "smi_enc", "smi_rs", "smi_join"])
def test_other_handles_return_every_buffer(make):
    start = _counters()
    for _ in range(2):
        h = make()
        torch.cuda.synchronize()
        live = _counters()
        assert live[0] > start[0] and live[1] > start[1], (start, live)
        h.close()
        assert _counters() == start, (start, _counters())
