"""``oracle.llm_ref.layer_stages_f64`` gathers the call's own K / V rows of a slot with one indexed assignment (the prompt-pass
tests hand it hundreds of rows).  Pinned here to the row-pair loop it replaced, restated below, on a 40-row layout that holds two
runs of consecutive rows next to single rows with cached contexts; ``qkv_only`` returns the same q / k / v."""
import numpy as np


def _attention_by_row_pairs(cfg, rows, q, k, v, kcache, vcache):
    """The previous form: for every row, every row of the call is visited and copied in when it is an earlier position of the slot."""
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    rep = nh // nkv
    attn = np.zeros((len(rows), nh * hd))
    for i, (s, pos) in enumerate(rows):
        K = np.array(kcache[int(s)][: pos + 1], dtype=np.float64) if int(s) in kcache else np.zeros((0, nkv, hd))
        V = np.array(vcache[int(s)][: pos + 1], dtype=np.float64) if int(s) in vcache else np.zeros((0, nkv, hd))
        K = np.concatenate([K, np.zeros((pos + 1 - len(K), nkv, hd))])
        V = np.concatenate([V, np.zeros((pos + 1 - len(V), nkv, hd))])
        for j, (s2, p2) in enumerate(rows):
            if s2 == s and p2 <= pos:
                K[p2], V[p2] = k[j], v[j]
        Kr, Vr = np.repeat(K, rep, axis=1), np.repeat(V, rep, axis=1)
        sc = np.einsum("hd,thd->ht", q[i], Kr) * hd ** -0.5
        pr = np.exp(sc - sc.max(-1, keepdims=True))
        pr /= pr.sum(-1, keepdims=True)
        attn[i] = np.einsum("ht,thd->hd", pr, Vr).reshape(-1)
    return attn


def test_own_rows_gathered_at_once_equal_the_row_pair_loop():
    from oracle.llm_ref import layer_stages_f64
    from sparkmi import config as C, weights as W
    cfg = C.tiny_llm()
    syn = W.SyntheticLLM(cfg)
    w = {n: syn[n] for n in syn.names() if n.startswith("model.layers.1.")}
    rng = np.random.default_rng(40)
    # 40 rows: slot 5 positions 0 .. 11 (a prompt from its start), single rows of slots 0 .. 8 over cached contexts, slot 9
    # positions 20 .. 38 (a run over 20 cached keys), in an order that interleaves the three kinds
    run_a = [(5, t) for t in range(12)]
    run_b = [(9, 20 + t) for t in range(19)]
    singles = [(s, p) for s, p in zip((0, 1, 2, 3, 4, 6, 7, 8, 10), (0, 1, 15, 16, 17, 63, 64, 65, 33))]
    rows = np.array(singles[:4] + run_a + singles[4:7] + run_b + singles[7:], dtype=np.int64)
    assert rows.shape == (40, 2)
    nkv = cfg.num_key_value_heads
    kc, vc = {}, {}
    for s in np.unique(rows[:, 0]):
        n = int(rows[rows[:, 0] == s, 1].min())
        kc[int(s)] = rng.standard_normal((n, nkv, 64)).astype(np.float32)
        vc[int(s)] = rng.standard_normal((n, nkv, 64)).astype(np.float32)
    x = rng.standard_normal((40, cfg.hidden_size)).astype(np.float32)
    got = layer_stages_f64(cfg, w, 1, rows, x, kc, vc)
    want = _attention_by_row_pairs(cfg, rows, got["q"], got["k"], got["v"], kc, vc)
    assert np.array_equal(got["attn"], want)
    assert np.abs(want).max() > 0.1
    only = layer_stages_f64(cfg, w, 1, rows, x, {}, {}, qkv_only=True)
    assert sorted(only) == ["k", "q", "v"] and all(np.array_equal(only[n], got[n]) for n in only)
