"""ORACLE (test infrastructure, never the product path): CPU restatement of the Qwen2
causal-LM forward and HF greedy ``generate`` that ``cli/SparkTTS.py:197-204`` calls.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
this module.  The arithmetic lives in a third-party dependency of the reference
(``transformers==4.46.2`` pinned at ``requirements.txt:12``; 5.15.0 is installed in this image),
not in ``/root/reference``.  Each function cites the ``modeling_qwen2.py`` lines (abbrev. ``MQ``,
transformers 5.15.0) it restates.  Pinning: ``tests/test_oracle_llm.py`` checks this file against
``transformers.Qwen2ForCausalLM`` itself (logits, prefill+decode cache path, greedy tokens) and
against the committed fixtures in ``tests/golden/``.

Plain fp32 torch-CPU ops, B=1 per call (the reference never batches the LM:
``cli/SparkTTS.py:194`` tokenises a single prompt).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F


def _bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


class Qwen2Ref:
    """Weights are a ``name -> fp32 ndarray/tensor`` mapping under HF parameter names."""

    def __init__(self, cfg, weights, kv_dtype: str = "f32"):
        self.cfg = cfg
        self.kv_dtype = kv_dtype  # "f32" (reference behaviour) or "bf16" (emulates the GPU KV cache)
        g = lambda n: torch.as_tensor(np.asarray(weights[n]), dtype=torch.float32)  # noqa: E731
        self.embed = g("model.embed_tokens.weight")
        self.lm_head = self.embed if cfg.tie_word_embeddings else g("lm_head.weight")
        self.final_norm = g("model.norm.weight")
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}."
            self.layers.append(dict(
                ln1=g(p + "input_layernorm.weight"), ln2=g(p + "post_attention_layernorm.weight"),
                wq=g(p + "self_attn.q_proj.weight"), bq=g(p + "self_attn.q_proj.bias"),
                wk=g(p + "self_attn.k_proj.weight"), bk=g(p + "self_attn.k_proj.bias"),
                wv=g(p + "self_attn.v_proj.weight"), bv=g(p + "self_attn.v_proj.bias"),
                wo=g(p + "self_attn.o_proj.weight"),
                wg=g(p + "mlp.gate_proj.weight"), wu=g(p + "mlp.up_proj.weight"),
                wd=g(p + "mlp.down_proj.weight"),
            ))
        d = cfg.head_dim
        # MQ:91-93  inv_freq = 1 / theta^(2i/d)
        self.inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
        self.reset()

    # ------------------------------------------------------------------ pieces
    def reset(self) -> None:
        self.k_cache: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers
        self.v_cache: List[Optional[torch.Tensor]] = [None] * self.cfg.num_hidden_layers
        self.pos = 0

    def rmsnorm(self, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """MQ:247-252: x * rsqrt(mean(x^2) + eps) in fp32, then * weight."""
        var = x.pow(2).mean(-1, keepdim=True)
        return w * (x * torch.rsqrt(var + self.cfg.rms_norm_eps))

    def rope(self, x: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        """MQ:95-102 + MQ:105-133: x*cos + rotate_half(x)*sin on the full head_dim.
        x: (S, H, D); positions: (S,)."""
        freqs = positions.to(torch.float32)[:, None] * self.inv_freq[None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        cos, sin = emb.cos()[:, None, :], emb.sin()[:, None, :]
        h = x.shape[-1] // 2
        rot = torch.cat((-x[..., h:], x[..., :h]), dim=-1)
        return x * cos + rot * sin

    def attention(self, q, k, v, q_pos: torch.Tensor) -> torch.Tensor:
        """MQ:150-173 eager path: repeat_kv, softmax(q k^T * d^-0.5 + causal mask) in fp32, @ v.
        q: (S, Hq, D); k, v: (T, Hkv, D) full cache; q_pos: absolute positions (S,)."""
        cfg = self.cfg
        rep = cfg.num_attention_heads // cfg.num_key_value_heads
        kk = k.repeat_interleave(rep, dim=1)  # (T, Hq, D)  == repeat_kv (MQ:138-147)
        vv = v.repeat_interleave(rep, dim=1)
        scores = torch.einsum("shd,thd->hst", q, kk) * (cfg.head_dim ** -0.5)
        t_idx = torch.arange(k.shape[0])
        mask = t_idx[None, :] > q_pos[:, None]  # key position beyond the query's -> masked
        scores = scores.masked_fill(mask[None], float("-inf"))
        p = torch.softmax(scores, dim=-1, dtype=torch.float32)
        return torch.einsum("hst,thd->shd", p, vv).reshape(q.shape[0], -1)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, ids: Sequence[int], last_only: bool = False,
                return_hidden: bool = False):
        """Append ``ids`` at positions pos..pos+S-1 (KV cache kept) and return logits
        (S, V) (or (1, V) when ``last_only``).  MQ:342-470."""
        cfg = self.cfg
        ids_t = torch.as_tensor(np.asarray(ids), dtype=torch.long)
        S = ids_t.shape[0]
        positions = torch.arange(self.pos, self.pos + S)
        h = self.embed[ids_t]
        hiddens = []
        for li, L in enumerate(self.layers):
            x = self.rmsnorm(h, L["ln1"])
            q = F.linear(x, L["wq"], L["bq"]).view(S, cfg.num_attention_heads, cfg.head_dim)
            k = F.linear(x, L["wk"], L["bk"]).view(S, cfg.num_key_value_heads, cfg.head_dim)
            v = F.linear(x, L["wv"], L["bv"]).view(S, cfg.num_key_value_heads, cfg.head_dim)
            q, k = self.rope(q, positions), self.rope(k, positions)
            if self.kv_dtype == "bf16":
                k, v = _bf16_round(k), _bf16_round(v)
            if self.k_cache[li] is not None:
                k = torch.cat((self.k_cache[li], k), dim=0)
                v = torch.cat((self.v_cache[li], v), dim=0)
            self.k_cache[li], self.v_cache[li] = k, v
            a = self.attention(q, k, v, positions)
            h = h + F.linear(a, L["wo"])
            x = self.rmsnorm(h, L["ln2"])
            # MQ:46-48  down( silu(gate x) * up x )
            h = h + F.linear(F.silu(F.linear(x, L["wg"])) * F.linear(x, L["wu"]), L["wd"])
            if return_hidden:
                hiddens.append(h.clone())
        self.pos += S
        hn = self.rmsnorm(h[-1:] if last_only else h, self.final_norm)
        logits = F.linear(hn, self.lm_head)
        return (logits, hiddens) if return_hidden else logits

    @torch.no_grad()
    def generate_greedy(self, prompt_ids: Sequence[int], max_new_tokens: int,
                        eos_ids: Sequence[int] = ()) -> List[int]:
        """HF ``generate(do_sample=False)`` for one sequence: prefill emits token 1, each
        decode forward emits the next; stops after emitting an EOS id or at
        ``max_new_tokens``.  Returns only the new tokens (the slice the reference takes at
        ``cli/SparkTTS.py:207-210``).  ``torch.argmax`` breaks ties toward the lowest index."""
        self.reset()
        eos = set(int(e) for e in eos_ids)
        logits = self.forward(prompt_ids, last_only=True)
        out: List[int] = []
        for _ in range(max_new_tokens):
            tok = int(torch.argmax(logits[-1]).item())
            out.append(tok)
            if tok in eos or len(out) == max_new_tokens:
                break
            logits = self.forward([tok], last_only=True)
        return out


# ---------------------------------------------------------------------------- one decoder layer, stage by stage, in float64
def rope_angles(cfg, positions) -> np.ndarray:
    """(S, head_dim / 2) RoPE angles as MQ:81-102 forms them: inv_freq and position * inv_freq in fp32 (that rounding is part
    of the model's definition -- the arena's table and transformers share it); cos / sin of them are taken in float64."""
    d = cfg.head_dim
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    pos = torch.as_tensor(np.asarray(positions), dtype=torch.float32)
    return (pos[:, None] * inv_freq[None, :]).numpy().astype(np.float64)


def layer_stages_f64(cfg, weights, layer: int, rows, x, kcache: Dict[int, np.ndarray], vcache: Dict[int, np.ndarray],
                     own_kv: bool = True, qkv_only: bool = False, mlp: bool = True) -> Dict[str, np.ndarray]:
    """One Qwen2 decoder layer (MQ Qwen2DecoderLayer) on M caller rows, every product and sum in float64.

    ``weights``: ``name -> array`` under HF names; ``rows``: (M, 2) (KV slot, position) pairs; ``x``: (M, hidden) residual rows
    entering the layer; ``kcache`` / ``vcache``: slot -> (n, kv heads, head_dim) cached keys (already rotated) / values of
    positions 0 .. n-1.  Row (s, p) attends to positions 0 .. p of slot s: position t is the K/V of the call's own row (s, t)
    when there is one and ``own_kv`` is set, else ``kcache[s][t]`` (``own_kv=False``: the caches already hold the rows' K/V,
    e.g. as a bf16 cache stored them).  Returns what ``SparkLLM.debug_layer`` returns for stages 0-4, in its layouts:
    q (M, heads, hd), k / v (M, kv heads, hd) after bias and RoPE, attn (M, heads * hd), h_mid (M, hidden) after o_proj +
    residual, act (M, intermediate) = silu(gate) * up, h_out (M, hidden) after down_proj + residual.  ``qkv_only``: q, k, v alone
    (the caches are not read); ``mlp=False``: q .. h_mid (the MLP, which never sees the context, is left out)."""
    p = f"model.layers.{layer}."
    w = lambda n: np.asarray(weights[p + n], dtype=np.float64)  # noqa: E731
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    x = np.asarray(x, dtype=np.float64)
    M = rows.shape[0]

    def rms(h, g):                                                   # MQ:247-252
        return g * (h / np.sqrt((h * h).mean(-1, keepdims=True) + cfg.rms_norm_eps))

    def rope(t, ang):                                                # MQ:105-133 (rotate_half on the full head_dim)
        c = np.cos(np.concatenate([ang, ang], -1))[:, None, :]
        s = np.sin(np.concatenate([ang, ang], -1))[:, None, :]
        return t * c + np.concatenate([-t[..., hd // 2:], t[..., : hd // 2]], -1) * s

    xn = rms(x, w("input_layernorm.weight"))
    q = (xn @ w("self_attn.q_proj.weight").T + w("self_attn.q_proj.bias")).reshape(M, nh, hd)
    k = (xn @ w("self_attn.k_proj.weight").T + w("self_attn.k_proj.bias")).reshape(M, nkv, hd)
    v = (xn @ w("self_attn.v_proj.weight").T + w("self_attn.v_proj.bias")).reshape(M, nkv, hd)
    ang = rope_angles(cfg, rows[:, 1])
    q, k = rope(q, ang), rope(k, ang)
    if qkv_only:
        return {"q": q, "k": k, "v": v}
    attn = np.zeros((M, nh * hd))
    rep = nh // nkv
    for i, (s, pos) in enumerate(rows):                              # MQ:150-173 eager attention, GQA by repeat_kv
        K = np.array(kcache[int(s)][: pos + 1], dtype=np.float64) if int(s) in kcache else np.zeros((0, nkv, hd))
        V = np.array(vcache[int(s)][: pos + 1], dtype=np.float64) if int(s) in vcache else np.zeros((0, nkv, hd))
        if own_kv:
            K = np.concatenate([K, np.zeros((pos + 1 - len(K), nkv, hd))])
            V = np.concatenate([V, np.zeros((pos + 1 - len(V), nkv, hd))])
            own = np.flatnonzero((rows[:, 0] == s) & (rows[:, 1] <= pos))     # (a position named twice: the later row's, as a loop would)
            K[rows[own, 1]], V[rows[own, 1]] = k[own], v[own]
        assert K.shape[0] == V.shape[0] == pos + 1, f"row {i} (slot {s}, pos {pos}): keys for {K.shape[0]} positions"
        Kr, Vr = np.repeat(K, rep, axis=1), np.repeat(V, rep, axis=1)          # (T, nh, hd)
        sc = np.einsum("hd,thd->ht", q[i], Kr) * hd ** -0.5
        pr = np.exp(sc - sc.max(-1, keepdims=True))
        pr /= pr.sum(-1, keepdims=True)
        attn[i] = np.einsum("ht,thd->hd", pr, Vr).reshape(-1)
    h_mid = x + attn @ w("self_attn.o_proj.weight").T
    if not mlp:
        return {"q": q, "k": k, "v": v, "attn": attn, "h_mid": h_mid}
    xn2 = rms(h_mid, w("post_attention_layernorm.weight"))
    g = xn2 @ w("mlp.gate_proj.weight").T
    act = g / (1.0 + np.exp(-g)) * (xn2 @ w("mlp.up_proj.weight").T)  # MQ:46-48 silu(gate) * up
    h_out = h_mid + act @ w("mlp.down_proj.weight").T
    return {"q": q, "k": k, "v": v, "attn": attn, "h_mid": h_mid, "act": act, "h_out": h_out}
