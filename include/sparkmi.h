/*
 * sparkmi.h -- C ABI of libsparkmi.so: the MI355X (gfx950) Spark-TTS inference hot path.
 *
 * The reference (arghyasur1991/Spark-TTS) is pure Python and has no FFI of its own; its seams
 * for this path are Python call sites.  Each entry point below names the reference call it
 * stands behind, so a maintainer can bind it (ctypes stub in INTEGRATION.md):
 *
 *   smi_llm_*   <- AutoModelForCausalLM.generate(...)            cli/SparkTTS.py:197-204
 *                  (Qwen2 forward: transformers modeling_qwen2.py, pinned 4.46.2 at requirements.txt:12)
 *   smi_voc_*   <- BiCodec.detokenize(semantic, global)          sparktts/models/bicodec.py:171-189
 *                  via BiCodecTokenizer.detokenize               sparktts/models/audio_tokenizer.py:132-146
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.  Every function returns an int:
 *     0 = SMI_OK, negative = SMI_E*.  smi_last_error() returns a thread-local message.
 *   - "dev" pointers are device (HBM) addresses on the current HIP device, "host" pointers are
 *     ordinary host memory.  `stream` is a hipStream_t passed as void* (0 = default stream).
 *   - The caller owns the weight arenas (they must outlive the handle).  The library owns the
 *     handle, its KV cache and scratch (allocated at create, freed at destroy).
 *   - A handle is bound to the device current at create and may be used by one host thread at
 *     a time.  All launches go to the caller's stream; nothing synchronises unless stated.
 *   - There is no CPU fallback anywhere behind this ABI.
 *   - libsparkmi.so reads NO environment variable.  Timing probes, in-kernel stamps, scratch dumps, A/B switches and the
 *     experimental one-row engine live in libsparkmi_diag.so (the same sources built with -DSMI_DIAG; it exports this
 *     header's symbols plus include/sparkmi_debug.h's) -- tools, the bench probes and the op-level tests load that one.
 */
#ifndef SPARKMI_H
#define SPARKMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMI_OK 0
#define SMI_EINVAL (-1)   /* bad argument / shape outside the kernel contract */
#define SMI_EHIP (-2)     /* a HIP runtime call failed (message has hipGetErrorString) */
#define SMI_ENOMEM (-3)   /* device allocation failed */
#define SMI_ESTATE (-4)   /* call sequence violated (e.g. decode before prefill) */

#define SMI_ABI_VERSION 4   /* 2: eos id LISTS, per-sequence sampler streams; 3: smi_llm_cfg.wd_plain (the W_down tile order is data, not environment);
                              4: diagnostics (timing probes, stamps, scratch dumps, the one-row engine) left this header for sparkmi_debug.h /
                                 libsparkmi_diag.so; the product library reads no environment variable */
#define SMI_MAX_EOS 4      /* eos ids per generation (HF stops on ANY id of generation_config.eos_token_id) */
#define SMI_MAX_ROWS 64   /* rows (= concurrent sequences, or prompt tokens per prefill chunk) per step */

int smi_version(void);
const char* smi_last_error(void);
/* Fills name[0..n) with the device's gcnArchName; fails unless it is a gfx950 part. */
int smi_device_check(char* name, int n);

/* ------------------------------------------------------------------------------------------
 * LLM: Qwen2 decoder-only LM, greedy or sampled generation with a KV cache.
 * ---------------------------------------------------------------------------------------- */
typedef struct smi_llm smi_llm;

typedef struct smi_llm_cfg {
  int32_t vocab_size;        /* config.json: vocab_size */
  int32_t hidden_size;       /* multiple of 32 */
  int32_t num_layers;
  int32_t num_heads;         /* query heads */
  int32_t num_kv_heads;
  int32_t head_dim;          /* must be 64 */
  int32_t intermediate_size; /* multiple of 32 */
  int32_t max_slots;         /* concurrent sequences, 1..SMI_MAX_ROWS */
  int32_t max_positions;     /* tokens (prompt + generated) per sequence */
  int32_t kv_dtype;          /* 0 = bf16 KV cache, 1 = f32 KV cache */
  int32_t use_graph;         /* 1 = replay the decode step as a hipGraph */
  float rms_eps;
  /* Paged KV cache (the functional analogue of TensorRT-LLM's paged KV under in-flight batching,
   * runtime/triton_trtllm/run.sh:50-65): kv_page_tokens = 0 gives every slot max_positions contiguous tokens
   * (max_slots x max_positions reserved).  A power of two in 16..1024 that divides max_positions makes the cache a
   * POOL of kv_pages pages of that many tokens; a sequence holds only the pages its length needs (allocated as it
   * grows, returned at smi_llm_retire / the next prefill), so many live sequences do not each reserve the longest
   * context.  A call that needs more pages than are free fails with SMI_ENOMEM and changes nothing.  Tokens are the
   * same either way. */
  int32_t kv_page_tokens;
  int32_t kv_pages;
  /* Layout of the WD (down_proj) tiles IN THE ARENA the caller packed: 0 (default) = row-part-major [q:4][k8:4][r:4][8],
   * 1 = the plain tile order of the other matrices (kept for A/B: sparkmi/arena.py packs it under SPARKMI_WD_PLAIN=1 and
   * sets this field).  The library reads the layout from here, never from the environment: an arena and the handle that
   * reads it cannot disagree silently. */
  int32_t wd_plain;
  /* Exact-weights verification mode: 1 = the arena holds every matrix as fp32 [N][K] row-major (same row / column orders as
   * the bf16 tiles; 2x the bytes) and every GEMM of the path runs as an exact fp32 multiply-add chain over k
   * (v_mfma_f32_16x16x4_f32), activations exact as always.  For checkpoints SAVED in fp32 -- the published Spark-TTS-0.5B
   * LLM/model.safetensors is: the reference loads it as saved (cli/SparkTTS.py:48-51) and the default bf16 arena ROUNDS it
   * (logits move ~1e-2) -- this mode reproduces the fp32 PyTorch CPU path's greedy tokens (north_star's acceptance sentence
   * on such a checkpoint).  Opt-in and slow (~4x the step time at one row); 0 (default) = bf16 weights, north_star's arithmetic. */
  int32_t weights_exact;
} smi_llm_cfg;

/* Arena sections.  The arena is one device buffer the caller fills (see sparkmi/arena.py):
 *   matrices: bf16, rows grouped into 16-row x 32-col tiles stored [n_tile][k_tile][k8:4][n:16][8]
 *             (one tile = 1 KiB = exactly one wave64 x 16-byte load = one MFMA 16x16x32 A operand);
 *   QKV rows: q heads, then k heads, then v heads; inside each q/k head the 64 rows are ordered
 *             (0,32,1,33,...) so a RoPE pair sits in adjacent rows; QKV bias in the same order;
 *   WO columns (the attention output it multiplies): 32-column k tiles head-interleaved -- tile (half * num_heads + head)
 *             holds dims 32*half .. 32*half+31 of that head (sparkmi/arena.py: o_proj_col_perm);
 *   GATE_UP rows: gate and up interleaved (g0,u0,g1,u1,...);
 *   WD (down_proj) tiles: the 64 pieces of a tile are stored row-part-major [q:4][k8:4][r:4][8] (row n = 4q + r) instead
 *             of [k8:4][n:16][8]: the row-split down_proj kernels (4 or 8 rows of a tile per block) then read whole
 *             128-byte lines (sparkmi/arena.py: pack_tiles(row_parts=True));
 *   LM_HEAD: vocab padded up to a multiple of 16 rows with zeros (also the embedding table);
 *   norms/bias: f32;  ROPE: float2 (cos,sin) [max_positions][head_dim/2].                      */
enum smi_llm_section {
  SMI_LLM_LN1 = 0, SMI_LLM_WQKV, SMI_LLM_BQKV, SMI_LLM_WO, SMI_LLM_LN2, SMI_LLM_WGU, SMI_LLM_WD, /* per layer */
  SMI_LLM_FINAL_NORM, SMI_LLM_LM_HEAD, SMI_LLM_ROPE, SMI_LLM_TAG,                               /* layer = 0 */
  SMI_LLM_NUM_SECTIONS
};
/* SMI_LLM_TAG: 256 bytes the packer fills with a smi_llm_arena_tag.  smi_llm_create reads it back from the device and refuses
 * an arena that was packed for another ABI version, other dimensions or another W_down tile order than the config it is given
 * says: a packed arena and the handle that streams it cannot disagree silently (an arena re-used under a different
 * SPARKMI_WD_PLAIN setting used to give wrong logits with no error). */
typedef struct smi_llm_arena_tag {
  char magic[8];             /* "SMIARENA" */
  int32_t abi_version;       /* SMI_ABI_VERSION of the packer */
  int32_t wd_plain;          /* = smi_llm_cfg.wd_plain the matrices were packed with */
  int32_t vocab_size, hidden_size, num_layers, num_heads, num_kv_heads, intermediate_size, max_positions;
  int32_t weights_exact;     /* = smi_llm_cfg.weights_exact: fp32 [N][K] matrices instead of bf16 tiles */
  int32_t reserved[52];
} smi_llm_arena_tag;
/* Total arena size in bytes for this config (0 on invalid config). */
size_t smi_llm_arena_bytes(const smi_llm_cfg* cfg);
/* Byte offset and byte size of one section; returns SMI_EINVAL for a bad section/layer. */
int smi_llm_arena_section(const smi_llm_cfg* cfg, int section, int layer, size_t* offset, size_t* bytes);

int smi_llm_create(const smi_llm_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_llm** out);
int smi_llm_destroy(smi_llm* h);

/* Start B sequences (slots 0..B-1): run the prompts through the model (KV cache filled) and emit
 * each sequence's first new token (generate()'s prefill forward + argmax).
 *   ids_host:  [B][P_max] int64 prompt ids, right-padded;  lens_host: [B] prompt lengths (>= 1).
 *   eos_ids_host / n_eos: a sequence stops counting tokens after emitting ANY of these ids, as HF generate()
 *              does with every id of generation_config.json's eos_token_id (cli/SparkTTS.py:197-204 passes none
 *              itself); 0 <= n_eos <= SMI_MAX_EOS, n_eos = 0: never stop.                          */
int smi_llm_prefill(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int B, int P_max,
                    const int64_t* eos_ids_host, int n_eos, void* stream);
/* Token selection for the following prefill/decode calls.  do_sample = 0: greedy argmax (lowest id
 * on ties, like torch.argmax).  do_sample = 1: the reference's default at cli/SparkTTS.py:197-204 --
 * temperature, then top-k (1..256), then nucleus top-p, one multinomial draw per step from a
 * Philox stream keyed by (seed; the sequence's admission number, its own token index): reproducible per
 * seed whatever else is in the batch, statistically (not bitwise) equivalent to transformers' sampler.
 * Ids that tie with the k-th largest logit all stay, as in TopKLogitsWarper (-0.0 ties with +0.0), up to the 256 ranks the
 * sampler sorts: of more survivors, the 256 first in (logit descending, id ascending) order are the ones drawn from.  A -inf
 * logit is never drawn; a row with no finite logit gives token 0.  The draw itself is exact integer arithmetic and an exactly
 * sorted inverse CDF: tests/sample_ref.py names the token of every draw and tests/test_sample_draws_gpu.py holds the kernels
 * to it. */
int smi_llm_set_sampling(smi_llm* h, int do_sample, float temperature, int top_k, float top_p, uint64_t seed);
/* Run n_steps more decode steps for all B sequences (finished ones keep stepping; their
 * tokens are not counted).  Asynchronous. */
int smi_llm_decode(smi_llm* h, int n_steps, void* stream);
/* Synchronises the stream; *all_done = 1 when every sequence has emitted eos. */
int smi_llm_all_done(smi_llm* h, int* all_done, void* stream);
/* Synchronises; copies the generated ids: out_host [B][cap] int64 (row b holds lens_host[b] ids,
 * the eos included when one was emitted). */
int smi_llm_get_tokens(smi_llm* h, int64_t* out_host, int32_t* lens_host, int cap, void* stream);
/* Continuous (in-flight) batching: sequences join and leave between decode steps, each in its own KV slot;
 * the functional analogue of the reference's Triton / TensorRT-LLM in-flight batching
 * (runtime/triton_trtllm/run.sh:50-65).  smi_llm_session_begin starts an empty session; smi_llm_admit
 * prefills n new prompts into free slots (returned in slots_out) and emits their first token without
 * touching the live sequences; smi_llm_decode then steps every live sequence; smi_llm_slot_tokens reads one
 * sequence's tokens so far and whether it has produced eos; smi_llm_retire frees its slot.  A sequence's
 * tokens do not depend on what else is live, was admitted with it or shares its call: rows are independent in every decode
 * kernel and every decode path (row-grouped GEMMs, chain-split down_proj, one-row kernels) sums a row in the same order, and the
 * kernels its PROMPT rows run through are chosen from ITS OWN length alone (up to SMI_MAX_ROWS rows: the decode kernels; more:
 * the prefill GEMM family, whose few-row and many-row shapes sum o_proj / down_proj in the same K segments in the same order),
 * each class of a call in its own pass -- bit for bit, with either KV cache type (tests/test_fullsize_gpu.py: 32 of 32 rows,
 * prompts of 3 .. 600 tokens in one call against every sequence alone, K rows compared).  Round 3 chose the prompt kernels
 * from the call's TOTAL rows; with the bf16 cache a last-bit difference between two kernels could then move a K/V element to
 * the neighbouring bf16 value and flip a near-tie arg-max between two batch compositions. */
int smi_llm_session_begin(smi_llm* h, const int64_t* eos_ids_host, int n_eos, void* stream);
int smi_llm_admit(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max, int32_t* slots_out, void* stream);
/* Per-request token selection (TensorRT-LLM's per-request temperature / runtime_top_k / runtime_top_p / random_seed inputs,
 * runtime/triton_trtllm/model_repo/tensorrt_llm/config.pbtxt:160-251).  smi_llm_admit_sampled takes one record per prompt; the
 * library keeps it per KV slot in device memory next to the sequence's admission number, so records of any mix ride the same
 * captured decode step (nothing of them is a kernel argument; the step graph only knows whether SOME live row may sample).
 *   SMI_SAMPLING_INHERIT: smi_llm_set_sampling's settings and stream, bit for bit what smi_llm_admit gives.
 *   SMI_SAMPLING_GREEDY:  arg-max, lowest id on ties -- the greedy path's bits, even while the handle samples.
 *   SMI_SAMPLING_SAMPLE:  this record's temperature (> 0), top_k (1..256) and top_p (0, 1].  has_seed = 1: the draws come from a
 *                         Philox stream keyed by (seed; the sequence's own token index) alone, so its tokens do not depend on its
 *                         slot, on what else is live or was admitted with it, on the admission order or on the handle -- the
 *                         random_seed contract (the stream's counter carries a marker no admission number takes, so it never
 *                         meets an inheriting row's stream).  has_seed = 0: the handle's seed and smi_llm_set_sampling's key
 *                         (seed; admission number, token index).
 * Other fields are ignored outside SMI_SAMPLING_SAMPLE.  params = NULL: every prompt inherits (= smi_llm_admit).  Every record
 * is checked before anything of the handle is touched: a bad one fails the call with SMI_EINVAL and takes no slot, KV page
 * or admission number. */
#define SMI_SAMPLING_INHERIT 0
#define SMI_SAMPLING_GREEDY 1
#define SMI_SAMPLING_SAMPLE 2
typedef struct smi_sample_params {
  int32_t mode;          /* SMI_SAMPLING_* */
  float temperature;
  int32_t top_k;
  float top_p;
  uint64_t seed;
  int32_t has_seed;      /* 0 or 1 */
  int32_t reserved;      /* 0 */
} smi_sample_params;
int smi_llm_admit_sampled(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                          const smi_sample_params* params, int32_t* slots_out, void* stream);
/* Per-request logits penalties (TensorRT-LLM's per-request repetition_penalty / presence_penalty / frequency_penalty /
 * min_length inputs).  smi_llm_admit_penalized = smi_llm_admit_sampled plus one penalty record per prompt (pens = NULL: exactly
 * smi_llm_admit_sampled), kept per KV slot in device memory like the sampling record.  Before token selection, a penalised
 * row's fp32 logits x go through, in this order:
 *   1. repetition_penalty r > 0 (transformers' RepetitionPenaltyLogitsProcessor): every id of the row's history becomes
 *      x < 0 ? x * r : x / r (IEEE fp32 product / quotient, once per distinct id).  History = prompt + generated tokens with
 *      penalize_prompt = 1 (transformers' default), the generated tokens alone with 0 (its prompt_ignore_length = len(prompt);
 *      what voice cloning wants: the prompt holds the reference clip's semantic tokens).
 *   2. presence_penalty p and frequency_penalty f in [-2, 2] (the OpenAI / vLLM additive form): with c = occurrences of the id
 *      among the GENERATED tokens, x - (f * c + p * (c > 0 ? 1 : 0)), each operation fp32, in this order.
 *   3. min_new_tokens n (transformers' MinNewTokensLengthLogitsProcessor): every id of the session's eos list is -inf while the
 *      sequence has emitted fewer than n tokens (the first token, emitted by the admission, is token 0).
 *   4. selection as without penalties, on the processed logits: arg-max (lowest id on ties), or temperature -> top-k -> top-p
 *      -> draw (transformers' processors-before-warpers order).
 * A record with r = 1, p = f = 0 and n = 0 is neutral: that row is not penalised and its tokens are the bits it gets without
 * the record.  Checked before anything of the handle is touched (SMI_EINVAL, no slot, page or admission number taken):
 * r finite and > 0, p and f finite in [-2, 2], 0 <= n <= max_positions, penalize_prompt 0 or 1, reserved 0. */
typedef struct smi_penalty_params {
  float repetition_penalty;    /* r; 1 = off */
  float presence_penalty;      /* p; 0 = off */
  float frequency_penalty;     /* f; 0 = off */
  int32_t min_new_tokens;      /* n; 0 = off */
  int32_t penalize_prompt;     /* 0 or 1 */
  int32_t reserved[3];         /* 0 */
} smi_penalty_params;
int smi_llm_admit_penalized(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                            const smi_sample_params* params, const smi_penalty_params* pens, int32_t* slots_out, void* stream);
/* Per-token log-probabilities (TensorRT-LLM's return_log_probs -> output_log_probs / cum_log_probs).
 * smi_llm_admit_logprobs = smi_llm_admit_penalized plus one 0/1 flag per prompt (return_log_probs = NULL: exactly
 * smi_llm_admit_penalized).  For every token a flagged sequence emits -- the admission's first token and an eos included --
 * the library keeps one fp32 value
 *     lp = z[tok] - logsumexp(z), over the full vocabulary,
 * where z is the logits token selection saw: the lm_head's fp32 logits after the row's allowed-token stage 0
 * (smi_llm_admit_constrained: -inf outside the set, so the values are normalised over the allowed ids) and penalties
 * (stages 1-3 above, the -inf of min_new_tokens included), multiplied by the row's 1/temperature when the row samples (its record's, or the handle's for
 * an inheriting row of a sampling handle).  In transformers' terms: log_softmax of the scores after the logits processors
 * and TemperatureLogitsWarper, before TopK / TopP.  A greedy, unpenalised row gets the model's own log_softmax(logits)[tok].
 * The value is NOT renormalised over the top-k / top-p survivors (that variant is not provided); a sampled token's value is
 * always finite, since top-k / top-p only remove ids and do not change z.  A flag other than 0 / 1 is SMI_EINVAL, checked
 * with the other records before anything of the handle is touched (no slot, page or admission number taken).
 * smi_llm_slots_logprobs mirrors smi_llm_slots_tokens: out_host [n][cap] (the first n_out[i] values of row i, one per token
 * of smi_llm_slots_tokens), one round trip; a retired slot stays readable until a later admission reuses it; a slot whose
 * sequence was admitted without the flag is SMI_ESTATE.  Static generation (smi_llm_prefill) keeps no log-probabilities. */
int smi_llm_admit_logprobs(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                           const smi_sample_params* params, const smi_penalty_params* pens, const int32_t* return_log_probs,
                           int32_t* slots_out, void* stream);
int smi_llm_slots_logprobs(smi_llm* h, const int32_t* slots, int n, float* out_host, int cap, int32_t* n_out, void* stream);
/* Several takes of one prompt (TensorRT-LLM's num_return_sequences): n_return[b] >= 1 takes of prompt b.  Output sequences are
 * prompt-major: prompt 0's takes, then prompt 1's, ...  N = sum(n_return).  params / pens / return_log_probs hold one entry per
 * OUTPUT sequence ([N]; NULL as in smi_llm_admit_logprobs).  slots_out [N].
 *   Equivalence: the call equals smi_llm_admit_logprobs of the expanded prompt list, in which prompt b appears n_return[b]
 *     times in a row, with the same records -- bit for bit in the slots returned (lowest free slots, in order), the admission
 *     numbers given out, every token and log-probability, and every K/V element at every position, with either cache dtype,
 *     contiguous or paged.  n_return = NULL or all ones: exactly smi_llm_admit_logprobs.
 *   Prefill work: each distinct prompt's prompt rows (all its tokens but the last) run once, in the slot of its first take
 *     (its leader), through the kernels its own length selects; the leader's K/V rows 0 .. L-2 then reach the other takes
 *     (k_kv_fork), and one step over all N rows emits every take's first token with its own record.
 *   Paged cache (page size P, prompt length L): the followers share the leader's first S = floor((L-1)/P) pages read-only
 *     (they hold positions < S P <= L-1, which no later step writes); every take owns its pages from page S on, and positions
 *     S P .. L-2 (possibly none) are copied into each follower's page S.  A page goes back to the pool when its last holder
 *     retires (smi_llm_retire, smi_llm_retire_many, smi_llm_session_begin, smi_llm_prefill); smi_llm_kv_pages counts as free
 *     only the pages no slot holds.  One prompt's n takes use ceil(L/P) + (n-1) (ceil(L/P) - S) pages, against n ceil(L/P)
 *     for the expanded admission.
 *   Contiguous cache: positions 0 .. L-2 of every layer, K and V, every kv head, are copied into each follower.
 *   All or nothing: every n_return[b] >= 1, N within the free slots, the records (as smi_llm_admit_logprobs) and the pool's
 *     pages for the formula above are checked before anything of the handle is touched; a failing call returns SMI_EINVAL
 *     or SMI_ENOMEM and takes no slot, page, page reference or admission number.
 * Static generation (smi_llm_prefill) has no forks. */
int smi_llm_admit_forked(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                         const int32_t* n_return, const smi_sample_params* params, const smi_penalty_params* pens,
                         const int32_t* return_log_probs, int32_t* slots_out, void* stream);
/* Allowed-token constraints (vLLM's allowed_token_ids; transformers' SuppressTokensLogitsProcessor of the complement).
 * smi_llm_admit_constrained = smi_llm_admit_forked plus one allow record per OUTPUT sequence ([N], like the other records;
 * allow = NULL: exactly smi_llm_admit_forked).  The allowed set of a record is the union of the half-open ranges
 * [lo[i], hi[i]), i < n_ranges.  Stage 0, before the penalty stages 1-3 of smi_llm_admit_penalized: every id outside the
 * row's set gets logit -inf; selection (arg-max, or temperature -> top-k -> top-p -> draw) then sees only allowed ids, the
 * admission's first token included.  Log-probabilities (smi_llm_admit_logprobs) are taken over the logits after stage 0, so
 * they are normalised over the allowed set (SuppressTokensLogitsProcessor placed first among the processors).
 *   Eos ids are NOT added implicitly: a set without an eos id runs until the token budget runs out.
 *   Neutral: n_ranges = 0, or ranges that cover [0, vocab_size); that row takes the route and the bits it gets without a record.
 *   Checked before anything of the handle is touched (SMI_EINVAL, no slot, page, page reference or admission number taken):
 *   0 <= n_ranges <= SMI_MAX_ALLOW_RANGES, reserved = 0, 0 <= lo[i] < hi[i] <= vocab_size, ranges sorted and disjoint
 *   (hi[i] <= lo[i + 1]), and with min_new_tokens > 0 the set holds at least one id that is not an eos id.
 *   Independence: a constrained row's tokens and log-probabilities do not depend on what else is live, bit for bit, with
 *   either KV dtype, paged or contiguous -- nor on whether its step read only the lm_head rows the constrained rows can emit
 *   (every row of the step constrained) or the whole table.
 * Static generation (smi_llm_prefill) has no constraints. */
#define SMI_MAX_ALLOW_RANGES 16
typedef struct smi_allow_params {
  int32_t n_ranges;                     /* 0 .. SMI_MAX_ALLOW_RANGES; 0 = no constraint */
  int32_t reserved;                     /* 0 */
  int32_t lo[SMI_MAX_ALLOW_RANGES];     /* first id of range i */
  int32_t hi[SMI_MAX_ALLOW_RANGES];     /* one past its last id */
} smi_allow_params;
int smi_llm_admit_constrained(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                              const int32_t* n_return, const smi_sample_params* params, const smi_penalty_params* pens,
                              const int32_t* return_log_probs, const smi_allow_params* allow, int32_t* slots_out, void* stream);
/* Per-request sequence bias, banned and stop token sequences (TensorRT-LLM's per-request embedding_bias / bad_words_list /
 * stop_words_list inputs, runtime/triton_trtllm/model_repo/tensorrt_llm/config.pbtxt; transformers'
 * SequenceBiasLogitsProcessor, and NoBadWordsLogitsProcessor = the same with bias -inf).
 * smi_llm_admit_biased = smi_llm_admit_constrained plus one smi_seq_params record per OUTPUT sequence ([N], like the other
 * records; seq = NULL: exactly smi_llm_admit_constrained).
 *   Stage 0b, after the allowed-set stage 0 and before the penalty stages 1-3 (transformers puts sequence_bias ahead of the
 *   repetition penalty, TensorRT-LLM adds embedding_bias first; the stage is additive and does not commute with the
 *   multiplicative repetition penalty, so the order is part of the contract).  Let ctx = the sequence's prompt followed by
 *   the tokens it has generated so far, at the step that chooses the next token.  Bias entry i (bias_len[i] = L ids
 *   bias_ids[i][0 .. L), value bias[i]) APPLIES to its last id when L <= len(ctx) and ctx's last L - 1 ids equal the entry's
 *   first L - 1; an entry of length 1 always applies.  The prompt counts as context, as in transformers (the library keeps the
 *   prompt's last SMI_MAX_SEQ_LEN - 1 ids with the record; the takes of a fork get their prompt's).  Per id, the applying
 *   biases are summed in fp32 starting from 0: the length-1 entry first, then the longer entries in record order (transformers'
 *   order); the logit then becomes x + total, one fp32 add.  A bias is finite or -inf; -inf bans the id at that step
 *   (bad_words_list / bad_words_ids).  An id outside the row's allowed set stays -inf.  Log-probabilities
 *   (smi_llm_admit_logprobs) are taken after this stage, as after the others; selection is unchanged.
 *   Stop sequences: after a token is emitted, let g = the tokens the sequence has GENERATED, the new one included.  Stop
 *   sequence j (stop_len[j] = L ids stop_ids[j][0 .. L)) is met when len(g) >= L, g's last L ids equal it and len(g) >= the
 *   row's min_new_tokens.  From there the slot behaves exactly as after an eos id: the same finished flag in smi_llm_status /
 *   smi_llm_poll / smi_llm_slots_tokens, the same treatment in the later steps of the same smi_llm_decode call; the matched
 *   tokens stay in the history, as an eos id does.  Matching is on generated tokens only (TensorRT-LLM's semantics): a prompt
 *   that ends in the sequence does not stop the row.
 *   Neutral: n_bias = 0 and n_stop = 0; that row takes the route and the bits it gets without a record.
 *   Checked before anything of the handle is touched (SMI_EINVAL, no slot, page, page reference or admission number taken):
 *   0 <= n_bias <= SMI_MAX_BIAS_SEQS, 0 <= n_stop <= SMI_MAX_STOP_SEQS, every length in 1..SMI_MAX_SEQ_LEN, every id in
 *   [0, vocab_size), no bias NaN or +inf, the bias entries pairwise distinct sequences and the stop sequences likewise,
 *   reserved = 0, and a survivor: the row's allowed set (the whole vocabulary without one) minus the distinct last ids of its
 *   -inf entries -- whatever their length: a conservative static bound -- holds at least one id, and with min_new_tokens > 0 at
 *   least one id that is not an eos id.
 *   Independence: a row's tokens and log-probabilities do not depend on what else is live, nor on whether its step read the
 *   restricted lm_head -- bit for bit, with either KV dtype, paged or contiguous.
 * Static generation (smi_llm_prefill) has none of this. */
#define SMI_MAX_BIAS_SEQS 32
#define SMI_MAX_STOP_SEQS 8
#define SMI_MAX_SEQ_LEN 8
typedef struct smi_seq_params {
  int32_t n_bias;                                          /* 0 .. SMI_MAX_BIAS_SEQS */
  int32_t n_stop;                                          /* 0 .. SMI_MAX_STOP_SEQS */
  int32_t bias_len[SMI_MAX_BIAS_SEQS];                     /* 1 .. SMI_MAX_SEQ_LEN */
  float bias[SMI_MAX_BIAS_SEQS];                           /* finite or -inf */
  int32_t bias_ids[SMI_MAX_BIAS_SEQS * SMI_MAX_SEQ_LEN];   /* entry i: bias_ids[i * SMI_MAX_SEQ_LEN + 0 .. bias_len[i]) */
  int32_t stop_len[SMI_MAX_STOP_SEQS];                     /* 1 .. SMI_MAX_SEQ_LEN */
  int32_t stop_ids[SMI_MAX_STOP_SEQS * SMI_MAX_SEQ_LEN];   /* sequence j: stop_ids[j * SMI_MAX_SEQ_LEN + 0 .. stop_len[j]) */
  int32_t reserved[2];                                     /* 0 */
} smi_seq_params;
int smi_llm_admit_biased(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                         const int32_t* n_return, const smi_sample_params* params, const smi_penalty_params* pens,
                         const int32_t* return_log_probs, const smi_allow_params* allow, const smi_seq_params* seq,
                         int32_t* slots_out, void* stream);
/* No repeated n-grams (transformers' no_repeat_ngram_size / NoRepeatNGramLogitsProcessor; TensorRT-LLM's sampling-config field
 * of the same name).  smi_llm_admit_ngram = smi_llm_admit_biased plus no_repeat_ngram [N]: one int32 n per OUTPUT sequence
 * (NULL, or all zeros: exactly smi_llm_admit_biased).  n = 0: none; valid values 0 .. SMI_MAX_NGRAM.
 *   Let ctx = the sequence's full prompt followed by the tokens it has generated so far, at the step that chooses the next
 *   token, L = len(ctx).  The prompt counts, as in transformers (the library keeps every flagged slot's prompt ids on the
 *   device; the takes of a fork see their prompt's ids and their own generated ids).  If L + 1 < n nothing is banned.
 *   Otherwise let tail = ctx[L-n+1 .. L) (n - 1 ids, empty for n = 1): for every i in [0, L-n] with ctx[i .. i+n-1) == tail
 *   the logit of id ctx[i+n-1] becomes -inf.  Nothing else of the row changes: no finite logit moves by a bit.  So no n-gram
 *   of the context is ever emitted twice.
 *   Stage order: between the penalty stages 1-3 and the min_new_tokens mask, transformers' place for it.  It writes only
 *   -inf, and every other stage maps -inf to -inf, so the result is the same wherever the ban is physically applied (the
 *   library applies it to the lm_head's row, before stage 0).  Log-probabilities (smi_llm_admit_logprobs) are taken after it;
 *   selection is unchanged.
 *   Neutral: n = 0; that row takes the route and the bits it gets without the record.
 *   Checked with the other records before anything of the handle is touched (SMI_EINVAL, no slot, page, page reference or
 *   admission number taken): 0 <= n <= SMI_MAX_NGRAM, and for n > 0 the survivor rule: a step bans at most
 *   L - n + 1 <= max_positions - 1 distinct ids, so the row's static survivor count -- its allowed set (the whole vocabulary
 *   without one) minus the distinct last ids of its -inf bias entries, minus the eos ids when min_new_tokens > 0 -- must be at
 *   least max_positions.  Conservative and static, like smi_llm_admit_biased's bound: no row ever reaches selection with
 *   every logit -inf.
 *   Independence: a row's tokens and log-probabilities do not depend on what else is live, nor on whether its step read the
 *   restricted lm_head -- bit for bit, with either KV dtype, paged or contiguous.
 * Static generation (smi_llm_prefill) has none of this. */
#define SMI_MAX_NGRAM 64
int smi_llm_admit_ngram(smi_llm* h, const int64_t* ids_host, const int32_t* lens_host, int n, int P_max,
                        const int32_t* n_return, const smi_sample_params* params, const smi_penalty_params* pens,
                        const int32_t* return_log_probs, const smi_allow_params* allow, const smi_seq_params* seq,
                        const int32_t* no_repeat_ngram, int32_t* slots_out, void* stream);
int smi_llm_retire(smi_llm* h, int slot, void* stream);
int smi_llm_slot_tokens(smi_llm* h, int slot, int64_t* out_host, int cap, int32_t* n_out, int32_t* finished, void* stream);
/* Several sequences leave at once with no host round trip (the device row list is compacted in place), and the tokens of
 * several slots in one round trip: out_host [n][cap], n_out [n], finished [n].  A retired slot's history stays readable
 * until a later admission reuses the slot. */
int smi_llm_retire_many(smi_llm* h, const int32_t* slots, int n, void* stream);
int smi_llm_slots_tokens(smi_llm* h, const int32_t* slots, int n, int64_t* out_host, int cap, int32_t* n_out, int32_t* finished,
                         void* stream);
/* The tokens the listed slots have emitted since their own offsets, in one small round trip -- what a streaming loop needs
 * every few decode steps.  Per listed slot i: count[i] = tokens emitted so far, finished[i] = its eos flag,
 * n_out[i] = max(0, min(count[i], from[i] + cap) - from[i]) and out_host[i][0 .. n_out[i]) = its history entries from[i] ..
 * (out_host is [n][cap]).  By definition this is smi_llm_slots_tokens of the same slots, sliced; like it, it reads live slots
 * and retired ones until a later admission reuses them, and synchronises the stream.  A gather kernel (one block per listed
 * slot) packs {count, finished, ids[cap]} per slot into a staging buffer of the handle, and ONE copy of n * (8 + 8 * cap) bytes
 * brings them to a pinned host buffer of the handle (cap counts up to max_positions, the history's length) -- against the whole
 * [max_positions][SMI_MAX_ROWS] history that smi_llm_slots_tokens copies.  The kernel runs on the caller's stream between decode
 * calls, never inside the captured decode step.  n outside 1..SMI_MAX_ROWS, a slot out of range, from[i] < 0 or cap < 1:
 * SMI_EINVAL, nothing written. */
int smi_llm_poll(smi_llm* h, const int32_t* slots, const int32_t* from, int n, int64_t* out_host, int cap, int32_t* n_out,
                 int32_t* count, int32_t* finished, void* stream);
/* Park and resume: a sequence leaves its KV slot as a snapshot ("blob") in CALLER-OWNED device memory and comes back later into
 * any free slot, with not one bit changed -- so more requests may be open than there are decode rows (a streaming server parks
 * the requests that are far ahead of their listeners).  The library keeps no pointer to a blob: it may be freed, copied or
 * restored more than once as soon as the call's work on the stream has run.
 *   smi_llm_slot_blob_bytes: the snapshot size of the sequence now in `slot` (host arithmetic, no device work).  It depends on
 *     the sequence's cache positions, tokens emitted and record set: a part belonging to a feature the sequence does not use
 *     takes no space (the penalty history row, 2 * vocab_size bytes, only with a penalty record; the prompt ids,
 *     4 * prompt length bytes, only with no_repeat_ngram_size; the log-probabilities only with return_log_probs; the bias /
 *     stop record only with one).
 *   smi_llm_slots_save: writes the complete state of each listed busy slot into blobs_dev[i] (16-byte aligned, caps[i] bytes
 *     available; used[i] = bytes written = smi_llm_slot_blob_bytes).  A snapshot, not a move: the slots stay exactly as they
 *     were; parking is a save followed by smi_llm_retire_many.  Between decode calls of a session, on the caller's stream,
 *     outside any capture; it touches no cached step graph (like smi_llm_poll) and does not synchronise.
 *   Blob layout (all of it device memory; every part starts on a 16-byte boundary): a header -- magic, sizes, the feature byte,
 *     a stamp of the handle's configuration, of the handle and of the session (the smi_llm_session_begin it was saved in),
 *     cache length, prompt length, the admission number (sampler stream id), the sampling / penalty / log-probability /
 *     allowed-set / n-gram records as admitted, a checksum of those host-written bytes, and 32 bytes the gather kernel writes:
 *     the row descriptor (position, last token, token index), count, finished -- then the bias / stop record if the sequence
 *     has one, then K/V [layer][K, V][kv head][position][row] for the positions written so far, the sequence's column of
 *     the token history, of the log-probabilities, its penalty history row and its prompt ids.  The host part travels IN the
 *     blob's header: a blob is self-contained.  Nothing in it names the slot it came from: saving a restored sequence again
 *     gives the same bytes.  Not in it, because they are session state: the eos list, the handle's sampler settings and seed.
 *     A blob belongs to the handle and session that wrote it and goes back nowhere else: the handle and session stamps decide
 *     that.  The configuration stamp (a hash of the raw smi_llm_cfg bytes) is checked first and only words the refusal of a
 *     blob from a handle built otherwise; it is no means of telling whether two handles' configurations are compatible.
 *   smi_llm_slots_restore: puts each snapshot (bytes[i] = its used size) into a free KV slot -- the lowest free ones, in order,
 *     returned in slots_out; not necessarily the slot or row position it came from -- through an admission's bookkeeping:
 *     slot and pages (pages of its own, whatever the original shared with a fork's other takes; all or nothing), records,
 *     feature byte, and the re-embedding of every live row.  The sequence keeps its admission number; no new one is given
 *     out.  The sampler stream is keyed by (seed; token index, admission number) and every decode kernel treats rows
 *     independently, so the restored sequence emits exactly the tokens (log-probabilities, stops) it would have emitted
 *     without the park.  Restoring a snapshot whose original is still live is allowed: both continue with the same stream
 *     and emit the same tokens.  Synchronises the stream (it reads the headers back, as an admission reads the live rows).
 *   Refusals, each changing nothing: outside a session SMI_ESTATE; a blob saved under another configuration, by another
 *     handle or in an earlier session of this one SMI_ESTATE; a truncated or corrupt blob (magic, checksum, sizes that do not
 *     add up to bytes[i], impossible lengths), a cap below the needed size, a slot that is not busy or listed twice, a
 *     misaligned address SMI_EINVAL; fewer free slots than n SMI_ESTATE; a page pool that cannot hold all n SMI_ENOMEM
 *     (nothing allocated).  The payload behind the header is not checksummed: every bound the scatter uses comes from the
 *     checked header, so a damaged payload can change the sequence's tokens but cannot write outside its slot. */
int smi_llm_slot_blob_bytes(smi_llm* h, int slot, size_t* bytes);
int smi_llm_slots_save(smi_llm* h, const int32_t* slots, int n, void* const* blobs_dev, const size_t* caps, size_t* used, void* stream);
int smi_llm_slots_restore(smi_llm* h, const void* const* blobs_dev, const size_t* bytes, int n, int32_t* slots_out, void* stream);
/* count_host / finished_host [SMI_MAX_ROWS]: tokens emitted and eos flag per KV slot, one round trip. */
int smi_llm_status(smi_llm* h, int32_t* count_host, int32_t* finished_host, void* stream);
/* Test/teacher-forcing entry: feeds ids_host[0..S) at positions 0..S-1 of slot 0 (cache reset) and
 * writes every position's logits to logits_dev [S][vocab_size] f32. */
int smi_llm_forward_logits(smi_llm* h, const int64_t* ids_host, int S, float* logits_dev, void* stream);
/* Steps generated so far per sequence (including the prefill token), and the KV bytes per token. */
int smi_llm_steps(smi_llm* h);
/* Paged KV cache: pages in the pool and pages currently free (both 0 when the cache is not paged). */
int smi_llm_kv_pages(smi_llm* h, int32_t* total, int32_t* free_pages);
/* ------------------------------------------------------------------------------------------
 * Vocoder: BiCodec.detokenize (codebook lookup, d-vector, ConvNeXt prenet, WaveGenerator).
 * ---------------------------------------------------------------------------------------- */
typedef struct smi_voc smi_voc;

typedef struct smi_voc_cfg {
  int32_t vq_input_dim, codebook_size, codebook_dim;
  int32_t spk_out_dim, spk_latent_dim, spk_token_num, fsq_dims; /* fsq_dims = len(fsq_levels) */
  int32_t fsq_levels[8];
  int32_t pre_input_channels, pre_dim, pre_inter, pre_layers, pre_out_channels, pre_cond_dim;
  int32_t pre_num_down;      /* len(sample_ratios); every ratio must be 1 */
  int32_t pre_tanh_final;
  int32_t dec_in, dec_channels, dec_nblocks;
  int32_t dec_rates[8], dec_ksizes[8];
  int32_t max_batch;         /* utterances per forward */
  int32_t max_frames;        /* semantic frames per utterance */
  /* 0 (default): the dense conv / linear stack runs on the bf16 matrix pipe with both operands split into two bf16 planes
   * (w x ~= w_hi x_hi + w_hi x_mid + w_mid x_hi, fp32 accumulate): 5e-5 max-abs from the fp32 waveform at the 0.5B shape,
   * north_star's bound being 1e-3.  1: every contraction on the exact-fp32 matrix pipe (verification mode, 1/16 of the rate).
   * The arena packing of the affected weights differs (smi_voc_arena_entry reports the kind). */
  int32_t exact_fp32;
} smi_voc_cfg;

/* The vocoder arena is a flat f32 buffer of tensors in the order smi_voc_arena_entry enumerates
 * (name = the reference state_dict key after remove_weight_norm, or a derived packed tensor). */
int smi_voc_arena_count(const smi_voc_cfg* cfg);
/* info: int32[6] = {packing kind (0 raw f32 copy, 1 Conv1d/Linear weight [Cout][Cin][K], 2 ConvTranspose1d
 * weight [Cin][Cout][K], 3 / 4 the same two as bf16 planes), Cout, Cin, K, stride, padding}.  Kinds 1 / 2 are laid out
 * [phase][cout_tile:32][tap][cin_group:8][lane:64][4 f32] = v_mfma_f32_32x32x2_f32 A operands; kinds 3 / 4
 * [phase][cout_tile:32][tap][cin_step:16][plane:2 (hi, mid)][lane:64][8 bf16] = v_mfma_f32_32x32x16_bf16 A operands,
 * lane l holding row l & 31, channels 8 (l >> 5) .. + 7 of the step (sparkmi/bicodec.py: pack_conv / pack_conv_b). */
int smi_voc_arena_entry(const smi_voc_cfg* cfg, int index, char* name, int name_cap,
                        size_t* offset, size_t* bytes, int32_t* info);
size_t smi_voc_arena_bytes(const smi_voc_cfg* cfg);

int smi_voc_create(const smi_voc_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_voc** out);
int smi_voc_destroy(smi_voc* h);
/* sem_dev [B][T_max] int64 semantic ids (row b valid for lens_host[b] frames), glob_dev [B][Ntok]
 * int32 global ids, wav_dev [B][hop*T_max] f32 (samples beyond hop*lens[b] are zeroed).
 * Each row's result equals an un-padded B=1 run of that row. */
int smi_voc_forward(smi_voc* h, const int64_t* sem_dev, const int32_t* lens_host, const int32_t* glob_dev,
                    int B, int T_max, float* wav_dev, void* stream);
/* smi_voc_forward's arguments; row b of the result equals, bit for bit, smi_voc_forward of that row alone (B = 1,
 * T_max = lens_host[b]) on a handle of the same config -- whatever else is in the call and wherever the row sits; samples beyond
 * hop*lens[b] are zero.  (smi_voc_forward chooses each layer's tiling, channel split and kernel form from its call shape
 * (B, longest row), so one of its rows equals its solo run only up to fp32 re-association.)  Here every such choice is taken as
 * if the call were the row's own (1, lens[b]); consecutive rows whose choices agree in every layer run as ONE launch sequence
 * whose grids cover their count and their longest row (a shorter row's spare blocks exit), so the call costs one launch sequence
 * per run of equal plans: sort the rows by length (BiCodecVocoder.detokenize_rows does) and a scheduler's few chunk lengths give
 * a handful of runs.  The kernels are smi_voc_forward's. */
int smi_voc_forward_rows(smi_voc* h, const int64_t* sem_dev, const int32_t* lens_host, const int32_t* glob_dev,
                         int B, int T_max, float* wav_dev, void* stream);
/* Test entry: copies an internal activation (after `stage`) of the last forward to out_dev. */
int smi_voc_debug_stage(smi_voc* h, int stage, float* out_dev, size_t max_floats, size_t* n_floats, void* stream);
/* Per-kernel timing probe (see smi_llm_time_kernel): stage index into the launch list of the last
 * forward; returns avg ms and the kernel's FLOPs per launch. */
int smi_voc_num_launches(smi_voc* h);
int smi_voc_time_launch(smi_voc* h, int index, int iters, float* ms_avg, double* flops, char* name, int name_cap, void* stream);

/* One block of the vocoder on caller tensors -- the op-level test entry points.  The launches are built by the very functions
 * smi_voc_forward builds them with (same kernels, launch geometry and epilogue fusions), so the reference's own layer classes
 * can be checked one at a time: ResidualUnit (sparktts/modules/blocks/layers.py:51-67), DecoderBlock
 * (sparktts/modules/encoder_decoder/wave_generator.py:29-53), ConvNeXtBlock with LayerNorm or AdaLayerNorm
 * (sparktts/modules/blocks/vocos.py:26-110).  A block's little arena is described exactly like the vocoder's
 * (smi_voc_block_arena_entry: names are "L." + the layer's own state_dict keys, "cat:a|b" = rows concatenated). */
enum { SMI_VOC_BLOCK_RESUNIT = 0, SMI_VOC_BLOCK_DECBLOCK = 1, SMI_VOC_BLOCK_CONVNEXT = 2 };
typedef struct smi_voc_block_cfg {
  int32_t kind;        /* SMI_VOC_BLOCK_* */
  int32_t C;           /* RESUNIT: channels; DECBLOCK: input channels; CONVNEXT: model dim */
  int32_t Cout;        /* DECBLOCK: output channels */
  int32_t K, S;        /* DECBLOCK: ConvTranspose1d kernel size and stride (padding (K - S) / 2) */
  int32_t dil;         /* RESUNIT: dilation of the 7-tap conv (1, 3 or 9) */
  int32_t I;           /* CONVNEXT: intermediate dim */
  int32_t cond_dim;    /* CONVNEXT: 0 = LayerNorm; > 0 = AdaLayerNorm on a [B][cond_dim] condition */
  int32_t exact_fp32;  /* as smi_voc_cfg.exact_fp32 */
} smi_voc_block_cfg;
int smi_voc_block_arena_count(const smi_voc_block_cfg* cfg);
size_t smi_voc_block_arena_bytes(const smi_voc_block_cfg* cfg);
int smi_voc_block_arena_entry(const smi_voc_block_cfg* cfg, int index, char* name, int name_cap,
                              size_t* offset, size_t* bytes, int32_t* info);
/* x_dev [B][C][L] f32 (contiguous), y_dev [B][C or Cout][L or L * S].  The vocoder applies a block's LEADING Snake in the
 * producer's epilogue, so: RESUNIT takes x_dev and xs_dev = snake(x, block.0.alpha); DECBLOCK takes only xs_dev =
 * snake(x, block.0.alpha); CONVNEXT takes x_dev (and cond_dev [B][cond_dim] for AdaLayerNorm).  lens_host (may be null =
 * all rows full) masks ragged rows as in smi_voc_forward.  Synchronises the stream before returning. */
int smi_voc_block_run(const smi_voc_block_cfg* cfg, const void* arena_dev, size_t arena_bytes, const float* x_dev,
                      const float* xs_dev, const float* cond_dev, const int32_t* lens_host, int B, int L, float* y_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prompt encoder (voice cloning): BiCodecTokenizer.tokenize (sparktts/models/audio_tokenizer.py:85-130)
 * = zero-mean/unit-variance wav -> wav2vec2 (layers below the last tapped hidden state) -> mean of
 * three hidden states -> BiCodec Encoder -> cosine VQ arg-max (semantic ids); reference clip -> mel
 * -> ECAPA-TDNN latent -> perceiver resampler -> FSQ (global ids)  (sparktts/models/bicodec.py:151-169).
 * One utterance per call, as the reference's tokenize() (smi_enc_forward), or a ragged batch (smi_enc_forward_rows).
 * ---------------------------------------------------------------------------------------- */
typedef struct smi_enc smi_enc;

typedef struct smi_enc_cfg {
  /* wav2vec2 (transformers Wav2Vec2Config; layer-norm / stable-layer-norm variant) */
  int32_t w2v_conv_dim, w2v_nconv;
  int32_t w2v_kernel[8], w2v_stride[8];
  int32_t w2v_hidden, w2v_layers /* = max(taps): layers actually run */, w2v_heads, w2v_inter;
  int32_t w2v_pos_k, w2v_pos_groups;
  int32_t w2v_taps[3];       /* hidden_states indices averaged (audio_tokenizer.py:96-98) */
  float w2v_eps;
  /* BiCodec encoder + quantizer */
  int32_t enc_in, enc_dim, enc_inter, enc_layers, enc_out, enc_num_down;
  int32_t codebook_size, codebook_dim;
  /* mel (bicodec.py:200-211) */
  int32_t n_fft, win_length, hop_length, num_mels;
  /* speaker encoder analysis side */
  int32_t ecapa_channels, ecapa_out, spk_latent, spk_tokens, fsq_dims;
  int32_t fsq_levels[8];
  int32_t perc_depth, perc_heads, perc_ff_inner;
  int32_t max_samples;       /* longest prompt wav (samples) */
  int32_t max_ref_samples;   /* longest reference clip (samples) */
  /* 0 (default): wav2vec2's transformer projections and the BiCodec encoder's ConvNeXt stack run on the bf16-split matrix
   * pipe (as smi_voc_cfg.exact_fp32 describes); 1: every contraction on the exact-fp32 matrix pipe.  Token ids are arg-max /
   * rounding decisions: they agree between the two modes wherever the decision margin exceeds the split's 2^-17 noise. */
  int32_t exact_fp32;
} smi_enc_cfg;

/* Arena: like the vocoder's (same entry info and conv packing).  Names are the reference / transformers
 * state_dict keys ("w2v." + key for wav2vec2), "cat:a|b|c" row concatenations, or derived tensors the host
 * computes: "bnscale:<bn prefix>" / "bnshift:<bn prefix>" (BatchNorm eval affine), "transpose:<key>",
 * "mel.dft" ([2*(n_fft/2+1)][n_fft] windowed cos / -sin DFT basis) and "mel.fb" ([num_mels][n_fft/2+1]). */
int smi_enc_arena_count(const smi_enc_cfg* cfg);
int smi_enc_arena_entry(const smi_enc_cfg* cfg, int index, char* name, int name_cap,
                        size_t* offset, size_t* bytes, int32_t* info);
size_t smi_enc_arena_bytes(const smi_enc_cfg* cfg);
int smi_enc_create(const smi_enc_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_enc** out);
int smi_enc_destroy(smi_enc* h);
/* wav_dev [n_samples] f32 (volume-normalised, NOT yet zero-mean/unit-var), ref_dev [n_ref] f32 reference clip;
 * sem_dev [>= frames] int64 out, glob_dev [spk_tokens] int32 out; *n_frames = wav2vec2 frames produced. */
int smi_enc_forward(smi_enc* h, const float* wav_dev, int n_samples, const float* ref_dev, int n_ref,
                    int64_t* sem_dev, int32_t* glob_dev, int* n_frames, void* stream);
/* A ragged batch of B prompts in one call.  wav_dev [B][wav_stride] f32 (row b valid for n_samples_host[b]), ref_dev
 * [B][ref_stride] f32 (n_ref_host[b]); sem_dev [B][sem_stride] int64 out: row b receives n_frames_host[b] ids, entries beyond are
 * left untouched; glob_dev [B][spk_tokens] int32 out.  Row b's ids -- and every intermediate activation -- equal, bit for bit,
 * smi_enc_forward of that row alone on a handle of the same config, whatever else is in the call and wherever the row sits.
 * (The conv launch builder picks tile width, channel split and kernel form from its call shape, and the ids are arg-max and
 * rounding decisions, so a batch planned as a whole would not do.)  Here every such choice is taken as if the call were the
 * row's own; consecutive rows whose choices agree in every launch run as ONE launch sequence whose grids cover their count and
 * their longest row (a shorter row's spare blocks exit; attention is over the row's own keys), so the call costs one launch
 * sequence per run of equal plans: sort the rows by length (BiCodecEncoder.tokenize_rows does).  Every row gets
 * smi_enc_forward's argument checks before anything reaches the device.  The launches are eager (no graph); the solo path, its
 * graph cache and its debug views are neither read nor disturbed.
 * smi_enc_rows_reserve allocates (or re-allocates, when the arguments change) the rows workspace: max_rows rows of up to
 * max_row_samples (<= max_samples) / max_row_ref_samples (<= max_ref_samples); smi_enc_forward_rows allocates nothing and
 * returns SMI_EINVAL without a reserve or beyond it.  smi_enc_destroy frees it. */
int smi_enc_rows_reserve(smi_enc* h, int max_rows, int max_row_samples, int max_row_ref_samples);
int smi_enc_forward_rows(smi_enc* h, const float* wav_dev, long long wav_stride, const int32_t* n_samples_host,
                         const float* ref_dev, long long ref_stride, const int32_t* n_ref_host, int B,
                         int64_t* sem_dev, long long sem_stride, int32_t* glob_dev, int32_t* n_frames_host, void* stream);
/* Test entry: copies a named internal activation of the last forward ("feat", "z", "mel", "ecapa_latent",
 * "perceiver", "hs0", "conv_feats", "input_values", ...) to out_dev as [rows][cols] f32; dims[2] = {rows, cols}. */
int smi_enc_debug_stage(smi_enc* h, const char* name, float* out_dev, size_t max_floats, int32_t* dims, void* stream);
int smi_enc_num_launches(smi_enc* h);
int smi_enc_time_launch(smi_enc* h, int index, int iters, float* ms_avg, double* flops, char* name, int name_cap, void* stream);

/* ------------------------------------------------------------------------------------------
 * Audio front / back end on the device: a rational resampler with scipy.signal.resample_poly's arithmetic (what
 * sparkmi/encoder.py: load_audio runs on the host; NOT the reference's soxr VHQ), and the voice prompt's preparation
 * (sparktts/utils/audio.py: audio_volume_normalize; audio_tokenizer.py:57-72: get_ref_clip) written straight into the buffers
 * smi_enc_forward_rows reads.  Opt-in: nothing else of the library calls it.
 *
 * Resampling.  For an input row x[0 .. n), a ratio up/down in lowest terms and taps h[0 .. 2H]:
 *     n_out = ceil(n * up / down)                                               (smi_rs_out_len)
 *     y[k]  = sum over j of x[j] * h[H + k * down - j * up],   0 <= j < n, tap index in [0, 2H]   (zero-padded edges)
 * With h = firwin(2H + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up and H = 10 * max(up, down) this is
 * resample_poly(x, up, down) (sparkmi/audio.py: resample_taps computes those taps with numpy alone).  Taps are data the caller
 * registers once per ratio (smi_rs_register: float64 on the host, rounded to fp32 once, kept on the device by the handle).
 * A sample is summed in ascending j, in fp32, in one accumulator, product and sum rounded separately: its bits depend on its
 * row's samples and ratio alone -- not on the row's place in the call, the other rows, the strides or the tiling.  up = down = 1
 * needs no filter and copies the row.  Indices are 32-bit: n * up and n_out * down must stay below 2^31.
 *
 * smi_rs_create reserves nothing but limits: max_rows (1..64) rows a call, max_in / max_out samples a row (1..2^24); a call
 * beyond them is refused.  One launch covers every row of a call (the row index is in the grid; rows may carry different
 * ratios); the calls are asynchronous on the caller's stream and never synchronise.  Every argument of every row is checked
 * before anything reaches the device: a bad one returns SMI_EINVAL, names the argument in smi_last_error and launches nothing. */
typedef struct smi_rs smi_rs;
int smi_rs_create(int max_rows, int max_in, int max_out, smi_rs** out);
int smi_rs_destroy(smi_rs* h);
/* taps_host [n_taps] float64, n_taps = 2H + 1 odd.  Synchronous (one small copy); a ratio is registered once.  A filter whose taps
 * plus the input window of one 1024-sample output tile exceed 16384 floats (the kernel stages both in 64 KiB of LDS) is refused. */
int smi_rs_register(smi_rs* h, int up, int down, const double* taps_host, int n_taps);
/* ceil(n * up / down); -1 for a negative n or a non-positive up / down.  Pure host arithmetic. */
long long smi_rs_out_len(long long n, int up, int down);
/* in_dev [B][in_stride] f32 (row b valid for n_in_host[b]); out_dev [B][out_stride] f32: row b receives its n_out samples and
 * zeros from there to out_stride. */
int smi_rs_resample_rows(smi_rs* h, const float* in_dev, long long in_stride, const int32_t* n_in_host, const int32_t* up_host,
                         const int32_t* down_host, int B, float* out_dev, long long out_stride, void* stream);
/* Prompt preparation: raw mono rows at their own rates -> wav_dev [B][wav_stride] (the model-rate prompt, zeros past n_out) and
 * ref_dev [B][ref_stride] (the reference clip, zeros past ref_len_host[b]), in two launches:
 *   1. resample, as smi_rs_resample_rows;
 *   2. normalize = 1: audio_volume_normalize with its quirks.  temp = sort(|y|) of the resampled row; peak = temp[-1]; peak < 0.1:
 *      gain 0.1 / max(peak, 1e-3); of temp only the values > 0.01 count, n of them; n <= 10: done; else volume =
 *      mean(temp[int(0.9 n) .. int(0.99 n))) -- peak and temp are taken BEFORE the < 0.1 rescale --, the gain is multiplied by
 *      clip(0.2 / volume, 0.1, 10), and divided by the scaled peak if that exceeds 1.  The ranks are selected exactly (a radix
 *      select on the bit patterns of |y|, ties by counts) and the range is summed in 64-bit fixed point (every counted value is
 *      a multiple of 2^-30; exact while |y| < 2^13), so the statistic has no summation order: the gain, formed in float64, is
 *      reproducible bit for bit and independent of the batch.  Each sample becomes fl32(float64(y) * gain) -- one rounding,
 *      where the host path rounds per stage.  gain_out_dev [B] float64 (may be null) receives the gain (1 with normalize = 0);
 *   3. ref[i] = wav[i mod n_out] for i < ref_len_host[b], of the normalized samples.
 * n_out_host [B] (may be null) receives the rows' lengths.  in_dev must not overlap wav_dev. */
int smi_rs_prompt_rows(smi_rs* h, const float* in_dev, long long in_stride, const int32_t* n_in_host, const int32_t* up_host,
                       const int32_t* down_host, int B, int normalize, float* wav_dev, long long wav_stride,
                       const int32_t* ref_len_host, float* ref_dev, long long ref_stride, double* gain_out_dev,
                       int32_t* n_out_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stream joiner: the overlapping chunks of a streamed request become one contiguous, playable stream on the device, at the
 * model's rate or at any registered-style ratio up/down of it.  State is kept across chunk edges per stream (a slot of the
 * handle): the held tail for the fade and the resampler's last input samples.  Opt-in: nothing else of the library calls it.
 *
 * Join.  A stream's chunks c_0 .. c_{m-1} have L_i samples; `overlap` = n samples; fade_in = linspace(0, 1, n) and fade_out =
 * linspace(1, 0, n) are float64 tables the caller uploads at creation (the device computes no linspace).  t is the held tail,
 * the last n samples of c_{i-1}:
 *     c_0, the only chunk:     emits c_0                                   holds nothing
 *     c_0, not last:           emits c_0[:L-n]                             holds c_0[L-n:]
 *     c_i, i >= 1, not last:   emits fade(c_i[:n], t), then c_i[n:L-n]     holds c_i[L-n:]
 *     c_i, i >= 1, last:       emits fade(c_i[:n], t), then c_i[n:]        holds nothing
 *     fade(a, t)[q] = fl32( fl64(fl64(a[q]) * fade_in[q]) + fl64(fl64(t[q]) * fade_out[q]) )
 * -- two float64 products rounded separately, one float64 add, one rounding to fp32, no FMA.  Where every L_i >= 2n the joined
 * stream is sparkmi/streaming.py: crossfade(chunks, n) cast to fp32, bit for bit; its length is sum L_i - n (m - 1).  Two cases
 * are defined here and not by crossfade: n = 0 is plain concatenation (crossfade degenerates), and a last chunk with
 * n <= L < 2n follows the table (crossfade would repeat samples).  A chunk that is not the last needs L >= 2n and a last chunk
 * with i >= 1 needs L >= n: anything else is SMI_EINVAL.  An empty last chunk is valid where those rules allow it (n = 0, or the
 * only chunk) and flushes the resampler.
 *
 * Resample with state.  x is the joined stream, N samples so far; up/down and taps h[0 .. 2H] as for smi_rs_register.  Output k is
 * exactly the sum smi_rs_resample_rows forms for the whole stream: j ascending from ceil((k down - H) / up), clamped at 0, to
 * floor((k down + H) / up), clamped at the stream's end; fp32, one accumulator, product and sum rounded separately.  After a push
 * that is not the last the stream has emitted K(N) = max(0, ceil((N up - H) / down)) outputs in all, after the last one
 * ceil(N up / down); a push emits the difference, which may be 0.  The handle keeps ceil((2H + down) / up) + 1 input samples of
 * history per stream, which is enough; the latency is H / up input samples.  up = down = 1 needs no filter: the join's output is
 * emitted as it is, with no latency.
 *
 * Guarantees: the concatenation of a stream's pieces is, bit for bit, smi_rs_resample_rows of its whole joined waveform, whatever
 * the granularity of the pushes, the stream's slot, its row in a call and the other rows.  A piece's length is pure host
 * arithmetic (smi_join_piece_len); nothing synchronises.  A stream is refused (SMI_EINVAL) before N up or K down reaches 2^31.
 *
 * The per-stream counters (chunk index, N, K) live on the host, the tails and histories on the device in two sets that a
 * stream uses in turn: a push reads one and writes the other, so one launch serves a call whatever B.  All pushes of a handle
 * must go to one HIP stream (or be ordered by the caller). */
typedef struct smi_join smi_join;
/* max_streams (1..4096) slots; max_chunk (1..2^24) samples a chunk; overlap = n (0..max_chunk / 2); fade_*_host [n] float64 (may
 * be null for n = 0); taps_host [n_taps] float64, n_taps = 2H + 1 odd, LDS-limited as in smi_rs_register (ignored for 1/1).
 * Synchronous (one allocation, small copies). */
int smi_join_create(int max_streams, int max_chunk, int overlap, const double* fade_in_host, const double* fade_out_host, int up, int down,
                    const double* taps_host, int n_taps, smi_join** out);
int smi_join_destroy(smi_join* h);
/* A new stream in slot `stream`: chunk index, N and K are zero.  Host only.  A stream closes with its last chunk. */
int smi_join_open(smi_join* h, int stream);
/* One ready chunk per row: chunks_dev [B][stride] f32 (row b valid for len_host[b]), of the open streams stream_host[b], each at
 * most once in a call; last_host[b] = 1 on a stream's last chunk.  out_dev [B][out_stride] f32: row b receives its piece and
 * zeros from there to out_stride (>= 1 and >= the longest piece).  n_out_host [B] (may be null) receives the pieces' lengths,
 * filled before the launch.  B <= 64.  One launch, asynchronous on `stream`.  Every argument of every row is checked before
 * anything changes or is launched: a bad one returns SMI_EINVAL and names the argument in smi_last_error.  chunks_dev must not
 * overlap out_dev. */
int smi_join_push_rows(smi_join* h, const float* chunks_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                       const int32_t* last_host, int B, float* out_dev, long long out_stride, int32_t* n_out_host, void* stream);
/* The piece length of one push, pure host arithmetic: a stream with n_before joined samples and k_before emitted outputs takes a
 * chunk of len samples (first = 1: its first chunk; last = 1: its last); n_after / k_after (may be null) receive the counters
 * after it.  n_taps = 2H + 1 (1 for up = down = 1).  -1 for a length the rules above refuse or a bad argument. */
long long smi_join_piece_len(int overlap, int up, int down, int n_taps, int first, long long n_before, long long k_before, long long len,
                             int last, long long* n_after, long long* k_after);

/* ------------------------------------------------------------------------------------------
 * Long-form audio edge: the speech bounds of vocoded rows and their assembly into one waveform with pauses and fades, for text
 * that is generated sentence by sentence (sparkmi/pipeline.py: inference_long).  Free functions: no handle and no state, every
 * buffer is the caller's; asynchronous on the caller's stream; opt-in like the rest of this unit.  Every argument of every row
 * is checked before anything reaches the device: a bad one returns SMI_EINVAL, names the argument in smi_last_error and
 * launches nothing.
 *
 * Speech bounds (smi_trim_rows): the arithmetic of detect_speech_boundaries (sparktts/utils/audio.py:186-225), which
 * remove_silence_on_both_ends applies.  For a row x[0 .. n), window W >= 1, step s >= 1, threshold thr >= 0, margin m >= 0 and
 * n >= W:
 *     windows  x[i s .. i s + W),  i = 0 .. floor((n - W) / s)
 *     window i is speech when  S_i = sum of fl64(x)^2 over the window  >=  fl64(thr) * fl64(thr) * fl64(W)
 *         (float64 throughout; every square is the exact product of the fp32 sample; the reference compares
 *          sqrt(mean(x^2)) >= thr in fp32, which is the same test up to fp32 rounding at the threshold)
 *     start = max(0, first s - m),   end = min(n, last s + m)      (first / last: the first / last speech window)
 * end counts from the last speech window's START plus the margin, not from its end: that is the reference's behaviour.  The
 * reference passes W = int(0.1 sr), s = W / 10 (integer), m = 2 W, thr = 0.01.  Two cases are defined here and not by the
 * reference, which raises in both: n < W: the row is kept whole, (0, n); no window is speech: (0, 0), an empty piece.
 * Two launches whatever B: k_trim_scan, grid (tiles of 64 windows, rows) -- a block stages the samples its windows span in LDS
 * once, a wave sums a window from there (lane l takes samples l, l + 64, ... in ascending order, then a fixed butterfly) and
 * the block writes its tile's first and last speech window to work_dev --, then k_trim_bounds, one wave a row.  No atomics.
 * Guarantee: a row's bounds depend on its samples, n and the parameters alone -- not on B, the row's place, the strides, what
 * lies past n or the grid.  64 windows must fit the LDS: 63 s + W <= 16320, else SMI_EINVAL.  n <= 2^24, B <= 64.
 *
 * Assembly (smi_concat_rows): piece b is p = x_b[start_b .. end_b), L samples, behind gap_b >= 0 samples of silence; f >= 0
 * is the fade length, f' = min(f, L / 2) (integer division):
 *     w_q = fl64(q + 1) / fl64(f' + 1)                              (one correctly rounded float64 division)
 *     p[q] and p[L - 1 - q], q < f', become fl32( fl64(p[.]) * w_q )   (one float64 product, one rounding; no FMA, no table)
 * -- where the two edges meet in a piece of odd length the middle sample is untouched.  out holds the pieces in row order, each
 * behind its gap, then zeros from the total length to cap.  An empty piece (end = start) writes nothing, and neither is its gap
 * written.  One launch for the whole call, grid (tiles of 1024 samples, B + 1): row b writes gap b and piece b, row B the
 * zeros.  A sample's bits depend on its piece and f alone.  Lengths and offsets are host arithmetic (smi_concat_layout). */
/* int32 elements of work_dev that smi_trim_rows needs for B rows of at most n_max samples; -1 for a bad argument.  Pure host. */
long long smi_trim_work_len(long long n_max, int window, int step, int B);
/* in_dev [B][in_stride] f32 (row b valid for n_host[b], 0 .. min(in_stride, 2^24)); work_dev [work_len] int32 scratch (contents
 * do not matter before, mean nothing after); bounds_dev [B][2] int32 receives (start, end) of every row. */
int smi_trim_rows(const float* in_dev, long long in_stride, const int32_t* n_host, int B, int window, int step, double threshold,
                  int margin, int32_t* work_dev, long long work_len, int32_t* bounds_dev, void* stream);
/* The total length of the assembled waveform; offset_host [B] (may be null) receives where each piece begins in it (behind its
 * gap; for an empty piece: where it would).  -1 for B outside 1..64, a negative start or gap, or end < start.  Pure host. */
long long smi_concat_layout(const int32_t* start_host, const int32_t* end_host, const int32_t* gap_host, int B, long long* offset_host);
/* in_dev [B][in_stride] f32, row b valid for n_host[b]; 0 <= start_host[b] <= end_host[b] <= n_host[b]; out_dev [cap] f32,
 * cap >= max(1, total), below 2^31; must not overlap in_dev.  offset_host [B] / total_host (may be null) as smi_concat_layout,
 * filled before the launch. */
int smi_concat_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host,
                    const int32_t* gap_host, int B, int fade, float* out_dev, long long cap, long long* offset_host, long long* total_host,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Output loudness: the programme loudness of rows after ITU-R BS.1770 (K-weighting, 400 ms blocks, absolute and relative gate)
 * and the gain that brings each row to a target under a peak ceiling, measured and applied on the device.  Free functions like
 * the long-form edge above: no handle, no state, asynchronous on the caller's stream, never synchronising, opt-in.  Every
 * argument of every row is checked before anything reaches the device: a bad one returns SMI_EINVAL, names the argument in
 * smi_last_error and launches nothing.  B <= 64, n <= 2^24.
 *
 * A row is measured over a span x[start .. end) of L samples.  Samples before start and from end on are never read; the filter
 * starts from zero state (zero input and output history) at start.
 *
 * K-weighting.  Two cascaded biquads in direct form I, float64; coef_host[10] = b0 b1 b2 a1 a2 of stage 1, then of stage 2, is
 * data the caller passes (sparkmi/audio.py: k_weighting derives it for a sample rate; the device designs no filter).  Every
 * fp32 sample enters as its exact float64 value v.  With the stage's last inputs v1, v2 and last outputs y1, y2:
 *     w = ((fl(b0 v) + fl(b1 v1)) + fl(b2 v2)) - fl(a2 y2),    y = w - fl(a1 y1)
 * -- every product and sum rounded on its own (no FMA), in that order; stage 2 takes stage 1's y as its v.
 * Segments.  The span is cut into segments of 128 samples (a constant of the arithmetic, not of the call).  The state of the
 * cascade, s = (y1, y2 of stage 1, y1, y2 of stage 2), at the start of segment k + 1 is
 *     s_{k+1} = T s_k + e_k,   s_0 = 0
 * where e_k is the state at the end of segment k filtered from s = 0 (with its true input history: the two samples before it),
 * T is the 4x4 matrix whose column i is unit state i after 128 samples of silence -- computed on the host in float64 by the
 * recurrence above --, and row i of the product is (((fl(T_i0 s_0) + fl(T_i1 s_1)) + fl(T_i2 s_2)) + fl(T_i3 s_3)) + e_i.  Each
 * segment is then filtered from s_k.  In exact arithmetic that is the sequential filter; in float64 it differs from it by
 * rounding only (DESIGN.md 4.1.3 derives the bound).
 * Blocks.  block = the caller's sample count for 400 ms, a multiple of 4; hop = block / 4.  Block j covers [j hop, j hop + block)
 * for j = 0 .. floor((L - block) / hop); a tail shorter than a hop is dropped.  y^2 is summed in ascending sample order within
 * a hop part (the piece of a hop inside one segment), the parts of a hop in ascending order from 0, and
 *     z_j = (((H_j + H_{j+1}) + H_{j+2}) + H_{j+3}) / fl64(block).
 * Gates, both in the linear domain.  A = 10^((-70 + 0.691) / 10), computed once on the host.  Block j passes the absolute gate
 * when z_j > A; of those, it passes the relative gate when z_j > fl64(0.1 * (sum of the passing z / their count)).  A sum over
 * blocks takes j = t, t + 256, ... in ascending order for t = 0 .. 255, then adds the 256 partial sums in a fixed tree (t and
 * t + 128, then t and t + 64, ...).  loudness = -0.691 + 10 log10(sum of the z passing both gates / their count).
 * Defined here where the standard is silent:  1 <= L < block: one block, the whole span, z = (the hop sums in ascending
 * order) / fl64(L), and the absolute gate alone;  no block passes, or L = 0: loudness = -inf, gain = 1, limit = 0.
 * Peak.  peak = max |x| over the span, exact.  It is a SAMPLE peak: the 4x oversampled true peak is not measured
 * (not here: smi_limit_rows below measures it and holds the ceiling sample by sample).
 * Gain, float64, formed on the device:  g = 10^((target - loudness) / 20);  g = min(g, 10^(max_gain_db / 20)) (limit = 1 where
 * that binds);  if g * peak > ceiling then g = ceiling / peak (limit = 2).  A NaN target measures only: g = 1, limit = 0.
 * Apply (smi_gain_rows).  out[i] = fl32(fl64(x[i]) * g): one float64 product, one rounding, no FMA.
 *
 * Launches, whatever B: k_loud_seg, grid (tiles of 64 segments, rows) -- a wave stages its tile in LDS with coalesced reads and
 * each lane filters one segment from zero state --; k_loud_carry, one wave a row, the recurrence of s_k; k_loud_energy, the
 * grid of k_loud_seg, each segment again from s_k, writing hop parts and the segment's max |x|; k_loud_gate, one block a row.
 * smi_gain_rows is one launch, grid (tiles of 1024 samples, rows).  No atomics.  Guarantee: a row's four stats, bit for bit,
 * depend on its span and the parameters alone -- not on B, the row's place, the strides, what lies outside the span or the grid. */
/* float64 elements of work_dev that smi_loud_rows needs for B rows of at most n_max samples; -1 for a bad argument.  Pure host. */
long long smi_loud_work_len(long long n_max, int block, int B);
/* in_dev [B][in_stride] f32, row b valid for n_host[b]; 0 <= start_host[b] <= end_host[b] <= n_host[b] (both null: the whole
 * row); target_host [B] float64 (LUFS; NaN: measure only); max_gain_db >= 0; ceiling > 0; work_dev [work_len] float64 scratch
 * (contents do not matter before, mean nothing after); stats_dev [B][4] float64 receives (loudness, peak, gain, limit). */
int smi_loud_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                  const double* coef_host, int block, const double* target_host, double max_gain_db, double ceiling, double* work_dev,
                  long long work_len, double* stats_dev, void* stream);
/* Row b of out_dev [B][out_stride] receives the row's n samples -- the span times stats_dev[b][2], read from the device, the
 * rest copied -- and zeros from n to out_stride (>= the longest row).  out_dev == in_dev with equal strides is allowed (in
 * place); any other overlap is refused. */
int smi_gain_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                  const double* stats_dev, float* out_dev, long long out_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * Output limiter: a look-ahead limiter with true-peak detection that keeps every sample of a row at or under a ceiling by
 * reducing the gain around the overs only -- it starts ahead of them and recovers smoothly behind them --, on the device.  Free
 * functions like the sections above: no handle, no state, asynchronous on the caller's stream, never synchronising, opt-in.
 * Every argument of every row is checked before anything reaches the device: a bad one returns SMI_EINVAL, names the argument
 * in smi_last_error and launches nothing.  B <= 64, n <= 2^24.  The limiter is feed-forward -- a sliding minimum followed by
 * FIR smoothing --: no recursion, no carry, no order of segments, so a sample's bits follow from the definition alone.
 *
 * A row is limited over a span x[start .. end) of L samples, taken to be finite.  Samples outside the span are never read: they
 * count as zero for the oversampler and as "no over" (r = 1) for the gain, and they are copied through unchanged, as
 * smi_gain_rows copies them.  Everything is float64; fl() is one rounding: every product and every sum is rounded on its own
 * (no FMA).  i and j index the span.
 *
 * 1 Envelope.  e[i] = max(|x[i]|, |u_1[i]|, .., |u_{P-1}[i]|), P = phases.  u_k[i], the interpolated value at time i + k / P, is
 *     u_k[i] = sum over d = -10 .. 9, ascending from 0, of fl(h[P d + k + H] * fl64(x[i - d]))
 *   -- every tap of phase k.  h = taps_host: 2 H + 1 float64 taps, H = 10 P, data the caller passes (sparkmi/audio.py:
 *   resample_taps(P, 1), the resampler's own low-pass; the device designs no filter).  n_taps = 0: e[i] = |x[i]|, the
 *   sample-peak mode.  Phase 0 is the sample itself, so the sample peak is always covered exactly.
 * 2 Required gain.  v = fl(g * e[i]);  r[i] = ceiling / v (one correctly rounded division) where v > ceiling, else 1.  g is the
 *   row's gain, read from device memory: gain_dev[b * gain_stride]; a null gain_dev: g = 1.  (The gain of smi_loud_rows' stats
 *   is stats_dev + 2 with stride 4.)
 * 3 Look-ahead minimum.  m[i] = min r[j] over i - R <= j <= i + A, r = 1 outside the span; A = lookahead, R = release, in
 *   samples, 0 <= A <= 256, 0 <= R <= 2048.  m is defined outside the span as well.
 * 4 Smoothing.  s'[i] = 1 - (the sum over k = -R .. A, ascending from 0, of fl(w[k + R] * fl(1 - m[i - k])));
 *   s[i] = min(s'[i], r[i]).  w = win_host: A + R + 1 non-negative float64 weights, |sum of w (ascending) - 1| <= 1e-12, data
 *   the caller passes (sparkmi/audio.py: limiter_window).  The sum is taken on the reduction 1 - m, so s is exactly 1 where no
 *   over lies within A + R samples on either side.  Every m[i - k] of the sum has i inside its window, so s'[i] <= r[i] in exact
 *   arithmetic; the min removes the last rounding.
 * 5 Apply.  out[i] = fl32(fl(fl(fl64(x[i]) * g) * s[i])), then clamped to +-c32, the largest float32 <= ceiling.  Since
 *   |fl64(x[i]) g s[i]| <= ceiling up to rounding, the clamp can only move a value by the final float32 rounding.
 * 6 Stats, [4] float64 a row, all exact: fl(g * max e) -- the true peak going in (the sample peak with n_taps = 0) --; g;
 *   min s; the count of samples with s < 1.  L = 0: (0, g, 1, 0).
 *
 * Guarantees.  A row's output and stats, bit for bit, depend on its span and the parameters alone -- not on B, the row's
 * place, the strides, what lies outside the span or the grid.  |out[i]| <= ceiling for every sample of the span, exactly.  Where
 * s[i] == 1, out[i] is smi_gain_rows' fl32(fl64(x[i]) g) bit for bit (but for a product in (c32, ceiling] that float32 rounds
 * up past the ceiling, which the clamp brings to c32).  What the limiter does not promise: the true peak of the OUTPUT is
 * held only as far as a gain that varies between samples allows (DESIGN.md 4.1.7 records the overshoot measured).
 *
 * Launches, whatever B, no atomics: k_limit_win, ceil((A + R + 1) / 384) launches of one block that carry the window to
 * work_dev as kernel arguments (no copy is enqueued, nothing waits); k_limit_env, grid (tiles of 1024 samples of the span,
 * rows) -- the tile and 10 samples on either side staged in LDS, r and the tile's max e to work_dev --; k_limit_apply, grid
 * (tiles of 1024 samples up to out_stride, rows) -- r over the tile and A + R samples on either side staged in LDS, the minimum
 * formed there in place by doubling, then the smoothing sums, the product, the clamp, and the tile's min s and count to
 * work_dev --; k_limit_stats, one block a row.  r travels through work_dev, so out_dev == in_dev is allowed. */
/* float64 elements of work_dev that smi_limit_rows needs for B rows of at most n_max samples; -1 for a bad argument.  Pure host. */
long long smi_limit_work_len(long long n_max, int B);
/* in_dev [B][in_stride] f32, row b valid for n_host[b]; 0 <= start_host[b] <= end_host[b] <= n_host[b] (both null: the whole
 * row); gain_dev (may be null) and gain_stride >= 0 as in 2; ceiling > 0; taps_host [n_taps], n_taps = 0 or 20 phases + 1,
 * 1 <= phases <= 8; win_host [lookahead + release + 1]; work_dev [work_len] float64 scratch (contents do not matter before,
 * mean nothing after).  Row b of out_dev [B][out_stride] receives the row's n samples -- the span limited, the rest copied --
 * and zeros from n to out_stride (>= the longest row); out_dev == in_dev with equal strides is allowed (in place), any other
 * overlap is refused.  stats_dev [B][4] float64 as in 6; it must not overlap gain_dev. */
int smi_limit_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const double* gain_dev, int gain_stride, double ceiling, const double* taps_host, int n_taps, int phases, int lookahead,
                   int release, const double* win_host, double* work_dev, long long work_len, float* out_dev, long long out_stride,
                   double* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tempo: a pitch-preserving time-scale change of rows (WSOLA: overlap-add of frames whose places are found by a waveform
 * similarity search), on the device.  Free functions like the two sections above: no handle, no state, asynchronous on the
 * caller's stream, never synchronising, opt-in.  Every argument of every row is checked before anything reaches the device: a
 * bad one returns SMI_EINVAL, names the argument in smi_last_error and launches nothing.  B <= 64, L <= 2^24.
 *
 * A row is scaled over a span x[0 .. L) = row[start .. end) of fp32 samples.  Everything outside the span reads as 0 and is
 * never fetched from memory.  The tempo is the rational p / q (> 1: faster), 1 <= p, q <= 32767, 1/4 <= p / q <= 4.  The frame
 * N is even, 16 <= N <= 2048, H = N / 2; the search radius is 0 <= D <= 1024.
 *
 * Quantised copy, for decisions only:  qx[i] = clamp(rint(fl64(x[i]) * 32767), -32767, 32767) -- the product is exact in
 * float64, rint rounds half to even; a NaN sample gives 0, and so does every position outside the span.
 * Lengths, host integer arithmetic (smi_tempo_layout):  M = ceil(L q / p) output samples in K = floor((M - 1) / H) + 1 frames
 * (K = 0 when M = 0).  Frame k's nominal place is a_k = floor(k H p / q), in 64-bit integers.
 * Frame places s_k.  s_0 = 0.  For k >= 1 the natural continuation is t_k = s_{k-1} + H, and s_k = a_k + delta where delta in
 * [-D, D] minimises the exact distance
 *     sum over i < N of (qx[t_k + i] - qx[a_k + delta + i])^2
 * -- every term is below 2^32 and the sum below 2^43, so it is exact in 64-bit integers and its order is free.  Ties go to the
 * smallest |a_k + delta - t_k|, then to the smaller delta.  Where |t_k - a_k| <= D this rule gives s_k = t_k without a search
 * (the distance there is 0 and nothing is closer to t_k): the kernel takes that shortcut; it is not a second rule.
 * Overlap-add.  w[i] = 0.5 - 0.5 cos(2 pi i / N), float64, is a table the caller passes (sparkmi/audio.py: tempo_window; the
 * device designs no window).  For output sample m, k = m / H (integer division) and j = m - k H:
 *     k = 0:   out[m] = x[m]
 *     k >= 1:  out[m] = fl32( fl(fl64(x[s_k + j]) w[j]) + fl(fl64(x[s_{k-1} + j + H]) w[j + H]) )
 * -- each product and the sum rounded on their own in float64 (no FMA), then one rounding to fp32.
 * Consequences.  At p = q every s_k = k H and the output is the span bit for bit.  M and K depend on L, p, q and N alone.
 *
 * Two launches whatever B.  k_tempo_search, one block a row: the frames in order (t_k hangs on s_{k-1}); a searched frame's
 * quantised target and candidate samples -- at most 2 N + 2 D int16 -- are staged in LDS, the candidates are spread over the
 * block's threads, each sums its distance in a 64-bit integer, and the block reduces to the minimum under the tie rule.
 * k_tempo_ola, grid (tiles of 1024 output samples, rows).  No atomics.  Guarantee: a row's places and samples depend, bit for
 * bit, on its span and its own p, q, N, D and window alone -- not on B, the row's place, the strides, what lies outside the
 * span or the grid. */
/* M, the output length of a span of L samples (0 .. 2^24) at tempo p / q with frame N; K_out (may be null) receives the frame
 * count.  -1 for a bad argument.  Pure host. */
long long smi_tempo_layout(long long L, int p, int q, int N, long long* K_out);
/* in_dev [B][in_stride] f32, row b valid for n_host[b]; 0 <= start_host[b] <= end_host[b] <= n_host[b] (both null: the whole
 * row); p_host / q_host [B]: every row's own tempo; win_dev [N] float64; pos_dev [B][pos_stride] int32 receives s_k (relative
 * to the span's start), then zeros to pos_stride (>= the most frames of a row, >= 1); out_dev [B][out_stride] f32 receives the
 * row's M samples, then zeros to out_stride (>= the longest output, >= 1, <= 2^26), and must not overlap in_dev; m_host [B]
 * (may be null) receives every M, filled before the launch. */
int smi_tempo_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const int32_t* p_host, const int32_t* q_host, int N, int D, const double* win_dev, int32_t* pos_dev, long long pos_stride,
                   float* out_dev, long long out_stride, int32_t* m_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pitch shift of rows: the frequency ratio of a row changed at an unchanged or separately chosen length, on the device.  It is
 * the tempo section's stretch followed by the resampler section's polyphase sum and a cut, with the pitch and the tempo
 * sharing ONE stretch pass.  Free functions like smi_tempo_rows: no handle, no state, asynchronous on the caller's stream, never
 * synchronising, opt-in.  Every argument of every row is checked before anything is launched: a bad one returns SMI_EINVAL,
 * names the argument in smi_last_error and leaves the output untouched.  B <= 64, L <= 2^24.
 *
 * For a span x[0 .. L) = row[start .. end), a tempo t = tp / tq (> 1: faster) and a pitch ratio r = rp / rq (> 1: higher),
 * 1 <= tp, tq, rp, rq <= 32767 (host integer arithmetic, smi_pitch_layout):
 * Stretch.   P / Q = (tp rq) / (tq rp) in lowest terms, within the tempo section's ranges (1 <= P, Q <= 32767,
 *            1/4 <= P / Q <= 4).  z[0 .. M) is smi_tempo_rows' result on the span at tempo P / Q -- the same N, D and window,
 *            the same integer search and tie rule, the same places s_k, K of them --, M = ceil(L Q / P).
 * Resample.  up / down = rq / rp in lowest terms.  With taps h[0 .. 2H] (fp32, caller data; sparkmi/audio.py passes
 *            resample_taps(up, down) rounded to fp32 once, H = 10 max(up, down)):
 *                y[k] = sum_j z[j] h[H + k down - j up]
 *            in smi_rs_resample_rows' order: j ascending from ceil((k down - H) / up), clamped at 0, to
 *            floor((k down + H) / up), clamped at M - 1 -- the edges are zero-padded against z's own length M --, fp32, one
 *            accumulator, the product and the sum rounded separately (no FMA).
 * Length.    The row's output is y[0 .. n_out), n_out = ceil(L tq / tp): what smi_tempo_rows alone gives at tp / tq, and L
 *            without a tempo.  ceil(M up / down) >= n_out (refused otherwise; for every hundredth r in [0.5, 2] and t in
 *            [0.5, 2] the surplus is 0 to 2 samples); the surplus is cut.
 * Consequences.  At rp = rq the row is smi_tempo_rows' row at tp / tq bit for bit, and at tp = tq too it is the span bit for
 * bit.  P, Q, M, K, up, down and n_out depend on L, tp, tq, rp, rq and N alone.  The formants move with the pitch: this is the
 * stretch-and-resample construction, not a pitch-synchronous one.
 *
 * Two launches whatever B, no atomics.  k_tempo_search as in the tempo section, with P / Q per row.  k_pitch_ola, grid (tiles of
 * 1024 final output samples, rows): a block stages its row's taps in LDS, computes the stretched samples its tile's sums reach
 * -- at most (1023 down + 2 H) / up + 3 of them, each by the tempo section's overlap-add from the places and the input --
 * straight into LDS, and after one barrier forms its sums; z never exists in memory.  A row at rp = rq writes the overlap-add
 * itself.  A row whose taps plus one tile's stretched window exceed 16384 floats of LDS is refused (the worst hundredth ratio,
 * 199/100, needs 6059).  Guarantee: a row's places and samples depend, bit for bit, on its span and its own tp, tq, rp, rq, N,
 * D, window and taps alone -- not on B, the row's place, the strides, what lies outside the span or the grid. */
/* n_out of a span of L samples (0 .. 2^24); P_out, Q_out, M_out, K_out, up_out, down_out (each may be null) receive the rest of
 * the plan.  -1 for a bad argument.  Pure host. */
long long smi_pitch_layout(long long L, int tp, int tq, int rp, int rq, int N, int* P_out, int* Q_out, long long* M_out, long long* K_out,
                           int* up_out, int* down_out);
/* in_dev, in_stride, n_host, start_host, end_host, B, N, D, win_dev as in smi_tempo_rows; tp_host / tq_host / rp_host / rq_host
 * [B]: every row's own tempo and pitch ratio; taps_dev [taps_len] f32: a pool of taps on the device, of which row b uses
 * n_taps_host[b] (odd, >= 3) from tap_off_host[b] on -- n_taps_host[b] = 0, and only 0, for a row whose rp / rq is 1/1; pos_dev
 * [B][pos_stride] int32 receives the stretch's s_k, then zeros to pos_stride (>= the most frames of a row, >= 1); out_dev
 * [B][out_stride] f32 receives the row's n_out samples, then zeros to out_stride (>= the longest output, >= 1, <= 2^26), and
 * must not overlap in_dev or taps_dev; m_host [B] (may be null) receives every n_out, filled before the launch. */
int smi_pitch_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const int32_t* tp_host, const int32_t* tq_host, const int32_t* rp_host, const int32_t* rq_host, int N, int D,
                   const double* win_dev, const float* taps_dev, long long taps_len, const int32_t* tap_off_host, const int32_t* n_taps_host,
                   int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride, int32_t* m_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tempo of joined streams: the arithmetic above with state carried from push to push, so that a stream whose input arrives in
 * chunks (a joined stream of smi_join at 1/1) leaves in pieces before it has ended.  No sample is defined here: the
 * concatenation of a stream's pieces is smi_tempo_rows of its whole input.  What is new is the state and the rule for when an
 * output sample is final.
 *
 * When a frame is final.  A stream is an input sequence x with n samples so far; its total L is known only with the last push.
 * H, a_k, t_k, s_k, M as above.  R_0 = H, and for k >= 1
 *     R_k = max(a_k, a_{k-1} + H) + D + N.
 * Frame k is final once n >= R_k: frame 0 copies x[0 .. H); for k >= 1 the target [t_k, t_k + N) ends at or before
 * a_{k-1} + D + H + N because t_k = s_{k-1} + H <= a_{k-1} + D + H, every candidate ends at or before a_k + D + N, and the two
 * overlap-add reads end before s_k + H <= a_k + D + H and s_{k-1} + N <= a_{k-1} + D + N -- all inside x[0 .. n), so nothing
 * the frame reads can change and nothing of it is the zero the batch reads beyond L.  R_k does not fall as k grows, and s_k
 * hangs on s_{k-1}, so final frames are emitted as a prefix.  A frame is emitted before the last push only when, in addition,
 * (k + 1) H <= ceil(n q / p): then it is whole in the final M = ceil(L q / p) >= ceil(n q / p).  After a push that is not the
 * last the stream has emitted E(n) = H F outputs, F the count of such frames; after the last push it has emitted M, the
 * remaining frames computed as the batch computes them, with zeros read beyond L.  A push emits the difference, which may be 0.
 * All of it is host integer arithmetic (smi_tempos_piece_len), never data.  A stream opened at p = q is a copy with no latency:
 * there the batch output is the input, and a push emits its chunk.  Otherwise the first piece waits for N + D + up to H
 * samples beyond the frame's nominal place.
 *
 * State.  On the host: n, F, p, q.  On the device, per stream: s_{F-1}, which is data-dependent and never copied back, and the
 * input from h(F) = max(0, min(a_F, a_{F-1} + H) - D) (h(0) = 0) to n: the first sample frame F can still read -- its target
 * starts at or after a_{F-1} - D + H, its candidates at a_F - D, its overlap-add reads at s_F >= a_F - D and s_{F-1} + H.
 * h(F) does not fall as F grows.  The history n - h(F) is bounded: frame F was not emitted, so either n < R_F, and then
 *     n - h(F) < |a_F - a_{F-1} - H| + 2 D + N <= 3 H + 2 D + N = 5 H + 2 D        (0 <= a_F - a_{F-1} <= 4 H),
 * or (F + 1) H > ceil(n q / p), so n < (F + 1) H p / q, and then with a_k > k H p / q - 1
 *     n - a_F + D < H p / q + 1 + D <= 4 H + 1 + D   and   n - a_{F-1} - H + D < 2 H p / q - H + 1 + D <= 7 H + 1 + D.
 * The handle keeps max(7 H + D, 5 H + 2 D) samples per stream and set, which is enough for every p / q in 1/4 .. 4; a push
 * makes at most 4 (max_chunk + that history) / H + 4 frames final.  Histories and places live in two sets that a stream uses in
 * turn: a push reads one and writes the other, so one launch sequence serves a call whatever B.
 *
 * Two launches a call.  k_tempos_search, one block a row, walks the row's newly final frames in order over the virtual
 * sequence of history followed by the new chunk, with the device functions k_tempo_search calls (distance, tie rule,
 * shortcut), and writes s_k; k_tempos_ola, grid (tiles of 1024 samples of the pieces, rows), forms the samples with
 * k_tempo_ola's expression and writes the next history.  No atomics.
 *
 * Guarantees: the concatenation of a stream's pieces is, bit for bit, smi_tempo_rows of its whole input at the same p, q, N, D
 * and window, and the frame places are equal too -- whatever the granularity of the pushes, the stream's slot, its row in a
 * call and the other rows.  A piece's length is pure host arithmetic; nothing synchronises and nothing is copied back.  A
 * stream is refused (SMI_EINVAL) before n passes 2^28.  All pushes of a handle must go to one HIP stream (or be ordered by the
 * caller). */
typedef struct smi_tempos smi_tempos;
/* max_streams (1..4096) slots; max_chunk (1..2^24) samples a push; N, D as for smi_tempo_rows; win_host [N] float64, the
 * window.  Synchronous (one allocation, one small copy). */
int smi_tempos_create(int max_streams, int max_chunk, int N, int D, const double* win_host, smi_tempos** out);
int smi_tempos_destroy(smi_tempos* h);
/* A new stream in slot `stream` at tempo p / q (ranges as for smi_tempo_rows): n and F are zero.  Host only.  A stream closes
 * with its last push. */
int smi_tempos_open(smi_tempos* h, int stream, int p, int q);
/* One chunk per row: in_dev [B][stride] f32 (row b valid for len_host[b], which may be 0), of the open streams stream_host[b],
 * each at most once in a call; last_host[b] = 1 on a stream's last push.  out_dev [B][out_stride] f32: row b receives its piece
 * and zeros from there to out_stride (>= 1 and >= the longest piece); it must not overlap in_dev.  pos_dev (may be null)
 * [B][pos_stride] int32 receives the places of the frames this push made final, in order, then zeros to pos_stride (>= 1 and
 * >= the most frames of a piece).  n_out_host [B] (may be null) receives the pieces' lengths, filled before the launch.
 * B <= 64.  Asynchronous on `stream`.  Every argument of every row is checked before anything changes or is launched: a bad one
 * returns SMI_EINVAL and names the argument in smi_last_error. */
int smi_tempos_push_rows(smi_tempos* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride,
                         int32_t* n_out_host, void* stream);
/* The piece length of one push, pure host arithmetic: a stream at p / q with frame N and radius D that holds n_before samples
 * and has emitted frames_before frames takes len samples (last = 1: its last push); n_after / frames_after (may be null)
 * receive the counters after it (at p = q the frames are the whole frames of n, which nothing depends on).  -1 for a bad
 * argument. */
long long smi_tempos_piece_len(int p, int q, int N, int D, long long n_before, long long frames_before, long long len, int last,
                               long long* n_after, long long* frames_after);

/* ------------------------------------------------------------------------------------------
 * Pitch shift of joined streams: the pitch section's arithmetic with state carried from push to push, the streaming form of
 * smi_pitch_rows as smi_tempos_* is that of smi_tempo_rows.  No sample is defined here: the concatenation of a stream's pieces
 * is smi_pitch_rows of its whole input at the same tp / tq, rp / rq, N, D, window and taps, bit for bit, and the stretch's frame
 * places are equal too.  What is new is the rule for when an output sample is final, and the state.
 *
 * When an output is final.  Host integer arithmetic only (smi_pitchs_piece_len), never data.  P / Q, up / down as in the pitch
 * section; taps h[0 .. 2G].  With n input samples so far, the stretch is smi_tempos_*' stream at P / Q and has emitted E(n)
 * stretched samples z[0 .. E), exactly as smi_tempos_piece_len gives (E = n at P = Q).  After a push that is not the last the
 * stream has emitted
 *     K(n) = max(0, ceil((E(n) up - G) / down))
 * final outputs -- smi_join's own expression, applied to the stretched stream: output k reads z up to floor((k down + G) / up),
 * which lies below E exactly when k down + G < E up, so the sums of the first K outputs reach nothing that is not final, and
 * their edge needs no clamp.  After the last push, with total length L, it has emitted n_out = ceil(L tq / tp): the remaining
 * sums are clamped at M - 1, M = ceil(L Q / P), as the batch call clamps them, and the surplus is cut.  A push emits the
 * difference, which may be 0.  K(n) never falls, since E never does.  K(n) <= ceil(n tq / tp), so what has left is at most the
 * final n_out whatever follows: E <= ceil(n Q / P) < n Q / P + 1 gives E up / down < n tq / tp + up / down, and
 * K < (E up - G) / down + 1 <= n tq / tp + 1 once G >= up; a stream with G < up is refused at open.  At rp = rq (up = down = 1,
 * no taps, G = 0) K = E: the stream is smi_tempos_*' stream at tp / tq bit for bit, and with tp = tq too it copies its chunks
 * with no latency.  Otherwise a piece is the tempo stream's hold-back at P / Q plus G / up stretched samples late.
 *
 * State.  On the host, per slot: n, the emitted frames F, the emitted outputs K, tp, tq, rp, rq.  On the device, per slot, in
 * two sets used in turn as in smi_tempos_* (a push reads one and writes the other, so a refused call has changed nothing):
 * smi_tempos_*' own state at P / Q -- s_{F-1} and the input from h(F), at most max(7 H + D, 5 H + 2 D) samples -- and the tail
 * of the stretched signal that later outputs still reach, z[j(K) .. E), j(K) = max(0, ceil((K down - G) / up)), the first
 * sample of output K's sum.  Where K > 0, K down >= E up - G, so j(K) >= E - 2 G / up and the tail holds at most 2 G / up
 * samples; where K = 0, E up <= G and the tail is E <= G / up samples.  The handle keeps max_taps + 1 per slot and set, which is
 * more than either, and a push whose tail would not fit is refused.  These are the only stretched samples that ever reach
 * memory; they are the values the overlap-add produced, so the bits cannot differ from computing them again.  The slot also
 * owns a copy of its stream's taps (fp32, at most max_taps of them), handed over at open.
 *
 * Two launches a call, whatever B, no atomics.  k_tempos_search as in the section above, with P / Q per row.  k_pitchs_ola, grid
 * (tiles of 1024 final outputs of the pieces, rows; every row has a tile): a block stages its row's taps in LDS, fills the
 * window of stretched samples its sums reach straight into LDS -- those below E before the push from the read set's tail, the
 * others by the tempo section's overlap-add over history and chunk, reading zeros beyond L on the last push --, and after one
 * barrier forms its sums; zeros from the piece's end to the stride.  A row at up = down = 1 writes the overlap-add itself.  Tile
 * 0 of a row also writes the written set's input history and stretched tail.  A stream whose taps plus one tile's stretched
 * window, (1023 down + 2 G) / up + 3 samples, exceed 16384 floats of LDS is refused at open, as the batch call refuses the row.
 *
 * Guarantees: as for smi_tempos_* -- pieces and places are those of smi_pitch_rows of the whole input whatever the granularity
 * of the pushes, the stream's slot, its row in a call and the other rows; a piece's length is pure host arithmetic; nothing
 * synchronises and nothing is copied back.  A stream is refused (SMI_EINVAL) before n passes 2^28 or E up or K down reaches
 * 2^31.  All opens and pushes of a handle must go to one HIP stream (or be ordered by the caller). */
typedef struct smi_pitchs smi_pitchs;
/* max_streams, max_chunk, N, D, win_host as for smi_tempos_create; max_taps (0 .. 16383): the longest filter a stream of this
 * handle may bring.  Synchronous (one allocation, one small copy). */
int smi_pitchs_create(int max_streams, int max_chunk, int N, int D, const double* win_host, int max_taps, smi_pitchs** out);
int smi_pitchs_destroy(smi_pitchs* h);
/* A new stream in `slot` at tempo tp / tq and pitch ratio rp / rq (ranges as for smi_pitch_rows): n, F and K are zero.
 * taps_host [n_taps] f32: the stream's filter h[0 .. 2G], n_taps odd and >= 3 -- or 0, and only 0, at rp = rq.  Refused:
 * G < up, n_taps > max_taps, and a filter that does not fit the LDS (above).  The taps are copied into the slot on `stream`,
 * ordered behind the slot's earlier pushes there and before later ones; taps_host is free on return.  A stream closes with its
 * last push.  A refused open has changed nothing. */
int smi_pitchs_open(smi_pitchs* h, int slot, int tp, int tq, int rp, int rq, const float* taps_host, int n_taps, void* stream);
/* Arguments and checks as for smi_tempos_push_rows: one chunk per row of the open streams stream_host[b], each at most once in
 * a call, len_host[b] may be 0, last_host[b] = 1 on a stream's last push; out_dev [B][out_stride] receives row b's piece and
 * zeros from there to out_stride (>= 1 and >= the longest piece) and overlaps neither in_dev nor the handle's state; pos_dev
 * (may be null) [B][pos_stride] receives the places of the stretch's frames this push made final, then zeros; n_out_host [B]
 * (may be null) receives the pieces' lengths, filled before the launch.  B <= 64.  Asynchronous on `stream`; it never
 * synchronises.  Every argument of every row is checked before anything changes or is launched: a bad one returns SMI_EINVAL
 * and names the argument in smi_last_error. */
int smi_pitchs_push_rows(smi_pitchs* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride,
                         int32_t* n_out_host, void* stream);
/* The piece length of one push, pure host arithmetic: a stream at tp / tq and rp / rq with frame N, radius D and n_taps taps
 * that holds n_before samples and has emitted frames_before frames of the stretch and k_before outputs takes len samples
 * (last = 1: its last push); n_after / frames_after / k_after (may be null) receive the counters after it.  -1 for a bad
 * argument, among them G < up and counters that reach the limits above. */
long long smi_pitchs_piece_len(int tp, int tq, int rp, int rq, int N, int D, int n_taps, long long n_before, long long frames_before,
                               long long k_before, long long len, int last, long long* n_after, long long* frames_after,
                               long long* k_after);

/* ------------------------------------------------------------------------------------------
 * Loudness of joined streams: a running BS.1770 gain with state carried from push to push.  Integrated loudness is a property
 * of the whole utterance, which a piece that has to leave early cannot know, so this is NOT smi_loud_rows run chunk by chunk;
 * it has a definition of its own.  The gain follows the integrated loudness of what has arrived, moves at a bounded rate and
 * stays under the peak ceiling, and everything is defined on the stream's absolute sample index, so that the chunking cannot
 * change a bit.
 *
 * Measuring is the section "Output loudness" above, unchanged, on a stream x[0 .. n) whose total L is known only with the
 * last push: the K-weighting from zero state at sample 0, segments of 128 samples counted from sample 0 with the carry
 * s_{k+1} = T s_k + e_k, y^2 summed into hop parts and the parts into hops H_h in ascending order, and
 * z_j = (((H_j + H_{j+1}) + H_{j+2}) + H_{j+3}) / fl64(block); hop = block / 4.  The kernels call smi_loud_rows' own device
 * functions.  Consequence: after the last push the hop sums, the z_j and the gated loudness over all blocks are those of
 * smi_loud_rows over the whole stream, bit for bit.
 *
 * Knots.  Knot j sits at sample j hop and is formed once blocks 0 .. j are whole, that is when n >= (j + 4) hop.  Every step is
 * float64 and rounded on its own (no FMA); G_{j-1} is the knot before.
 *   Running loudness.  I_j is the gated loudness over z_0 .. z_j: both gates as above (the relative threshold from the blocks
 *     0 .. j that pass the absolute one) and the sums in the order given there: j' = t, t + 256, ..., then the fixed tree.
 *   Target gain.  A_j = min(10^((target - I_j) / 20), 10^(max_gain_db / 20)) (flag 1 where the second binds).  If no block of
 *     0 .. j passes the gates, A_j = G_{j-1}, and 1 at j = 0 (flag 8: hold).
 *   Slew, for j > 0:  A_j is clamped to [fl(G_{j-1} s_dn), fl(G_{j-1} s_up)] (flag 4 where that moves it).  s_up =
 *     10^(max_slew_db / 20) and s_dn = 1 / s_up are formed on the host at smi_louds_open.  Knot 0 is not clamped.
 *   Peak.  P_j = max |x| over [(j - 1) hop, (j + 1) hop) intersected with [0, L): exact, a SAMPLE peak.  If fl(A_j P_j) > ceiling
 *     then G_j = ceiling / P_j (flag 2), else G_j = A_j.  This step is the last, so the ceiling always wins; after a capped
 *     knot the gain comes back at the slew rate.
 * Samples.  For j hop <= i < (j + 1) hop:
 *     g = G_j + fl(fl(G_{j+1} - G_j) * fl(fl64(i - j hop) / fl64(hop))),      out[i] = fl32(fl64(x[i]) * g).
 * g lies between two knots that are both at most ceiling / (the peak of that hop), so |out| <= ceiling up to the roundings.
 * End of the stream.  With K = floor((L - block) / hop), the last whole block: the stream has the knots 0 .. floor((L - 1) / hop)
 * + 1.  Those behind K hold the target gain A_j = G_K (flag 8); the slew step (relative to G_{j-1}) and the peak step, over
 * what exists of their hops, apply to them as to every knot.  1 <= L < block: smi_loud_rows' short-span rule (one block, the
 * whole stream, the absolute gate alone) gives the one loudness and the one A = min(10^((target - I) / 20), 10^(max_gain_db /
 * 20)) that all knots share (A = 1 and flag 8 where the gate fails); slew and peak steps as above.  L = 0: nothing.  A NaN
 * target measures only: every G = 1, every flag 0, and the output is the input bit for bit.
 *
 * Emission (smi_louds_piece_len, host integer arithmetic).  Hop j needs G_{j+1}, so it leaves once n >= (j + 5) hop: after a
 * push that is not the last a stream has emitted E(n) = hop * max(0, floor(n / hop) - 4) samples, after the last push L.  A
 * push emits the difference, which may be 0.  The delay is below 5 hops of audio: 500 ms.
 *
 * State.  On the host: n (the knots made and the samples emitted follow from it) and the stream's parameters.  On the device,
 * per stream and never copied back: the cascade's state at the last whole segment edge F = 128 floor(n / 128); the sum so far
 * of the hop that is open at F and the three hop sums before it; G of the last knot, its I, the OR of the flags and the peak so
 * far; every z_j so far (max_blocks bounds them: a push that would pass it is refused before anything changes); and the input
 * from max(0, min(E(n), F) - 2) to n -- what is not emitted yet, the tail short of a whole segment, and the two samples that
 * are the filter's input history at F -- at most max(5 hop, 128) + 2 samples.  Only whole segments change the carried state
 * before the last push: the tail behind F is filtered too, so that the hops that close inside it are known, and filtered again
 * from the same state by the push that completes its segment; a hop's sum is the same chain of additions either way, so the
 * order of every sum is a function of the absolute index alone.  State lives in two sets that a stream uses in turn (a push
 * reads one and writes the other), so one launch sequence serves a call whatever B; the z_j are written once each.
 *
 * Five launches a call, whatever B, no atomics: k_louds_seg, k_louds_carry, k_louds_energy -- smi_loud_rows' three filter
 * launches over the virtual sequence of held input followed by the chunk, from the stream's state --; k_louds_knots, one block
 * of 256 a row, which closes hops and blocks and walks the row's new knots in order; k_louds_apply, grid (tiles of 1024
 * samples of the pieces, rows), which writes the pieces and the next held input.
 *
 * Guarantees: the concatenation of a stream's pieces, its knot gains and its flags are, bit for bit, those of the same stream
 * pushed at once with last = 1 -- whatever the granularity of the pushes, empty ones included, the stream's slot, its row in
 * a call, the other rows, the strides and what lies outside len.  A stream is refused before n passes 2^28.  All pushes of a
 * handle must go to one HIP stream (or be ordered by the caller). */
typedef struct smi_louds smi_louds;
/* max_streams (1..4096) slots; max_chunk (1..2^24) samples a push; block: a multiple of 4; coef_host[10] as for smi_loud_rows;
 * max_blocks (1..2^26): the blocks a stream may reach.  Synchronous (one allocation, one clear). */
int smi_louds_create(int max_streams, int max_chunk, int block, const double* coef_host, int max_blocks, smi_louds** out);
int smi_louds_destroy(smi_louds* h);
/* A new stream in slot `stream`: n = 0.  target in LUFS (NaN: measure only), max_gain_db >= 0, ceiling > 0, max_slew_db >= 0
 * (dB a hop).  Host only.  A stream closes with its last push. */
int smi_louds_open(smi_louds* h, int stream, double target, double max_gain_db, double ceiling, double max_slew_db);
/* One chunk per row: in_dev [B][stride] f32 (row b valid for len_host[b], which may be 0), of the open streams stream_host[b],
 * each at most once in a call; last_host[b] = 1 on a stream's last push.  out_dev [B][out_stride] f32: row b receives its piece
 * and zeros from there to out_stride (>= 1 and >= the longest piece); it must not overlap in_dev.  gain_dev (may be null)
 * [B][gain_stride] float64 receives (G_j, flags) of the knots this push made final, in order, then zeros to gain_stride (>= 1
 * and >= two values a knot of the row with the most; smi_louds_piece_len counts them).  stats_dev (may be null) [B][4] float64
 * receives (I of the latest whole block -- after the last push the loudness of the whole stream --, the peak so far, the latest
 * G, the OR of all flags so far).  n_out_host [B] (may be null) receives the pieces' lengths, filled before the launch.
 * B <= 64.  Asynchronous on `stream`.  Every argument of every row is checked before anything changes or is launched: a bad one
 * returns SMI_EINVAL and names the argument in smi_last_error. */
int smi_louds_push_rows(smi_louds* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                        const int32_t* last_host, int B, double* gain_dev, long long gain_stride, float* out_dev, long long out_stride,
                        int32_t* n_out_host, double* stats_dev, void* stream);
/* The piece length of one push, pure host arithmetic: a stream that holds n_before samples takes len samples (last = 1: its
 * last push); n_after / knots_after (may be null) receive the samples and the knots made after it (before it the stream had
 * max(0, floor(n_before / hop) - 3) knots).  -1 for a bad argument. */
long long smi_louds_piece_len(int block, long long n_before, long long len, int last, long long* n_after, long long* knots_after);

/* ------------------------------------------------------------------------------------------
 * Limiter of joined streams: the section "Output limiter" above with state carried from push to push, so that a stream whose
 * input arrives in chunks leaves in pieces before it has ended.  No sample is defined here: the concatenation of a stream's
 * pieces is smi_limit_rows of its whole input x[0 .. L) as one span, with a null gain_dev (g = 1) and the stream's mode,
 * ceiling, A = lookahead, R = release, window and taps; after the last push the four stats are that call's stats.  All of it
 * bit for bit.  The limiter is feed-forward, so what is new is only the rule for when a sample is final, and the state.
 *
 * When a sample is final.  W = A + R.  out[i] reads s[i] and x[i]; s[i] reads m[i - A .. i + R] and r[i]; m[j] reads
 * r[j - R .. j + A]; r[j] reads e[j]; and e[j] reads x[j - 9 .. j + 10] (the taps d = -10 .. 9 of every phase; the sample-peak
 * mode reads x[j] alone).  So out[i] reads x[i - W - 9 .. i + W + 10] and nothing else.  With n samples so far, every i with
 * i + W + 10 <= n - 1 is final: nothing it reads lies at or beyond n, so nothing it reads can change, and none of it is the
 * zero or the r = 1 that the batch form reads beyond L -- those can never stand in for input that is still to come.
 *
 * Emission (smi_limits_piece_len, host integer arithmetic).  After a push that is not the last a stream has emitted
 * E(n) = max(0, n - (A + R + 10)) samples, after the last push L, the remaining samples formed as the batch forms them, with
 * zeros and r = 1 read beyond L.  A push emits the difference, which may be 0.  One rule serves both modes (the sample-peak
 * mode could leave 10 samples earlier; it does not), so a piece's length depends on n, A and R alone.  A piece leaves
 * A + R + 10 samples behind its input -- 450 samples, 28 ms, at the default reach at 16 kHz -- and never waits for another chunk.
 *
 * State.  On the host: n and the stream's mode and ceiling.  On the device, per stream and never copied back: the input from
 * max(0, E(n) - (A + R) - 9) to n -- the first sample that output E(n), the next to leave, reads -- which is at most
 * 2 (A + R) + 19 samples (919 at the default reach, 4627 at the largest); and the running stats: max e, min s and the count of
 * s < 1 over the samples emitted so far -- a max, a min and a sum of whole numbers, exact in any order.  r is not carried: a
 * push computes it anew over [max(0, E(n_before) - (A + R)), E(n_after) + A + R) from the held input followed by the chunk, by
 * the same expression, so it has the same bits.  State lives in two sets that a stream uses in turn (a push reads one and
 * writes the other), so one launch sequence serves a call whatever B.
 *
 * Stats, [4] float64 a row: (max e, 1, min s, the count of s < 1) over the samples [0, E) the stream has emitted after this
 * push: a function of n and the stream alone, not of how it was pushed.  Nothing emitted: (0, 1, 1, 0).
 *
 * Three launches a call, whatever B, no atomics; the window and the taps went to the device at smi_limits_create.  k_limits_env,
 * grid (tiles of 1024 samples of the range of r above, rows): k_limit_env over the virtual sequence of held input followed by
 * the chunk.  k_limits_apply, grid (tiles of 1024 samples of the pieces up to out_stride, rows): k_limit_apply's minimum by
 * doubling, smoothing sums, product and clamp; tile 0 of a row also writes the next held input.  k_limits_stats, one block a
 * row.  The three call the device functions that the batch kernels call.
 *
 * Guarantees: the concatenation of a stream's pieces and its final stats are, bit for bit, smi_limit_rows of the whole stream,
 * and |out| <= ceiling exactly -- whatever the granularity of the pushes, empty ones included, the stream's slot, its row in a
 * call, the other rows, the strides and what lies outside len.  A stream is refused before n passes 2^28.  All pushes of a
 * handle must go to one HIP stream (or be ordered by the caller). */
typedef struct smi_limits smi_limits;
/* max_streams (1..4096) slots; max_chunk (1..2^24) samples a push; lookahead, release, win_host [lookahead + release + 1],
 * taps_host [n_taps], n_taps (0: the handle serves the sample-peak mode only) and phases as for smi_limit_rows, with the same
 * ranges and the same check of the window's sum.  Synchronous (one allocation, one clear, two small copies). */
int smi_limits_create(int max_streams, int max_chunk, int lookahead, int release, const double* win_host, const double* taps_host, int n_taps,
                      int phases, smi_limits** out);
int smi_limits_destroy(smi_limits* h);
/* A new stream in slot `stream`: n = 0.  true_peak = 1: peaks of the oversampled signal (the handle's taps); 0: the sample
 * mode.  ceiling > 0.  Host only.  A stream closes with its last push. */
int smi_limits_open(smi_limits* h, int stream, int true_peak, double ceiling);
/* One chunk per row: in_dev [B][stride] f32 (row b valid for len_host[b], which may be 0), of the open streams stream_host[b],
 * each at most once in a call; last_host[b] = 1 on a stream's last push.  out_dev [B][out_stride] f32: row b receives its piece
 * and zeros from there to out_stride (>= 1 and >= the longest piece); it must not overlap in_dev.  stats_dev (may be null)
 * [B][4] float64 as above.  n_out_host [B] (may be null) receives the pieces' lengths, filled before the launch.  B <= 64.
 * Asynchronous on `stream`.  Every argument of every row is checked before anything changes or is launched: a bad one returns
 * SMI_EINVAL and names the argument in smi_last_error. */
int smi_limits_push_rows(smi_limits* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, float* out_dev, long long out_stride, int32_t* n_out_host, double* stats_dev,
                         void* stream);
/* The piece length of one push, pure host arithmetic: a stream with reach lookahead, release that holds n_before samples takes
 * len samples (last = 1: its last push); n_after (may be null) receives the samples after it.  -1 for a bad argument. */
long long smi_limits_piece_len(int lookahead, int release, long long n_before, long long len, int last, long long* n_after);

#ifdef __cplusplus
}
#endif
#endif /* SPARKMI_H */
