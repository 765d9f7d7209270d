/*
 * sparkmi_debug.h -- diagnostics and test entry points (the LLM half; the conv kernel forms of the vocoder / encoder; the prompt encoder's launch list).  NOT part of the product ABI: these symbols exist
 * only in libsparkmi_diag.so (spark-tts_amd/csrc built with -DSMI_DIAG), which also exports everything sparkmi.h declares and
 * -- unlike libsparkmi.so -- honours the SPARKMI_* environment switches listed in DESIGN.md 6.1.  Loaded by tools/, by
 * bench.py's per-kernel probes and by the tests that look inside a step (tests/test_llm_ops_gpu.py, test_engine_gpu.py).
 */
#ifndef SPARKMI_DEBUG_H
#define SPARKMI_DEBUG_H

#include "sparkmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-kernel timing probe used by bench.py: launches ONLY the named decode-step kernel of `layer`
 * `iters` times on `stream` (inputs are whatever the scratch holds), bracketed by HIP events, and
 * returns the average milliseconds per launch.  kernel: 0 qkv, 1 attn, 2 o_proj, 3 gate_up,
 * 4 down, 5 lm_head, 6 finalize, 7 = the whole decode step (graph or eager as configured), 8 = all layers of one step
 * (one launch of the one-row engine where it applies, else the layer kernels in order; needs a new prefill afterwards).
 * 16 + k (k = 0..4): layer kernel k timed in sequence -- (iters whole layers) minus (the same layers
 * without k) -- so that it finds the L2 state its producers leave, as inside the decode graph. */
int smi_llm_time_kernel(smi_llm* h, int kernel, int layer, int iters, float* ms_avg, void* stream);
/* Diagnostics: one launch of a decode-step GEMM kernel (ids as above, GEMM kernels only) with in-kernel
 * s_memrealtime phase stamps; out[0..7) = mean over blocks of (stamp i - earliest stamp 0) in microseconds,
 * out[7] = shader clock in MHz (tools/stamps.py).  kernel + 32: the layer's earlier kernels (and the previous layer's down_proj)
 * run first, un-stamped, so the stamped kernel finds the cache state it finds inside a decode step (tools/prefetch_stamps.py).
 * Needs a started generation. */
int smi_llm_debug_stamps(smi_llm* h, int kernel, int layer, double* out);
/* One-row decode engine (csrc/smi_eng.h).  With ONE live sequence in slot 0 (bf16 KV, contiguous cache, contexts up to
 * 1024 tokens) the layers of a decode step run as one persistent launch -- one workgroup per CU, weights streamed through
 * LDS rings by LDS-DMA, the five all-to-all edges of a layer handed over inside the launch -- instead of four dependent
 * launches per layer; the arithmetic (every product, accumulator chain and addition order) is the launch path's, so the
 * tokens are the same bits.  OPT-IN (SPARKMI_ENGINE=1 at create, or smi_llm_set_engine(h, 1), which builds it on first use:
 * 0.8 GB of re-packed weights): on MI355X at the 0.5B shape the five in-launch hand-offs of a layer cost more than the four
 * kernel boundaries they replace (26.3 vs 23.4 us per layer), so the launch path stays the default.
 *   smi_llm_engine: *enabled = 1 when one-row steps take the engine; info[4] = {CUs, images per wave and layer, LDS bytes,
 *                   built}; why = a one-line reason / description.
 *   smi_llm_set_engine: runtime switch between the engine and the launch path (A/B, tests); synchronises the device; on = 1
 *                   where the engine does not apply (f32 / paged KV, odd shapes, small device) leaves it off (see `why`).
 *   smi_llm_engine_plan: host-only check of the static work plan for `ncu` CUs (no GPU call): every weight image placed
 *                   exactly once, stream order = job order; stats[8] = {images per wave max, per wave and phase max, parts per
 *                   CU and phase max, jobs per wave max, images per CU min, max, LDS bytes, images per layer}.
 *   smi_llm_engine_stamps: diagnostics, SPARKMI_ENGINE_STAMPS=1: out[3][layers][16] microseconds of the last engine launch
 *                   (wave 0 of CU 0, wave 0 of the first head CU, wave 7 of CU 0; after the hand-offs h, q|k|v, attention, h_mid, act).
 * A hand-off that does not complete within SPARKMI_ENGINE_TIMEOUT_MS (default 500) ends the launch; the next call that
 * synchronises (smi_llm_get_tokens / _status / _all_done) returns SMI_EHIP. */
int smi_llm_engine(smi_llm* h, int32_t* enabled, int32_t* info, char* why, int n);
int smi_llm_set_engine(smi_llm* h, int on);
int smi_llm_engine_plan(const smi_llm_cfg* cfg, int ncu, int32_t* stats);
int smi_llm_engine_stamps(smi_llm* h, double* out, int cap);
/* Tests: synchronises and copies the residual row (hidden_size floats) of row 0 as the last step left it. */
int smi_llm_debug_hidden(smi_llm* h, float* out_host, int n);
/* Tests / debugging: synchronises and copies one scratch buffer as raw bytes (buffers 0..4 and 6 hold one entry per live row:
 * M rows after smi_llm_debug_layer).  what: 0 q [M][q_dim] f32, 1 / 2 / 3 the operand
 * triples of o_proj / down_proj / the next norm ([K / 32][3][4][M][16 B]), 4 the residual rows, 5 the engine's
 * granules [2][per buffer] u64 {tag << 32 | f32 bits}, 6 partial sums of squares [hidden / 4], 7 K rows of layer 0, slot 0,
 * kv head 0 (bf16), 8 h + o_proj of the fused one-row path, 9 the live rows' logits [rows][vocab] f32 as the last step's lm_head left
 * them (written only by a step that needs them: sampling, penalties, log-probabilities; a restricted lm_head writes the listed
 * tiles only).  16 .. 20: the prefill workspace after smi_llm_debug_prefill_layer, for
 * its M rows: 16 q [M][q_dim] f32, 17 / 18 / 19 the operand triples of o_proj / down_proj / the next norm (same layout, this M),
 * 20 the residual rows [M][hidden] f32.  cap must hold the buffer (M rows x 4864 x 6 B at the 0.5B shape: size it from M). */
int smi_llm_debug_read(smi_llm* h, int what, void* out_host, size_t cap, size_t* got);

/* Op-level tests of the LLM half: ONE decoder layer's kernels, stage by stage, on caller-given rows -- launched by the functions a
 * real step launches them with (same kernel choices per row count, launch geometry, prologue / epilogue fusions), so the classes
 * of transformers' modeling_qwen2.py can be checked one at a time (tests/test_llm_ops_gpu.py on tests/golden/llm_ops.npz):
 * Qwen2RMSNorm + q/k/v_proj + apply_rotary_pos_emb (MQ:247-252, 91-135), eager_attention_forward (MQ:150-173), o_proj + residual,
 * Qwen2MLP (MQ:46-48).
 *   smi_llm_debug_set_kv / _get_kv: write / read cache rows of (layer, slot) as fp32 [n][num_kv_heads][64] in transformers' dim
 *     order (keys rotated, as a cache holds them); the cache's own dtype and row order are converted on the host.
 *   smi_llm_debug_layer: rows_host = M (slot, pos) pairs, hidden_host [M][hidden] = the residual rows entering `layer`; runs its
 *     kernels up to and including `stage`: 0 QKV (+ bias, RoPE, K/V append: read q with smi_llm_debug_read(0), K/V with _get_kv),
 *     1 attention (buffer 1: the o_proj operand triples, head-interleaved k tiles), 2 o_proj + residual (buffer 4; one fused row:
 *     buffer 8), 3 gate_up + SwiGLU (buffer 2: act triples), 4 down_proj + residual (buffer 4).  smi_llm_debug_read's buffers
 *     0..4 and 6 then hold M rows.  Ends the current generation.
 *   Paged KV cache (kv_page_tokens > 0): _set_kv / _get_kv give the slot pages for positions 0 .. pos0 + n - 1 and copy page by page
 *     through the host's page table; _debug_layer / _debug_prefill_layer give every named slot pages up to its last row's position
 *     (SMI_ENOMEM when the pool is short; pages stay with the slot until the next prefill or release).  The order of those calls
 *     decides which pages a slot gets: tests/test_llm_paged_ops_gpu.py fills the slots a page at a time, round-robin.
 *   smi_llm_debug_page_table: the pages `slot` holds, in position order, from the host's page table: *n = their count (0 on a
 *     contiguous cache), the first min(*n, cap) of them in out. */
int smi_llm_debug_set_kv(smi_llm* h, int layer, int slot, int pos0, int n, const float* k_host, const float* v_host);
int smi_llm_debug_get_kv(smi_llm* h, int layer, int slot, int pos0, int n, float* k_host, float* v_host);
int smi_llm_debug_page_table(smi_llm* h, int slot, int32_t* out, int cap, int32_t* n);
int smi_llm_debug_layer(smi_llm* h, int layer, int M, const int32_t* rows_host, const float* hidden_host, int stage);
/* Op-level tests of the PROMPT pass (tests/test_llm_prefill_ops_gpu.py): one decoder layer's kernels as a pass over more than 64
 * prompt rows launches them -- k_pgemm in its few-row (split-K o_proj / down_proj + k_resid_comb) and many-row shapes, k_attn_pf<f32>,
 * k_attn_pf<bf16>, k_attn_pf2 on its 16-row tiles, or (family = SMI_PF_GROUPED) the row-grouped decode GEMMs -- through the per-layer
 * launch function every layer of a real pass goes through, on ONE row group in the prefill workspace.
 *   smi_llm_debug_prefill_layer: seq_host = n_seq (KV slot, first position, rows) triples, each sequence in its own slot; sequence
 *     b's rows are positions pos0 .. pos0 + n - 1 of its slot, in plan order.  pos0 > 0: the tail group of a prompt that straddles a
 *     4096-row group -- the caller fills positions 0 .. pos0 - 1 with smi_llm_debug_set_kv first.  hidden_host [M][hidden], M = the
 *     sum of the row counts (1 .. 4096): the residual rows entering `layer`.  Runs the layer's kernels up to and including `stage`:
 *     0 QKV (+ bias, RoPE, K/V append: smi_llm_debug_read(16), _get_kv), 1 attention (17), 2 o_proj + residual (20), 3 gate_up +
 *     SwiGLU (18), 4 down_proj + residual (20), 5 = stage 4, then layer + 1's QKV (16, _get_kv of layer + 1) -- the one reader of
 *     the RMSNorm partials down_proj leaves.  The last layer takes stage 0 only (a pass launches nothing after its K/V append): any
 *     other stage is SMI_EINVAL, as are M = 0 and a position outside the cache.  Ends the current generation.
 *   smi_llm_pf_tiles: host only, no GPU call -- the tiles the pass builds for k_attn_pf2 from M (slot, pos) rows: out[i] =
 *     (first row, rows, slot, first position) of tile i, *n = the number of tiles (at most cap are written). */
enum { SMI_PF_GROUPED = 1, SMI_PF_PGEMM = 2 };
int smi_llm_debug_prefill_layer(smi_llm* h, int layer, int stage, int n_seq, const int32_t* seq_host, const float* hidden_host, int family);
int smi_llm_pf_tiles(const int32_t* rows_host, int M, int32_t* out, int cap, int32_t* n);
/* Which kernel form each GEMM of a layer and the lm_head start with (tests/test_gemm_forms_cpu.py): host only, no
 * GPU call -- the pick functions the launch sites themselves call, on plain values.
 *   cfg, M: the model shape and the row count (a decode step: 1 .. 64; a prompt pass's row group: 1 .. 4096).
 *   layer_pos: first, middle or last layer (the last layer's down_proj has no next layer to prefetch for).
 *   flags: the switches a pick reads; -1 in a field = what smi_llm_create leaves there when no SPARKMI_* switch is set (fused:
 *     then 1 at one decode row of a shape that has the fused o_proj); null = every field so.
 *   out[5]: QKV, o_proj, gate_up, down_proj, lm_head.  kernel: the instantiation by name, template arguments as numbers in the
 *     kernel's own order ("k_gemm<1,1,16,2,1,1,2,0,1,1,2,16>"; a pair: "k_downC<10,1>+k_resid_comb<0,0>"), empty with launches = 0
 *     where nothing is launched (o_proj done by the attention kernel); grid (x, y) in blocks, block in threads and dynamic LDS
 *     bytes of the (first) kernel; grid2: blocks of 64 threads of the k_resid_comb of a pair; launches: kernels started (2 for a
 *     pair, one pass per 32 rows for the persistent lm_head above 16 rows). */
typedef struct smi_gemm_flags {
  int32_t pass;            /* 0: decode rows; SMI_PF_GROUPED / SMI_PF_PGEMM: a prompt pass's row group, every kernel in that family */
  int32_t fused;           /* decode: 1 = one row with the fused o_proj in effect, 2 = its 2 .. 8-row form (SPARKMI_FUSE2_ROWS), 0 = neither */
  int32_t stamps;          /* in-kernel phase stamps on (smi_llm_debug_stamps) */
  int32_t exact;           /* exact-weights mode (smi_llm_cfg.weights_exact) */
  int32_t tune2;           /* SPARKMI_TUNE2 bits */
  int32_t prefetch_mask, prefetch_rows;   /* helper-block prefetch: producer bits (1 QKV, 4 down_proj) and the row bound */
  int32_t kv_f32;          /* cache type (smi_llm_cfg.kv_dtype) */
  int32_t pg_split_rows;   /* SPARKMI_PG_SPLIT_ROWS */
  int32_t lm_restricted;   /* every row constrained: the restricted lm_head */
  int32_t lm_blocks;       /* blocks of the persistent lm_head */
  int32_t lm_screen;       /* one greedy row behind the int8 screen; -1 / 0: today's form */
} smi_gemm_flags;
typedef struct smi_gemm_form_info {
  char kernel[96];
  int32_t grid[2], block, launches, grid2;
  int64_t lds_bytes;
} smi_gemm_form_info;
enum { SMI_LAYER_FIRST = 0, SMI_LAYER_MIDDLE = 1, SMI_LAYER_LAST = 2 };
int smi_llm_gemm_forms(const smi_llm_cfg* cfg, int M, int layer_pos, const smi_gemm_flags* flags, smi_gemm_form_info* out);
/* Diagnostics: the raw stamp buffer (u64 s_memrealtime ticks, 10 ns) after smi_llm_debug_stamps; n entries. */
int smi_llm_debug_raw_stamps(smi_llm* h, unsigned long long* out, int n);
/* Tests: the sampler alone (k_sample_scan + k_sample, through launch_sampler, the one function a decode step too starts them
 * from) on a caller's logits row --
 * the reference's default decoding chain, cli/SparkTTS.py:166-168,197-204 -> transformers' TemperatureLogitsWarper ->
 * TopKLogitsWarper -> TopPLogitsWarper -> multinomial.  logits_host [vocab_size] is replicated to every row (null: the rows
 * of the previous call stay), n_rows rows draw one token each from the streams (seed; token index 0, sequence number = row),
 * tokens_out [n_rows].  use_bound = 1: the one-pass candidate collection with the top_k-th largest block maximum as the bound
 * (block j = the j-th contiguous share of the row, as many blocks as the lm_head launch of n_rows rows leaves); 0: the exact
 * radix selection.  Parameters come from smi_llm_set_sampling.  Synchronises; ends the current generation. */
int smi_llm_debug_sample(smi_llm* h, const float* logits_host, int n_rows, uint64_t seed, int use_bound, int32_t* tokens_out);
/* Tests: the penalty kernel alone (k_penalize, through the step's launch_penalize for n_rows rows, n_rows <= max_slots) on
 * caller rows:
 * logits_host [n_rows][vocab_size], hist_host [n_rows][vocab_size] history entries (bit 15: the id is in the prompt, bits 0..14:
 * its count among the generated tokens), pens [n_rows] records (smi_llm_admit_penalized's checks), emitted_host [n_rows]
 * tokens each row has emitted; eos ids: the last smi_llm_session_begin's.  logits_out [n_rows][vocab_size]: the processed rows;
 * argmax_out [n_rows]: the arg-max over the per-set maxima the kernel leaves for k_finalize.  Synchronises; ends the current
 * generation. */
int smi_llm_debug_penalize(smi_llm* h, const float* logits_host, int n_rows, const uint16_t* hist_host, const smi_penalty_params* pens,
                           const int32_t* emitted_host, float* logits_out, int32_t* argmax_out);
/* Tests: the log-probability kernels alone (k_logprob and k_finalize's combine, through the step's launch_logprob and
 * launch_finalize for n_rows rows, n_rows <= max_slots) on caller rows: logits_host [n_rows][vocab_size] (the processed logits z before temperature),
 * temperature_host [n_rows] (finite, > 0; each row is a sampling row with 1/T, T = 1: unscaled), tokens_host [n_rows] the
 * emitted ids.  The row maxima the kernel reads are left as the lm_head leaves them (per-set maxima over a contiguous
 * partition).  lp_out [n_rows]: z[tok] / T - logsumexp(z / T).  Synchronises; ends the current generation. */
int smi_llm_debug_logprob(smi_llm* h, const float* logits_host, int n_rows, const float* temperature_host, const int32_t* tokens_host,
                          float* lp_out);
/* Tests: the bias stage (stage 0b inside k_penalize) and k_finalize's stop match alone, through the step's launch_penalize
 * and launch_finalize for n_rows rows (n_rows <= max_slots), on caller rows: logits_host [n_rows][vocab_size]; seq [n_rows] records (smi_llm_admit_biased's
 * checks, without an allowed set); ctx_host [n_rows][ctx_cap] int64: row m's context ctx_len_host[m] ids long, of which the
 * first prompt_len_host[m] (>= 1) are its prompt and the rest the tokens it has generated; min_new_host [n_rows] (null: 0)
 * the rows' min_new_tokens for the stop match; eos ids: the last smi_llm_session_begin's.  The row maxima the kernels read
 * are left as the lm_head leaves them (per-set maxima over a contiguous partition).  logits_out [n_rows][vocab_size]: the
 * rows after the stage; token_out [n_rows]: the arg-max k_finalize emits; finished_out [n_rows]: the flag it leaves (an eos
 * id, or a stop sequence met by the generated tokens with the new one).  Synchronises; ends the current generation. */
int smi_llm_debug_seqbias(smi_llm* h, const float* logits_host, int n_rows, const smi_seq_params* seq, const int64_t* ctx_host,
                          const int32_t* ctx_len_host, const int32_t* prompt_len_host, int ctx_cap, const int32_t* min_new_host,
                          float* logits_out, int32_t* token_out, int32_t* finished_out);
/* Tests: the n-gram ban (k_ngram_ban), k_penalize and k_finalize alone, through the step's launch_ngram_ban, launch_penalize
 * and launch_finalize for n_rows rows (n_rows <= max_slots), on caller rows: logits_host [n_rows][vocab_size]; ngram_host [n_rows] each row's
 * no_repeat_ngram_size (0 .. SMI_MAX_NGRAM); ctx_host [n_rows][ctx_cap] int64: row m's context ctx_len_host[m] ids long, of
 * which the first prompt_len_host[m] (0 .. ctx_len, at most max_positions) go to the slot's prompt store and the rest to the
 * token history.  logits_out [n_rows][vocab_size]: the rows after the stage; token_out [n_rows]: the arg-max k_finalize
 * emits (lowest id on ties).  Synchronises; ends the current generation. */
int smi_llm_debug_ngram(smi_llm* h, const float* logits_host, int n_rows, const int32_t* ngram_host, const int64_t* ctx_host,
                        const int32_t* ctx_len_host, const int32_t* prompt_len_host, int ctx_cap, float* logits_out, int32_t* token_out);
/* Op-level tests of the HEAD of a decode step (tests/test_head_ops_gpu.py): the final RMSNorm, the lm_head and
 * the token pick -- launch_one(KLM) then launch_one(KFIN), the two calls a step ends with -- alone on caller rows.  Rows 0 .. M - 1
 * sit in slots 0 .. M - 1 (M <= max_slots) at position 0 with no token emitted; every record is clean except what follows.
 *   hidden [M][hidden]: the residual rows leaving the last layer.  k_load_hidden leaves them, their operand triples under the
 *     FINAL norm's weight and their sums of squares where the last down_proj leaves them.
 *   allow [M] or null: smi_llm_admit_constrained's records (its checks apply).  When every row's record is not neutral the
 *     tile list is built by the function an admission builds it with, and the restricted lm_head runs.
 *   reads [M] or null: 1 = the row reads its logits -- a neutral sampling record (top_k = 1, T = 1, top_p = 1) is installed in
 *     its slot, so the step's feature mask has the sampling bit and the lm_head stores the logits rows in the handle's own
 *     buffer, as in a real step (no logits pointer is passed to launch_one).  With SMI_HEAD_FIN such a row's token is the
 *     sampler's: the arg-max, or ANY id that ties with it (TopKLogitsWarper keeps ties).
 *   flags: SMI_HEAD_FIN also runs launch_one(KFIN); SMI_HEAD_POISON fills the handle's logits buffer with quiet NaNs first;
 *     SMI_HEAD_SCREEN asks for the screened lm_head at any vocabulary size: it runs where a step's would -- one
 *     row that does not read its logits, no constraint, bf16 weights, at most 32 k tiles -- and `form` says whether it did.
 * Outputs, each nullable: logits_lm / logits_fin [M][vocab_size] = the handle's logits rows after KLM / after KFIN (whatever
 * the buffer holds where nothing was stored); pval / pidx [M][nblk] as the lm_head left them (pcap = entries each holds;
 * fewer than M * nblk: SMI_EINVAL); tokens [M] (SMI_HEAD_FIN).  nblk = the partial columns k_finalize reads (lm_blocks_for);
 * form / grid / block / launches: the kernel form the lm_head launch site named, its grid (x, y) and block size, and how many
 * launches of it the call made (a pass per 32 rows).  After SMI_HEAD_FIN smi_llm_debug_read's buffers 4, 3 and 6 hold the next
 * step's residual rows, first-norm operand triples and sums-of-squares partials of the M rows.  Synchronises; ends the
 * current generation. */
enum { SMI_HEAD_FIN = 1, SMI_HEAD_POISON = 2, SMI_HEAD_SCREEN = 4 };
typedef struct smi_head_io {
  const float* hidden;
  const smi_allow_params* allow;
  const int32_t* reads;
  int32_t flags;
  int32_t pcap;
  float* logits_lm;
  float* logits_fin;
  float* pval;
  int32_t* pidx;
  int32_t* tokens;
  int32_t nblk, launches, grid[2], block;   /* out */
  char form[32];                            /* out */
} smi_head_io;
int smi_llm_debug_head(smi_llm* h, int M, smi_head_io* io);
/* The screened lm_head's last candidate list and its selection log: tiles[0 .. min(*n_tiles, cap)) = the vocabulary
 * tiles the last k_lm_select listed, ascending, *n_tiles their count; counts[0 .. min(*n_counts, ccap)) = the list lengths of the
 * last selections, oldest first (at most 4096 are kept), *n_counts how many there are.  reset != 0 empties the log afterwards.
 * Either array may be null with its cap 0.  Synchronises.  SMI_EINVAL on a handle without the int8 copy. */
int smi_llm_debug_lm_screen(smi_llm* h, int32_t* tiles, int cap, int32_t* n_tiles, int32_t* counts, int ccap, int32_t* n_counts, int reset);

/* ------------------------------------------------------------------------------------------
 * Conv kernel forms (csrc/smi_net.h): which instantiation of k_conv / k_convb / k_convbT / k_conv_c1 / k_gemv1 the launch
 * builder picks for a layer and a call shape, and one conv on caller tensors run through exactly that choice
 * (tests/test_conv_forms_cpu.py, tests/test_conv_forms_gpu.py).
 * ---------------------------------------------------------------------------------------- */
enum { SMI_CONV_K_CONV = 0, SMI_CONV_K_CONVB = 1, SMI_CONV_K_CONVBT = 2, SMI_CONV_K_C1 = 3, SMI_CONV_K_GEMV = 4 };
typedef struct smi_conv_form {
  int32_t kernel;      /* SMI_CONV_K_* */
  int32_t qb;          /* 32-column time sub-tiles per wave */
  int32_t ks;          /* the waves split the input channels of one output tile */
  int32_t chg;         /* a staged chunk holds 32 * chg input channels */
  int32_t nc;          /* the staged row is up to 64 * nc columns wide */
  int32_t nwv;         /* waves per block */
  int32_t wpf, wall;   /* small-grid forms: weights one chunk ahead / all taps' weights together */
  int32_t tph;         /* k_convbT: output phases per block; k_conv_c1: taps */
} smi_conv_form;
/* the table run_launch dispatches from: smi_conv_form_count() entries, index -> record */
int smi_conv_form_count(void);
int smi_conv_form_get(int index, smi_conv_form* out);

/* One conv layer and one call shape.  Conv1d: S = 1, out[q] = sum W[co][ci][j] x[ci][q * istr + j * dil - pad] with either
 * istr = 1 and 2 * pad = dil * (K - 1) (length-preserving, as every stride-1 layer of the models), or istr > 1 and pad = 0 (the
 * feature encoder's strided convs: L_out = (L - K) / istr + 1, exact pipe only -- k_convb stages with unit stride).
 * ConvTranspose1d: S > 1, pad = (K - S) / 2, L_out = L * S.  L is the longest row's INPUT length and the row stride of X;
 * Y / Ys / R are [B][Cout][L_out].  gemv = 1: the per-utterance vector projection (k_gemv1; K = 1, L = 1, X [B][Cin],
 * Y [B][Cout], act none / ReLU (3) / sigmoid (4)); c1 = 1: the one-output-channel 7-tap conv (k_conv_c1) -- the two forms the
 * callers of make_conv select themselves.  plan_frames > 0: the plan is that of ONE row of plan_frames input positions in a
 * call whose longest row has plan_ext_frames = L (PlanShape).  act: 0 none, 1 GELU, 2 tanh, 3 ReLU. */
typedef struct smi_conv_case {
  int32_t Cout, Cin, K, dil, S, pad, istr, act;
  int32_t bf;          /* 1: bf16-split pipe (weights packed with pack_conv_b), 0: exact fp32 (pack_conv) */
  int32_t B, L;
  int32_t has_R;       /* a residual operand enters the plan (it keeps a transposed conv off k_convbT) */
  int32_t plan_frames, plan_ext_frames;
  int32_t gemv, c1;
} smi_conv_case;
typedef struct smi_conv_plan_info {
  smi_conv_form form;
  int32_t form_index;  /* its index in the table */
  int32_t xw;          /* staged row width */
  int32_t grid[3];
  int32_t lout;        /* output positions per row (all phases) */
  int64_t lds_bytes;
  int64_t plan_blocks; /* blocks of the grid the plan was chosen for */
} smi_conv_plan_info;
/* what make_conv builds for the case: host only, no GPU call */
int smi_conv_plan(const smi_conv_case* c, smi_conv_plan_info* out);
/* device operands of smi_conv_run; null = absent.  R may alias Y.  bbias [B][Cout]; bias / gamma / beta / alpha [Cout] */
typedef struct smi_conv_operands {
  const float* W;
  const float* X;
  const float* X2;
  const float* bias;
  const float* bbias;
  const float* gamma;
  const float* beta;
  const float* R;
  const float* alpha;
  float* Y;
  float* Ys;
  float out_scale;     /* 1 or 3 */
  int32_t reserved;
} smi_conv_operands;
/* Builds the launch with make_conv, applies the staging limits the vocoder and the encoder apply to their launch lists, runs
 * it, synchronises and reports the plan.  lens_host [B] valid INPUT lengths (null: all L); a strided conv's valid output
 * lengths are derived from them.  X must be readable for at least Cout floats (absent epilogue operands read it). */
int smi_conv_run(const smi_conv_case* c, const smi_conv_operands* io, const int32_t* lens_host, smi_conv_plan_info* plan, void* stream);
/* The launches smi_voc_block_run would build for (cfg, B, L), without running: kind 0 a conv (form), 1 k_dwln (cpt = the
 * instantiated channels per thread), 5 k_resunit (res_nwv waves).  *n = launches (at most cap are written). */
typedef struct smi_block_launch_info {
  char name[64];
  int32_t kind, form_index, res_nwv, cpt;
  smi_conv_form form;
} smi_block_launch_info;
int smi_voc_block_plan(const smi_voc_block_cfg* cfg, int B, int L, smi_block_launch_info* out, int cap, int32_t* n);

/* ------------------------------------------------------------------------------------------
 * Prompt encoder (csrc/smi_enc.hip): its OWN launch list, one launch at a time, on caller-written buffers -- the grid, block,
 * dynamic LDS size and arguments are those of a real encode of the same (n_samples, n_ref), because the list is the one
 * smi_enc_forward's graph path builds (tests/test_enc_ops_gpu.py).
 *   smi_enc_debug_build: builds the launch list on the handle-owned in_wav / in_ref / out_sem / out_glob buffers, uploads the
 *     row's lengths and runs nothing.  smi_enc_forward's argument checks apply (SMI_EINVAL before any GPU call).  The captured
 *     graphs of the handle are left alone.  *n_frames = wav2vec2 frames, *n_launches = launches of the list.
 *   smi_enc_debug_launch: launch `index` of the list: name (at most cap bytes) and info[8] = {kind (0 conv, 1 k_dwln,
 *     9 one of the encoder's small kernels), grid x, y, z, threads per block, dynamic LDS bytes, k_dwln's instantiated channels
 *     per thread (kind 1, else 0), 0}.
 *   smi_enc_debug_io: synchronous copy between host_ptr and `floats` 4-byte words at offset_floats of a named handle buffer
 *     (write = 1: host -> buffer).  Names: wavn cf0 cf1 h x wide att acc feat e0 e1 e2 ew frames dft mag mel ec_a ec_b ec_c
 *     ec_cat ec_lat ec_vec pctx pq pkv po pff pg pout fsqb in_wav in_ref out_sem (int64 ids: two words each) out_glob (int32).
 *     A range outside the buffer is SMI_EINVAL.
 *   smi_enc_debug_run: launches first .. last of the list, ONCE each and in order, then synchronises; the first error.
 *     (smi_enc_time_launch runs a launch iters + 1 times: wrong for the in-place launches.)
 * ---------------------------------------------------------------------------------------- */
int smi_enc_debug_build(smi_enc* h, int n_samples, int n_ref, int* n_frames, int* n_launches, void* stream);
int smi_enc_debug_launch(smi_enc* h, int index, char* name, int cap, int32_t* info);
int smi_enc_debug_io(smi_enc* h, const char* buffer_name, int write, void* host_ptr, size_t offset_floats, size_t floats);
int smi_enc_debug_run(smi_enc* h, int first, int last, void* stream);

/* The rows list (smi_enc_forward_rows) the same way; smi_enc_rows_reserve first.
 *   smi_enc_rows_debug_build: builds the list of B rows of (n_samples[b], n_ref[b]) on the workspace's own in_wav / in_ref /
 *     out_sem / out_glob buffers (row b's in its slab), uploads the length arrays and runs nothing.  smi_enc_forward_rows'
 *     argument checks apply.  n_frames[B]; *n_runs runs, run_start[i] (at most run_cap written) = first row of run i.
 *   smi_enc_rows_debug_runs: the same run table of the list the last build or the last smi_enc_forward_rows left.
 *   smi_enc_rows_debug_launch: as smi_enc_debug_launch; grid z is the number of rows of the launch's run (times the phases of a conv).
 *   smi_enc_rows_debug_io: as smi_enc_debug_io on row `row`'s copy of the named buffer (any reserved row, used or not); a copy
 *     that leaves the buffer's per-row size is SMI_EINVAL.  Inside a run a [C][T] buffer's row stride is the run's longest row.
 *   smi_enc_rows_debug_run: launches first .. last of the rows list, once each and in order, then synchronises.
 *   smi_enc_rows_debug_stage: smi_enc_debug_stage for row `row` of the last smi_enc_forward_rows. */
int smi_enc_rows_debug_build(smi_enc* h, const int32_t* n_samples, const int32_t* n_ref, int B, int32_t* n_frames, int* n_launches,
                             int32_t* run_start, int run_cap, int* n_runs, void* stream);
int smi_enc_rows_debug_runs(smi_enc* h, int32_t* run_start, int run_cap, int* n_runs, int* n_launches);
int smi_enc_rows_debug_launch(smi_enc* h, int index, char* name, int cap, int32_t* info);
int smi_enc_rows_debug_io(smi_enc* h, int row, const char* buffer_name, int write, void* host_ptr, size_t offset_floats, size_t floats);
int smi_enc_rows_debug_run(smi_enc* h, int first, int last, void* stream);
int smi_enc_rows_debug_stage(smi_enc* h, int row, const char* name, float* out_dev, size_t max_floats, int32_t* dims, void* stream);

/* Device memory the library's handles and entry points hold in this process right now (every allocation has one owner,
 * csrc/smi_common.h: DevBuf): *live_buffers allocations of *live_bytes bytes in all, pinned host staging included.  Either
 * pointer may be null.  Both return to their earlier values when a handle is destroyed (tests/test_dev_owner_gpu.py). */
int smi_debug_dev_memory(long long* live_buffers, long long* live_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SPARKMI_DEBUG_H */
