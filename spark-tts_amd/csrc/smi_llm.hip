// smi_llm.hip -- Qwen2 speech-token generator for gfx950 (MI355X).
//
// Stands behind AutoModelForCausalLM.generate(..., do_sample=False) as called at
// cli/SparkTTS.py:197-204 of the reference; the arithmetic restated is transformers'
// modeling_qwen2.py (RMSNorm :247-252, attention :150-235, RoPE :91-135, MLP :46-48).
//
// One "step" pushes M <= 32 rows through the model.  A row is (sequence slot, position, token):
// in decode the rows are the B live sequences, in prefill they are 32 prompt tokens.  Every row is
// independent in every kernel, so a batched step is bit-identical to B single-sequence steps.
//
// Kernels per layer (HBM-bound weight streaming; weights read exactly once per step):
//   k_gemm<QKV>   RMSNorm prologue -> [q|k|v] projection -> +bias -> RoPE -> q buffer / KV-cache append
//   k_attn        GQA attention over the cached keys (online softmax, wave64 shuffles + LDS combine)
//   k_gemm<RESID> o_proj, residual add in the epilogue
//   k_gemm<SWIGLU> RMSNorm prologue -> [gate|up] (row-interleaved) -> silu(g)*u
//   k_gemm<RESID> down_proj, residual add
// then k_gemm<LM> (final RMSNorm -> tied lm_head -> per-block argmax) and k_finalize (argmax over
// blocks, token/position bookkeeping, next step's embedding gather).
//
// The GEMM core: weights are bf16 in 16x32 tiles stored in MFMA A-operand order (one 1 KiB tile =
// one coalesced 16-B-per-lane wave load = one v_mfma_f32_16x16x32_bf16 operand).  Activations stay
// fp32-exact: every GEMM operand is kept in HBM/L2 as three bf16 terms (hi+mid+lo, 8+8+8 mantissa
// bits) in B-operand order, written by the epilogue of the kernel that produced the value (with the
// next RMSNorm's weight folded in and the row's partial sums of squares beside it), so consumers
// only stream.  Every product is exact and only the fp32 summation order differs from the CPU
// oracle.  MFMA columns are the rows m of the step.
#include "smi_common.h"
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace {

constexpr int kMaxRows = SMI_MAX_ROWS;
constexpr int kHeadDim = 64;

struct RowDesc {  // 16 bytes, lives in device memory
  int32_t slot, pos, token, flags;
};

// One sequence's token selection (smi_sample_params as admitted, 32 bytes); all zero = SMI_SAMPLING_INHERIT.
struct SampRec {
  int32_t mode;                   // SMI_SAMPLING_*
  int32_t top_k;                  // SAMPLE: 1..min(256, vocab)
  float inv_temp, top_p;
  unsigned long long seed;
  int32_t has_seed, pad;          // has_seed: the stream is keyed by (seed; token index) alone
};

// One sequence's logits penalties (smi_penalty_params as admitted, 24 bytes); on = 0 (all zero): not penalised.
struct PenRec {
  float rep, pres, freq;          // repetition / presence / frequency penalty
  int32_t min_new;                // eos ids are -inf while fewer tokens than this have been emitted
  int32_t prompt;                 // the prompt ids count for the repetition penalty
  int32_t on;                     // the record is not neutral: k_penalize processes the row, k_finalize counts its tokens
};

// One sequence's allowed-token set (smi_allow_params as admitted, 136 bytes): the union of [lo[i], hi[i]), i < n, sorted and
// disjoint; n = 0: not constrained (a neutral record is stored as n = 0).
struct AllowRec {
  int32_t n, pad;
  int32_t lo[SMI_MAX_ALLOW_RANGES], hi[SMI_MAX_ALLOW_RANGES];
};

// Generation controls in device memory (written at prefill / session_begin / admit; read by k_finalize and the sampler),
// so that nothing of them is baked into the captured decode graph: the graph survives from one utterance to the next.
struct Ctl {
  long long eos[SMI_MAX_EOS];     // a sequence stops counting after emitting any of the first n_eos ids
  int32_t n_eos, pad;
  unsigned long long seed;        // sampler stream key
  int32_t seqid[SMI_MAX_ROWS];    // per KV slot: admission number of the sequence living there (sampler stream key)
  SampRec samp[SMI_MAX_ROWS];     // per KV slot: the sequence's sampling record (smi_llm_admit_sampled)
  PenRec pen[SMI_MAX_ROWS];       // per KV slot: the sequence's penalty record (smi_llm_admit_penalized)
  int32_t lp[SMI_MAX_ROWS];       // per KV slot: 1 = the sequence returns per-token log-probabilities (smi_llm_admit_logprobs)
  AllowRec allow[SMI_MAX_ROWS];   // per KV slot: the sequence's allowed-token ranges (smi_llm_admit_constrained; n = 0: none)
  int32_t ngram[SMI_MAX_ROWS];    // per KV slot: the sequence's no_repeat_ngram_size (smi_llm_admit_ngram; 0: none)
  int32_t ngplen[SMI_MAX_ROWS];   // per KV slot: prompt ids held in the slot's row of the context store (ngram > 0 only)
};

// One sequence's bias entries and stop sequences (smi_seq_params as admitted) with the tail of its prompt, 1616 bytes; all zero:
// none.  The records live in an array of their own beside Ctl (smi_llm::seq, one per KV slot): a kernel gets the array only in a
// step whose graph key says that some live row has an entry, and an admission uploads only the records that change, so a
// session without records neither reads nor copies them.
struct SeqRec {
  int32_t n_bias, n_stop;
  int32_t plen;                         // prompt length (the prompt counts as context for the bias entries)
  int32_t n_ptail;                      // min(plen, SMI_MAX_SEQ_LEN - 1) prompt ids kept in ptail
  int32_t ptail[SMI_MAX_SEQ_LEN];       // ptail[SMI_MAX_SEQ_LEN - 1 - q] = the prompt's q-th id from its end, q = 1 .. n_ptail
  int32_t blen[SMI_MAX_BIAS_SEQS];
  float bias[SMI_MAX_BIAS_SEQS];
  int32_t bids[SMI_MAX_BIAS_SEQS][SMI_MAX_SEQ_LEN];
  int32_t slen[SMI_MAX_STOP_SEQS];
  int32_t sids[SMI_MAX_STOP_SEQS][SMI_MAX_SEQ_LEN];
};

// stage 0: the id lies in one of the record's ranges
__device__ __forceinline__ bool allow_has(const AllowRec* a, int id) {
  const int n = a->n;
  bool in = false;
  for (int r = 0; r < n; ++r) in |= id >= a->lo[r] && id < a->hi[r];
  return in;
}

struct KvMap {
  const int32_t* ptab;   // [slots][ppslot] page ids, or null
  int pshift, ppslot;
};

enum { PRO_PLAIN = 0, PRO_NORM = 1, PRO_FUSEDO = 2 };   // FUSEDO: RMSNorm operand built in the kernel from the fused o_proj's per-head partials
enum { EPI_RESID = 0, EPI_SWIGLU = 1, EPI_QKV = 2, EPI_LM = 3 };

// Same-XCD L2 prefetch for a LATER kernel: block b of every kernel of a graph lands on XCD (s + b) mod 8
// (measured: strict round-robin with the same start for every kernel, tools/xccmap.py), so a helper
// block with blockIdx == c (mod 8) warms exactly the weight slices that consumer blocks == c (mod 8)
// will read: those then hit the XCD's own 4 MiB L2 (a 17 MB stream: 5 us cold, 2 us L2-warm).  Speed
// only -- nothing depends on the placement.
struct PfDesc {
  const unsigned char* base;   // consumer weight matrix
  int slice_bytes;             // bytes consumer block b reads: [b * slice_bytes, (b + 1) * slice_bytes)
  int nslices;                 // consumer work blocks
  int q0, q1;                  // this producer covers slices s with q0 <= s / 8 < q1
};

__device__ __forceinline__ void pf_run(const PfDesc& d, int helper, int nhelpers, int tid, int nthreads) {
  const int c = (int)blockIdx.x & 7, r = helper >> 3, R = (nhelpers + 7) >> 3;
  for (int q = d.q0 + r; q < d.q1; q += R) {
    const int sl = q * 8 + c;
    if (sl < d.nslices) smi_prefetch_range(d.base + (size_t)sl * d.slice_bytes, (size_t)d.slice_bytes, tid, nthreads);
  }
}

struct GemmP {
  const uint4* W;        // [NT][KT][64] 16-byte lane pieces (bf16 tiles in MFMA A-operand order)
  int NT, KT, M;         // n tiles, k tiles, rows
  const RowDesc* rows;
  const unsigned char* XS;   // operand: exact bf16 triples [KT][3][4][M][16 B] in MFMA B-operand order
  const float* sspart;   // PRO_NORM: [rows][npart] partial sums of squares of the operand's fp32 source row
  int npart;
  float eps;
  float* Y;              // RESID: h [M][N]; QKV: q [M][q_dim]; LM: logits [M][V] or null
  const float* bias;     // QKV bias [N] (arena order)
  const float2* rope;    // [max_pos][32] (cos, sin)
  void* kcache;          // this layer's K cache: [slot][kvh][max_pos][64]
  void* vcache;
  int q_dim, kv_dim, n_kv, max_pos;
  KvMap km;              // QKV: paged KV cache (ptab null: contiguous slots)
  int V;                 // LM: true vocab size
  float* pval;           // LM: [rows][work_blocks] per-block best logit
  int* pidx;
  // producer side: the next consumer's operand, written by the epilogue
  unsigned char* XSout;  // RESID: triples of gamma_next * h_new, [N/32][3][4][M][16]; SWIGLU: triples of act
  const float* gamma_next;  // RESID: [N] RMSNorm weight of the NEXT norm
  float* ssout;          // RESID: [rows][NT * 4] partial sums of squares of h_new, one per 4 columns (k_pgemm: [rows][NT])
  unsigned long long* stamps;
  int work_blocks;       // blocks >= work_blocks are prefetch helpers (pf)
  PfDesc pf;
  int ldsb;              // few rows: bytes of wave-private LDS for the activation triples (0 = read them from global per tile)
  int lt_shift;          // log2(lanes that fetch one k tile's 12*M pieces)
  // fused o_proj (one row): PRO_FUSEDO builds its operand from these instead of reading XS / sspart; RESID reads its residual from Yin
  const float* part_o;   // [n_oheads][K] per-head partials of the o_proj (k_attn<.., FUSE>)
  int n_oheads;
  const float* hres;     // [K] residual stream before the attention block's contribution
  const float* gam;      // [K] this RMSNorm's weight
  float* h2out;          // [K] block 0 leaves h + o_proj here (the residual down_proj adds to)
  const float* Yin;      // RESID: residual row source when it is not Y itself (null: Y)
  const unsigned char* pf2_base; int pf2_slice, pf2_nslices;   // PRO_FUSEDO: a later kernel's weights the work blocks touch (null: none)
  int wperm;             // weight tiles stored row-part-major [q:4][k8:4][r:4][8] (W_down): lane (k8, n = 4q + r) owns piece q*16 + k8*4 + r
  // k_pgemm<RESID>: the K range is summed in SEGMENTS of kseg k tiles (segment sums added in order) -- the association both the
  // in-block form (many rows: a second accumulator set) and the split-K form (few rows: one block per segment -> `slab`
  // [segment][n tile][m tile][lane] f32x4, combined in order by k_resid_comb) produce, so a prompt row has the same bits in
  // either.  kseg = 0: one running sum over all of K (the other GEMMs).
  int kseg;
  float4* slab;
  int slab_mt;           // m-tiles of the whole launch (slab indexing)
  // restricted lm_head (k_lm / k_lm32 with RT = 1): the vocabulary tiles come through tlist = {count, tile indices ascending}, and
  // the epilogue masks the ids outside each row's own ranges (ctl->allow of the row's slot)
  const int* tlist;
  const Ctl* ctl;
};
// piece index of `lane` inside a 1 KiB weight tile (see GemmP::wperm)
__device__ __forceinline__ int smi_wlane(int lane, int wperm) {
  return wperm ? ((lane & 12) << 2) + ((lane >> 4) << 2) + (lane & 3) : lane;
}
constexpr int kMaxOHeads = 16;

// One weight tile piece (16 B per lane) of a once-read decode weight stream: non-temporal policy (MI355X_MICROARCH.md, row
// nt-weights).  Measured as separate builds on one box: decode step 627.9 -> 625.3 us at one row (two alternating pairs);
// -DSMI_W_PLAIN builds the plain-load variant for A/B (make variant NAME=plain VARFLAGS=-DSMI_W_PLAIN).
__device__ __forceinline__ uint4 smi_ldw(const uint4* q) {
#ifndef SMI_W_PLAIN
  typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
  const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)q);
  return make_uint4(v.x, v.y, v.z, v.w);
#else
  return *q;
#endif
}

// exact 3-way bf16 split: x == hi + mid + lo (8 + 8 + 8 mantissa bits)
__device__ __forceinline__ void split3(float x, uint32_t& hi, uint32_t& mi, uint32_t& lo) {
  hi = smi_f32_to_bf16(x);
  const float r1 = x - smi_bf16_to_f32(hi);
  mi = smi_f32_to_bf16(r1);
  const float r2 = r1 - smi_bf16_to_f32(mi);
  lo = smi_f32_to_bf16(r2);
}
// byte offset of the 16-byte piece (k tile kt, split s, octet k8, row m) in a triples buffer
__device__ __forceinline__ size_t xs_off(int kt, int s, int k8, int m, int M) {
  return ((size_t)((kt * 3 + s) * 4 + k8) * M + m) * 16;
}
// Where token `pos` of (slot, kv head) lives in a layer's K (or V) cache, in rows of 64 elements.  Contiguous slots:
// [slot][kvh][max_pos]; paged (ptab != null): the cache is a pool of pages [page][kvh][1 << pshift] and a slot's
// positions map to pages through its row of the page table (smi_llm_cfg.kv_page_tokens / kv_pages).
__device__ __forceinline__ size_t kv_row(const KvMap& km, int slot, int kvh, int n_kv, int max_pos, int pos) {
  if (km.ptab) {
    const int pg = km.ptab[(size_t)slot * km.ppslot + (pos >> km.pshift)];
    return (((size_t)pg * n_kv + kvh) << km.pshift) + (size_t)(pos & ((1 << km.pshift) - 1));
  }
  return ((size_t)slot * n_kv + kvh) * max_pos + pos;
}

// o_proj's reduction index is stored head-interleaved: k tile (half * n_heads + head) holds dims 32 * half .. + 31 of
// `head` (W_o's columns in the arena and the attention output operand alike).  With the k tile -> wave map
// kt mod n_heads of the o_proj kernel, wave w then sums exactly head w's two tiles: the per-head partial that the
// one-row attention kernel can also produce itself (fused o_proj, below) -- same bits either way.
__device__ __forceinline__ int o_ktile(int head, int d, int n_heads) { return (d >> 5) * n_heads + head; }

// ------------------------------------------------------------------------------------------
// GEMM: Y[m][n] = sum_k W[n][k] * X[m][k], X given as exact bf16 triples in global memory.
// MT m-tiles of 16 rows, NTB 16-row weight tiles per block, NW waves split K (k tile kt belongs to
// wave kt mod NW), U tiles per wave in flight per batch.  One accumulator chain per split term,
// summed (lo + mid) + hi; cross-wave reduction in fixed order.  Nothing depends on M, so a row's
// result is bit-identical whatever else is in the batch.  PRO_NORM: the operand is gamma * x and the
// RMSNorm factor rsqrt(mean(x^2) + eps) -- a per-row scalar -- is applied to the accumulator.
// ------------------------------------------------------------------------------------------
// H > 1 (RESID only): the 16 rows of a weight tile are split over H blocks (8 or 4 rows each: only those
// lanes load, the others feed zeros to the MFMA), so a matrix with few n tiles (N = 896: 56) still
// spreads its HBM stream over 112 / 224 CUs.  Every output element keeps its own summation order.
// LEAN: the few-row decode instantiation (M <= 5, operands staged through wave-private LDS, no phase stamps): the paths it
// never takes are compiled out -- these kernels are bound by instruction issue as much as by memory.
// Sum of a row's RMSNorm partials for one lane (index order lane, lane + 64, ...; the caller adds the lanes with
// smi_wave_sum).  Four loads are issued together from clamped addresses and masked by value: written as a plain loop
// the compiler emits load -> wait -> add per trip, i.e. one L2 round trip per 64 partials behind the weight stream.
__device__ __forceinline__ float smi_ss_lane_sum(const float* sp, int npart, int lane) {
  float v = 0.f;
  for (int i0 = lane; i0 < npart; i0 += 256) {   // block-uniform trip count is not required: lanes past npart add zeros
    const int i1 = i0 + 64, i2 = i0 + 128, i3 = i0 + 192, last = npart - 1;
    float a0 = sp[i0 < npart ? i0 : last], a1 = sp[i1 < npart ? i1 : last], a2 = sp[i2 < npart ? i2 : last], a3 = sp[i3 < npart ? i3 : last];
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
    v += a0;                         // i0 < npart by the loop condition
    v += i1 < npart ? a1 : 0.f;
    v += i2 < npart ? a2 : 0.f;
    v += i3 < npart ? a3 : 0.f;
  }
  return v;
}

// One-row decode kernels: every 64-byte line of the kernel arguments is requested at entry, together.  Left to itself the
// compiler asks for them as they are needed -- the helper test (work_blocks), then the work path's pointers -- and every
// first touch of a line is a scalar-cache miss: two or three round trips in a row in front of the first weight load.
__device__ __forceinline__ void smi_kernarg_lines(const GemmP& p) {
  asm volatile("" ::"s"(p.W), "s"(p.bias), "s"(p.work_blocks), "s"(p.pf.base), "s"(p.Yin), "s"(gridDim.x));
}

// Hot entries (one-row decode): a second __global__ entry of a one-row kernel whose LEADING parameters are the values on the
// address path of its first loads and of the helper-block test -- pointers first, then ints, at most 14 dwords -- followed by the
// usual struct.  Built with -amdgpu-kernarg-preload-count (Makefile) those dwords are in SGPRs when the wave starts, so the
// first weight / K / V / partial loads leave without a scalar round trip to the kernel-argument segment in front of them (the
// struct's other lines are requested by the compiler where the epilogue needs them, behind those loads).  The launcher passes
// the hot values from the same struct it passes behind them; the body is shared with the struct-only entry, which every other
// instantiation keeps.  A kernel whose first parameter is a struct gets no preload and compiles as without the flag.
template <int MT, int NTB, int NW, int U, int WB, int PRO, int EPI, int KVF32, int H = 1, int OCC = 1, int LEAN = 0, int NOH = kMaxOHeads>
__device__ __forceinline__ void gemm_body(const GemmP& p) {
  static_assert(EPI == EPI_QKV || KVF32 == 0, "the cache type is a parameter of the kernels that write the cache");
  static_assert(H == 1 || ((H == 2 || H == 4) && NTB == 1 && EPI == EPI_RESID), "row-split tiles: RESID, one tile per block");
  static_assert(PRO != PRO_FUSEDO || (LEAN == 2 && MT == 1 && EPI == EPI_SWIGLU), "PRO_FUSEDO: the one-row gate_up kernel");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // QHOT: the one-row QKV.  Its first MFMA waits for the operand staging load and the RMSNorm partials -- written by the previous
  // launch, a full memory round trip away -- so these are requested first, from preloaded values only, before the row
  // descriptor and any other field of the struct is read (below).  Its wave index is a scalar, so tile indices, clamps and tile
  // base addresses are computed once per wave on the scalar unit and a load's address is a scalar base plus a 32-bit lane offset.
  // (The same scalar wave index in gate_up and k_down1, with k_down1's block-id division replaced by compares: built, same
  // bits, no faster on the step -- profiles/entry_loads_vs_parent.txt -- so they keep the parent's code.)
  constexpr bool QHOT = LEAN == 2 && EPI == EPI_QKV && PRO == PRO_NORM && MT == 1 && NTB == 1 && WB == 1 && H == 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = QHOT ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  if ((int)blockIdx.x >= p.work_blocks) {
    pf_run(p.pf, (int)blockIdx.x - p.work_blocks, (int)gridDim.x - p.work_blocks, tid, NW * 64);
    return;
  }
  const int bx = (int)blockIdx.x;
  const int KT = p.KT, M = LEAN == 2 ? 1 : p.M, NT = p.NT;   // LEAN == 2: exactly one row (batch-1 decode), folded at compile time
  const int mbase = LEAN == 2 ? 0 : (int)blockIdx.y * (MT * 16);   // row group (grid.y > 1: a prompt's rows, 32 per block row)
  const int nblk = p.work_blocks / H;   // blocks per row part; part r of tile t is block r * nblk + t (same XCD for all r)
  const int part = H > 1 ? (int)blockIdx.x / nblk : 0;
  const int nt0 = (H > 1 ? (int)blockIdx.x % nblk : (int)blockIdx.x) * NTB;
  const bool wact = H == 1 || ((lane & 15) >> (H == 2 ? 3 : 2)) == part;   // this lane's weight row is in the part
  const bool ract = H == 1 || ((lane >> 4) >> (H == 2 ? 1 : 0)) == part;   // this lane's 4 output columns are
#define SMI_STAMP(i) do { if (!LEAN && p.stamps && tid == 0) p.stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  SMI_STAMP(0);
  float4* red = (float4*)smem;                                   // [NW][NTB][MT][64]
  float* rarr = (float*)(smem + (size_t)NW * NTB * MT * 1024);  // [32] per-row RMSNorm factor
  float* bestv = rarr + 32;                                      // LM: [NTB][32]
  int* besti = (int*)(bestv + NTB * 32);

  // ---- operands in flight: the (cold, HBM) weight tiles of the first WB batches are requested up
  //      front; the activation triples (small, L2) are fetched per batch
  uint4 w[WB][U][NTB];
  bf16x8 bf[U][3][MT];
  const int k8 = lane >> 4;
  int mrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) { const int m = mbase + mt * 16 + (lane & 15); mrow[mt] = m < M ? m : M - 1; }
  const int wl = (H > 1 || EPI == EPI_RESID) ? smi_wlane(lane, p.wperm) : lane;
  auto load_w = [&](uint4 (&dst)[U][NTB], int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int j = j0 + u * NW;
      j = j < KT ? j : KT - 1;
#pragma unroll
      for (int nb = 0; nb < NTB; ++nb) {
        int nt = nt0 + nb;
        nt = nt < NT ? nt : NT - 1;
        dst[u][nb] = wact ? smi_ldw(&p.W[((size_t)nt * KT + j) * 64 + wl]) : make_uint4(0u, 0u, 0u, 0u);
      }
    }
  };
  auto load_bf = [&](int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int j = j0 + u * NW;
      j = j < KT ? j : KT - 1;
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bf[u][s][mt] = *(const bf16x8*)(p.XS + xs_off(j, s, k8, mrow[mt], M));
    }
  };
  // QKV: the epilogue's row descriptors are requested FIRST, so the counted wait for them does not include the weight
  // stream and the RoPE factors (addressed by the row's position) can be requested while the weights are in flight
  const int em = lane & 15;
  RowDesc erd[MT];
  if (EPI == EPI_QKV && wave < NTB && nt0 + wave < NT) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mbase + mt * 16 + em;
      if (LEAN != 2) erd[mt] = p.rows[m < M ? m : M - 1];
    }
  }
  // Non-LEAN PRO_NORM kernels (QKV / gate_up at 6+ rows): the partial sums of squares of the rows whose RMSNorm factor this wave
  // computes (rows wave, wave + NW, ...) are requested HERE, before the weight stream, and summed only after the MFMA loop (the
  // factor is an epilogue operand).  As a row-by-row loop in front of the MFMAs (where the compiler kept it: round-4 ISA of the
  // 32-row gate_up) every row was a dependent L2 round trip behind a vmcnt(0) that also covered all weight and operand loads:
  // four round trips per wave between the last operand byte and the first MFMA.
  constexpr int RPW = (MT * 16 + NW - 1) / NW;
  constexpr bool SS_EARLY = !LEAN && PRO == PRO_NORM && RPW <= 4;
  float ssv[SS_EARLY ? RPW : 1][4];
  const bool ss_early = SS_EARLY && p.npart <= 256;
  if constexpr (SS_EARLY) {
    if (ss_early) {
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        int m = mbase + wave + i * NW;
        m = m < M ? m : M - 1;
        const float* sp = p.sspart + (size_t)m * p.npart;
        const int last = p.npart - 1;
        ssv[i][0] = sp[lane < last ? lane : last]; ssv[i][1] = sp[lane + 64 < last ? lane + 64 : last];
        ssv[i][2] = sp[lane + 128 < last ? lane + 128 : last]; ssv[i][3] = sp[lane + 192 < last ? lane + 192 : last];
      }
    }
  }
  // PRO_FUSEDO: the per-head o_proj partials, the residual row and gamma of this wave's k tiles (two tiles per round, lane =
  // one k) are requested BEFORE the weight tiles: loads return in issue order, so behind the (cold) weights they would only
  // arrive after them and the whole operand build would sit between the weights' arrival and the first MFMA
  constexpr int FRND = PRO == PRO_FUSEDO ? 2 : 1;
  float fpv[FRND][NOH], fhv[FRND], fgv[FRND];   // NOH: the head count the instantiation is built for (PRO_FUSEDO: 14 or 4 -- no dead loads)
  int fkk[FRND];
  if constexpr (PRO == PRO_FUSEDO) {
    const int tw = (KT - wave + NW - 1) / NW, K = KT * 32;
#pragma unroll
    for (int r = 0; r < FRND; ++r) {
      const int tl = 2 * r + (lane >> 5);
      fkk[r] = (wave + (tl < tw ? tl : tw - 1) * NW) * 32 + (lane & 31);
#pragma unroll
      for (int hd = 0; hd < NOH; ++hd) fpv[r][hd] = p.part_o[(size_t)(hd < p.n_oheads ? hd : p.n_oheads - 1) * K + fkk[r]];
      fhv[r] = p.hres[fkk[r]]; fgv[r] = p.gam[fkk[r]];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  float qs0 = 0.f, qs1 = 0.f, qs2 = 0.f, qs3 = 0.f;   // QHOT: wave 0's RMSNorm partials (ss0 .. ss3 below)
  if constexpr (QHOT) {
    // Every address here is a preloaded base (W, XS, sspart) plus 32-bit offsets; a wave without a k tile (KT < NW) requests
    // nothing.  The operand goes first: loads return in issue order, and the weights behind it are mostly L2-warm (gate_up and
    // down_proj touch them) -- measured against weights first, graph step 487.9 against 489.4 us.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int tw = (KT - wave + NW - 1) / NW;          // this wave's k tiles
    const int tl = lane >> 4, r = lane & 15;           // 16 lanes fetch a tile's 12 pieces: four tiles per round
    u32x4 v0 = {0u, 0u, 0u, 0u};
    auto req_w = [&]() {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int j = wave + u * NW;
        j = j < KT ? j : KT - 1;
        const unsigned char* wb = (const unsigned char*)p.W + (((size_t)bx * KT + j) << 10);   // block bx is n tile bx (< NT)
        w[0][u][0] = smi_ldw((const uint4*)(wb + (uint32_t)lane * 16u));
      }
    };
    auto req_x = [&]() {
      v0 = *(const u32x4*)(p.XS + (uint32_t)((wave + (tl < tw ? tl : tw - 1) * NW) * 192 + (r < 12 ? r : 11) * 16));
      if (p.npart <= 256 && wave == 0) {   // ss_pre (below): the one row is wave 0's
        const int last = p.npart - 1;
        const unsigned char* sp = (const unsigned char*)p.sspart;
        qs0 = *(const float*)(sp + (uint32_t)(lane < last ? lane : last) * 4u);
        qs1 = *(const float*)(sp + (uint32_t)(lane + 64 < last ? lane + 64 : last) * 4u);
        qs2 = *(const float*)(sp + (uint32_t)(lane + 128 < last ? lane + 128 : last) * 4u);
        qs3 = *(const float*)(sp + (uint32_t)(lane + 192 < last ? lane + 192 : last) * 4u);
      }
    };
    unsigned long long rdesc = 0;
    if (tw > 0) {
      req_x();
      req_w();
    }
    // the row's descriptor sits at a uniform address, so it comes through the SCALAR cache (not counted by vmcnt).  Requested
    // here, behind the vector requests; nothing looks at it before the wait below -- the compiler does not know that the pair is
    // still being written, so no instruction may name it in between (tests/test_entry_waits_cpu.py reads the built library for
    // that).  The descriptor is rewritten by k_finalize
    // every step; like every compiler-scalarised load of data an earlier kernel wrote, this relies on the scalar-cache
    // invalidate of the dispatch's acquire fence (with `glc` the load is 1.3 us slower: 630 -> 662 us per step).
    if (wave == 0) asm volatile("s_load_dwordx2 %0, %1, 0x0" : "=s"(rdesc) : "s"(p.rows) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (tw > 0) {
      // the staging wait: operand and partials (issued first: a counted wait, the two weight tiles behind them stay in flight)
      asm volatile("" : "+v"(v0), "+v"(qs0), "+v"(qs1), "+v"(qs2), "+v"(qs3));
      unsigned char* qbw = smem + (size_t)NW * NTB * MT * 1024 + 32 * 4 + NTB * 32 * 8 + (size_t)wave * p.ldsb;
      if (tl < tw && r < 12) *(u32x4*)(qbw + ((size_t)tl * 12 + r) * 16) = v0;
    }
    // RoPE, bias and the KV append are epilogue work: the descriptor and the struct's other lines are first used from here on
    if (wave == 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(rdesc) : : "memory");
      erd[0].slot = (int32_t)(uint32_t)rdesc;
      erd[0].pos = (int32_t)(uint32_t)(rdesc >> 32);
    }
    __builtin_amdgcn_sched_barrier(0);
  } else {
#pragma unroll
    for (int b = 0; b < WB; ++b)
      if (wave + b * NW * U < KT) load_w(w[b], wave + b * NW * U);
  }
  // PRO_FUSEDO (gate_up at one row, 608 blocks): every block also touches its share -- one wave-instruction, a dword per 64-byte
  // line -- of the NEXT layer's QKV weights, right behind its own weight loads: the 2 MB are then in the L2 of the XCD whose QKV
  // blocks read them (consumer slice s is read by block s; 72 slices, 8 XCDs: block j takes slice j mod 72 -- same XCD) when
  // QKV starts two launches later, instead of a cold HBM round trip in front of a 3-us kernel.  The value is only kept alive
  // until the MFMA loop is over (the loads return in order behind the weights; nothing waits for them).
  uint32_t pf2v = 0;
  if constexpr (PRO == PRO_FUSEDO) {
    if (p.pf2_base && wave == NW - 1) {
      const int sl = bx % p.pf2_nslices, part = bx / p.pf2_nslices, nparts = (p.work_blocks + p.pf2_nslices - 1) / p.pf2_nslices;
      const int lines = p.pf2_slice >> 6, per = (lines + nparts - 1) / nparts;
      int ln = part * per + (lane < per ? lane : per - 1);
      ln = ln < lines ? ln : lines - 1;
      pf2v = *(const uint32_t*)(p.pf2_base + (size_t)sl * p.pf2_slice + (size_t)ln * 64);
    }
  }
  static_assert(LEAN != 2 || EPI != EPI_QKV || QHOT, "one row, QKV: the form that reads its row descriptor above (QHOT)");
  // ---- epilogue operands that do not depend on the GEMM: requested BEFORE the operand staging below, so that the
  // staging wait covers them too (behind it, the first MFMA waited one more L2 round trip for the bias / residual row).
  // (Not so for QHOT: its staging is done by here, so bias and RoPE are requested BEHIND the staging wait -- they need the
  // descriptor and the struct's lines, which that form reads only there -- and are in flight under the norm factor and the MFMAs.)
  float4 epre[MT], egam = make_float4(0.f, 0.f, 0.f, 0.f);
  float2 erope[MT][2];
  if (wave < NTB && nt0 + wave < NT) {
    const int n = (nt0 + wave) * 16 + 4 * (lane >> 4);
    if (EPI == EPI_RESID) egam = *(const float4*)(p.gamma_next + n);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mbase + mt * 16 + em;
      if (m < M && ract) {
        if (EPI == EPI_QKV) {
          epre[mt] = *(const float4*)(p.bias + n);
          if (n < p.q_dim + p.kv_dim) {
            const int i0 = (n & 63) >> 1;
            erope[mt][0] = p.rope[(size_t)erd[mt].pos * 32 + i0];
            erope[mt][1] = p.rope[(size_t)erd[mt].pos * 32 + i0 + 1];
          }
        }
        if (EPI == EPI_RESID) epre[mt] = *(const float4*)((p.Yin ? p.Yin : p.Y) + (size_t)m * (NT * 16) + n);
      }
    }
  }
  // few rows (MT == 1, ldsb > 0): a k tile's 12*M operand pieces are contiguous in XS, so the wave pulls
  // them with full-width loads into its own LDS slice (no block barrier) instead of 3 narrow loads per tile
  const bool vlds = LEAN || (MT == 1 && p.ldsb > 0);
  // LEAN PRO_NORM kernels: the partial sums of squares of the row this wave owns (row `wave` of the group) are requested
  // together with its first staging round
  float ss0 = qs0, ss1 = qs1, ss2 = qs2, ss3 = qs3;   // zeros, except QHOT: requested above
  const bool ss_pre = LEAN >= 1 && PRO == PRO_NORM && p.npart <= 256 && wave < MT * 16 && mbase + wave < M;
  unsigned char* bw = smem + (size_t)NW * NTB * MT * 1024 + 32 * 4 + NTB * 32 * 8 + (size_t)wave * p.ldsb;
  float* ssp = (float*)(smem + (size_t)NW * NTB * MT * 1024 + 32 * 4 + NTB * 32 * 8 + (size_t)NW * p.ldsb);   // PRO_FUSEDO: [K / 4] partial sums of squares
  if constexpr (PRO == PRO_FUSEDO) {
    // The operand of this GEMV is gamma * (h + o_proj(attention)), and the o_proj arrives as one partial per head.  Each wave
    // builds the 32-value tiles it owns: lane = one k (two tiles per round), heads added in order (the order k_gemm<RESID> with
    // NW = heads sums its waves in), then exactly the RESID epilogue's arithmetic: residual add, sum of squares per 4 columns,
    // gamma, exact 3-way split -- written as B-operand pieces into the wave's private staging slice.  All loads of a round
    // are issued together; they are L2 hits and land long before the weight tiles requested above.
    const int tw = (KT - wave + NW - 1) / NW;
#pragma unroll
    for (int r = 0; r < FRND; ++r) {
      const int tl = 2 * r + (lane >> 5), k = fkk[r];
      const bool ok = tl < tw;
      float (&pv)[FRND][NOH] = fpv;
      float (&hv)[FRND] = fhv;
      float (&gv)[FRND] = fgv;
      float y = pv[r][0];
#pragma unroll
      for (int hd = 1; hd < NOH; ++hd)
        if (hd < p.n_oheads) y += pv[r][hd];   // wave-uniform
      const float hm = hv[r] + y;
      uint32_t hi, mi, lo;
      split3(gv[r] * hm, hi, mi, lo);
      float sq = hm * hm;
      sq += __shfl_xor(sq, 1, 64);
      sq += __shfl_xor(sq, 2, 64);          // lanes k % 4 == 0: (x^2 + y^2) + (z^2 + w^2), the RESID epilogue's partial
      if (ok) {
        unsigned char* q = bw + (size_t)(tl * 12 + ((lane >> 3) & 3)) * 16 + (lane & 7) * 2;
        *(uint16_t*)q = (uint16_t)hi;
        *(uint16_t*)(q + 64) = (uint16_t)mi;
        *(uint16_t*)(q + 128) = (uint16_t)lo;
        if ((lane & 3) == 0) ssp[k >> 2] = sq;
        if (blockIdx.x == 0) p.h2out[k] = hm;
      }
    }
  } else if (vlds) {
    const int tw = (KT - wave + NW - 1) / NW;          // this wave's k tiles
    const int lts = LEAN == 2 ? 4 : p.lt_shift;
    const int per = 64 >> lts, pm = 12 * M;
    const int r = lane & ((1 << lts) - 1);
    // one row, many k tiles per wave (down_proj: 152 tiles over 16 waves = 3 rounds of 4 tiles): all rounds' loads leave
    // before the first LDS write -- one at a time each round was a full L2 round trip behind the weight stream
    constexpr int RIF = (LEAN == 2 && WB >= 4) ? 3 : 1;   // rounds in flight
    if constexpr (RIF > 1) {
      // (named registers and unconditional loads from clamped addresses: a conditionally written `uint4 v[3]` stays in
      // scratch memory, and `ok ? *p : zero` becomes a flat load through a select between p and a stack slot)
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const int rc = r < pm ? r : pm - 1;
      for (int t0 = 0; t0 < tw; t0 += per * 3) {
        const int ta = t0 + (lane >> lts), tb = ta + per, tc = tb + per;
        u32x4 va = *(const u32x4*)(p.XS + xs_off(wave + (ta < tw ? ta : tw - 1) * NW, 0, 0, 0, M) + rc * 16);
        u32x4 vb = *(const u32x4*)(p.XS + xs_off(wave + (tb < tw ? tb : tw - 1) * NW, 0, 0, 0, M) + rc * 16);
        u32x4 vc = *(const u32x4*)(p.XS + xs_off(wave + (tc < tw ? tc : tw - 1) * NW, 0, 0, 0, M) + rc * 16);
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc));   // all three loads are issued here, not sunk into the branches below
        if (ta < tw && r < pm) *(u32x4*)(bw + ((size_t)ta * pm + r) * 16) = va;
        if (tb < tw && r < pm) *(u32x4*)(bw + ((size_t)tb * pm + r) * 16) = vb;
        if (tc < tw && r < pm) *(u32x4*)(bw + ((size_t)tc * pm + r) * 16) = vc;
      }
    } else {
      int t0 = 0;
      if constexpr (QHOT) {
        if (tw > 0) t0 = per;   // the first round is in LDS already (above)
      } else if constexpr (LEAN >= 1 && PRO == PRO_NORM) {
        // first staging round and this wave's RMSNorm partials (if it owns a row) behind ONE wait: two round trips -> one
        if (tw > 0) {
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const int tl = lane >> lts;
          u32x4 v0 = *(const u32x4*)(p.XS + xs_off(wave + (tl < tw ? tl : tw - 1) * NW, 0, 0, 0, M) + (r < pm ? r : pm - 1) * 16);
          if (ss_pre) {
            const float* sp = p.sspart + (size_t)(mbase + wave) * p.npart;
            const int last = p.npart - 1;
            ss0 = sp[lane < last ? lane : last]; ss1 = sp[lane + 64 < last ? lane + 64 : last];
            ss2 = sp[lane + 128 < last ? lane + 128 : last]; ss3 = sp[lane + 192 < last ? lane + 192 : last];
          }
          asm volatile("" : "+v"(v0), "+v"(ss0), "+v"(ss1), "+v"(ss2), "+v"(ss3));
          if (tl < tw && r < pm) *(u32x4*)(bw + ((size_t)tl * pm + r) * 16) = v0;
          t0 = per;
        }
      }
      for (; t0 < tw; t0 += per) {
        const int tl = t0 + (lane >> lts);
        if (tl < tw && r < pm) {
          const uint4 v = *(const uint4*)(p.XS + xs_off(wave + tl * NW, 0, 0, 0, M) + r * 16);
          *(uint4*)(bw + ((size_t)tl * pm + r) * 16) = v;
        }
      }
    }
  } else if (wave < KT) {
    load_bf(wave);
  }

  // ---- RMSNorm factor per row from the producer's partial sums (fixed order: DPP tree over partials)
  if (PRO == PRO_NORM && !ss_early) {
    for (int ml = wave; ml < MT * 16 && mbase + ml < M; ml += NW) {
      float v;
      if (ss_pre && ml == wave) {   // same order as smi_ss_lane_sum
        v = lane < p.npart ? ss0 : 0.f;
        v += lane + 64 < p.npart ? ss1 : 0.f;
        v += lane + 128 < p.npart ? ss2 : 0.f;
        v += lane + 192 < p.npart ? ss3 : 0.f;
      } else {
        v = smi_ss_lane_sum(p.sspart + (size_t)(mbase + ml) * p.npart, p.npart, lane);
      }
      v = smi_wave_sum(v);
      if (lane == 0) rarr[ml] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
    }
  }
  SMI_STAMP(1);

  f32x4 acc[3][NTB][MT];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < NTB; ++a)
#pragma unroll
      for (int b = 0; b < MT; ++b) acc[c][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (vlds) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own staging writes have landed (same wave reads them)
  auto compute = [&](const uint4 (&wt)[U][NTB], int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u * NW < KT) {
        if constexpr (LEAN == 2) {
          // ONE row: the three split terms of the operand are three COLUMNS of one MFMA (lane (k8, col): col 0 hi, 1 mid, 2 lo;
          // the other columns repeat hi and are never read), not three MFMAs with the same operand in every column.  A
          // column's sum does not depend on its neighbours, so column c is bit for bit the old accumulator of split c -- one
          // third of the matrix-pipe work and of the operand reads behind the last weight byte (the kernel's tail).
          const bf16x8 b1 = *(const bf16x8*)(bw + ((size_t)((j0 - wave) / NW + u) * 12 + ((lane & 15) < 3 ? (lane & 15) : 0) * 4 + k8) * 16);
#pragma unroll
          for (int nb = 0; nb < NTB; ++nb)
            acc[0][nb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wt[u][nb]), b1, acc[0][nb][0], 0, 0, 0);
          continue;
        }
        if (vlds) {
          const unsigned char* bp = bw + ((size_t)((j0 - wave) / NW + u) * 12 * M + k8 * M + mrow[0]) * 16;
#pragma unroll
          for (int s = 0; s < 3; ++s) bf[u][s][0] = *(const bf16x8*)(bp + (size_t)s * 4 * M * 16);
        }
#pragma unroll
        for (int nb = 0; nb < NTB; ++nb) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, wt[u][nb]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[2][nb][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][2][mt], acc[2][nb][mt], 0, 0, 0);
            acc[1][nb][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][1][mt], acc[1][nb][mt], 0, 0, 0);
            acc[0][nb][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][0][mt], acc[0][nb][mt], 0, 0, 0);
          }
        }
      }
    }
  };
#pragma unroll
  for (int b = 0; b < WB; ++b) {
    const int j0 = wave + b * NW * U;
    if (j0 < KT) {
      if (b > 0 && !vlds) load_bf(j0);
      compute(w[b], j0);
    }
  }
  for (int j0 = wave + WB * NW * U; j0 < KT; j0 += NW * U) {   // only for K beyond NW*U*WB tiles
    load_w(w[0], j0);
    if (!vlds) load_bf(j0);
    compute(w[0], j0);
  }
  if constexpr (PRO == PRO_FUSEDO) asm volatile("" ::"v"(pf2v));
  if constexpr (SS_EARLY) {
    if (ss_early) {   // the partials requested at entry: same order as smi_ss_lane_sum + smi_wave_sum
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int ml = wave + i * NW;
        asm volatile("" : "+v"(ssv[i][0]), "+v"(ssv[i][1]), "+v"(ssv[i][2]), "+v"(ssv[i][3]));   // first looked at here, behind the MFMAs
        float v = lane < p.npart ? ssv[i][0] : 0.f;
        v += lane + 64 < p.npart ? ssv[i][1] : 0.f;
        v += lane + 128 < p.npart ? ssv[i][2] : 0.f;
        v += lane + 192 < p.npart ? ssv[i][3] : 0.f;
        v = smi_wave_sum(v);
        if (lane == 0 && ml < MT * 16 && mbase + ml < M) rarr[ml] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
      }
    }
  }
  SMI_STAMP(4);
  // ---- split-K reduction across the block's waves (fixed order => deterministic)
#pragma unroll
  for (int nb = 0; nb < NTB; ++nb)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      f32x4 t;
      if constexpr (LEAN == 2) {   // columns 1 / 2 (lanes + 1 / + 2 of the row of 16) hold mid / lo; only column 0 -- the row -- is read later
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = (smi_dpp<0x102>(acc[0][nb][mt][r]) + smi_dpp<0x101>(acc[0][nb][mt][r])) + acc[0][nb][mt][r];
      } else {
        t = (acc[2][nb][mt] + acc[1][nb][mt]) + acc[0][nb][mt];   // (lo + mid) + hi
      }
      red[((wave * NTB + nb) * MT + mt) * 64 + lane] = make_float4(t[0], t[1], t[2], t[3]);
    }
  if (EPI == EPI_LM) {
    for (int i = tid; i < NTB * 32; i += NW * 64) { bestv[i] = -INFINITY; besti[i] = 0x7fffffff; }
  }
  __syncthreads();
  SMI_STAMP(5);

  const int N = NT * 16;
  // SPREAD (gate_up with two m-tiles): the NTB * MT (tile, m-tile) pairs go to NTB * MT different waves instead of NTB waves
  // finishing MT pairs each (five of the eight waves used to idle through the epilogue: two expf, two divides, two exact splits
  // per pair).  Only kernels whose epilogue needs no per-wave prefetched operands (SWIGLU) do this.
  constexpr bool SPREAD = EPI == EPI_SWIGLU && MT == 2 && NTB * MT <= NW;
  for (int nb = SPREAD ? wave / MT : wave; nb < NTB; nb += NW) {
    const int nt = nt0 + nb;
    if (nt >= NT) continue;  // wave-uniform
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (SPREAD && mt != wave % MT) continue;   // wave-uniform
      float4 s = red[((0 * NTB + nb) * MT + mt) * 64 + lane];
#pragma unroll
      for (int wv = 1; wv < NW; ++wv) {
        const float4 t = red[((wv * NTB + nb) * MT + mt) * 64 + lane];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      const int ml = mt * 16 + em, m = mbase + ml;
      const int n = nt * 16 + 4 * (lane >> 4);
      const bool valid = m < M && ract;
      if (PRO == PRO_NORM) {
        const float r = rarr[m < M ? ml : 0];
        s.x *= r; s.y *= r; s.z *= r; s.w *= r;
      }
      if constexpr (PRO == PRO_FUSEDO) {   // the waves left their partial sums of squares in LDS; summed as smi_ss_lane_sum would
        const int npart = KT * 8;
        float v = lane < npart ? ssp[lane] : 0.f;
        v += lane + 64 < npart ? ssp[lane + 64] : 0.f;
        v += lane + 128 < npart ? ssp[lane + 128] : 0.f;
        v += lane + 192 < npart ? ssp[lane + 192] : 0.f;
        v = smi_wave_sum(v);
        const float r = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
        s.x *= r; s.y *= r; s.z *= r; s.w *= r;
      }
      if (EPI == EPI_RESID) {
        float ssq = 0.f;
        if (valid) {
          float4 h = epre[mt];   // fetched at kernel entry (only this lane ever writes it)
          h.x += s.x; h.y += s.y; h.z += s.z; h.w += s.w;
          *(float4*)(p.Y + (size_t)m * N + n) = h;
          ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
          // next consumer's operand: exact triples of gamma_next * h_new (4 of the 8 values of an octet)
          const float t[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
          uint32_t hi[4], mi[4], lo[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split3(t[e], hi[e], mi[e], lo[e]);
          const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
          const size_t pl = (size_t)4 * M * 16;
          *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
          *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
          *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
        }
        // one partial per 4 columns (this tile's 16 columns of row m sit in lanes em, em+16, em+32, em+48)
        if (valid) p.ssout[((size_t)m * NT + nt) * 4 + (lane >> 4)] = ssq;
      } else if (EPI == EPI_SWIGLU) {
        if (valid) {
          // rows are (gate, up, gate, up): silu(g) * u, MQ:46-48
          const float a0 = (s.x / (1.0f + expf(-s.x))) * s.y;
          const float a1 = (s.z / (1.0f + expf(-s.z))) * s.w;
          uint32_t h0, m0, l0, h1, m1, l1;
          split3(a0, h0, m0, l0);
          split3(a1, h1, m1, l1);
          const int k = n >> 1;   // activation index of a0
          const size_t o = xs_off(k >> 5, 0, (k >> 3) & 3, m, M) + ((k >> 1) & 3) * 4;
          const size_t pl = (size_t)4 * M * 16;
          *(uint32_t*)(p.XSout + o) = h0 | (h1 << 16);
          *(uint32_t*)(p.XSout + o + pl) = m0 | (m1 << 16);
          *(uint32_t*)(p.XSout + o + 2 * pl) = l0 | (l1 << 16);
        }
      } else if (EPI == EPI_QKV) {
        if (valid) {
          const float4 b = epre[mt];
          s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
          const RowDesc rd = erd[mt];
          if (n < p.q_dim + p.kv_dim) {
            // rows inside a head are ordered (0,32,1,33,..): (s.x,s.y) and (s.z,s.w) are RoPE pairs
            const float2 c0 = erope[mt][0], c1 = erope[mt][1];   // requested in the prologue
            float4 r;
            r.x = __fadd_rn(__fmul_rn(s.x, c0.x), __fmul_rn(-s.y, c0.y));  // x1*cos + (-x2)*sin
            r.y = __fadd_rn(__fmul_rn(s.y, c0.x), __fmul_rn(s.x, c0.y));   // x2*cos + x1*sin
            r.z = __fadd_rn(__fmul_rn(s.z, c1.x), __fmul_rn(-s.w, c1.y));
            r.w = __fadd_rn(__fmul_rn(s.w, c1.x), __fmul_rn(s.z, c1.y));
            s = r;
          }
          if (n < p.q_dim) {
            *(float4*)(p.Y + (size_t)m * p.q_dim + n) = s;
          } else {
            const bool isk = n < p.q_dim + p.kv_dim;
            const int c = n - p.q_dim - (isk ? 0 : p.kv_dim);
            const size_t off = kv_row(p.km, rd.slot, c >> 6, p.n_kv, p.max_pos, rd.pos) * 64 + (c & 63);
            void* base = isk ? p.kcache : p.vcache;
            if (KVF32) {
              *(float4*)((float*)base + off) = s;
            } else {
              uint2 pk;
              pk.x = smi_f32_to_bf16(s.x) | (smi_f32_to_bf16(s.y) << 16);
              pk.y = smi_f32_to_bf16(s.z) | (smi_f32_to_bf16(s.w) << 16);
              *(uint2*)((uint16_t*)base + off) = pk;
            }
          }
        }
      } else {  // EPI_LM
        if (valid && p.Y) {
          float* y = p.Y + (size_t)m * p.V + n;
          if (n + 0 < p.V) y[0] = s.x;
          if (n + 1 < p.V) y[1] = s.y;
          if (n + 2 < p.V) y[2] = s.z;
          if (n + 3 < p.V) y[3] = s.w;
        }
        // lane-local best over its 4 rows (ascending n, strict > keeps the lowest index on ties)
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.V && sv[r] > bv) { bv = sv[r]; bi = n + r; }
        // combine the 4 lanes that share this m (lane, lane^16, lane^32, lane^48)
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          float ov = __shfl_xor(bv, o, 64);
          int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane < 16 && valid) { bestv[nb * 32 + ml] = bv; besti[nb * 32 + ml] = bi; }
      }
    }
  }
  SMI_STAMP(6);
  if (EPI == EPI_LM) {
    __syncthreads();
    if (tid < MT * 16 && mbase + tid < M) {   // this block row's rows (33 .. 64 rows: two block rows of 32)
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int nb = 0; nb < NTB; ++nb) {
        float ov = bestv[nb * 32 + tid];
        int oi = besti[nb * 32 + tid];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      p.pval[(size_t)(mbase + tid) * p.work_blocks + blockIdx.x] = bv;   // [row][block]: finalize reads a row contiguously
      p.pidx[(size_t)(mbase + tid) * p.work_blocks + blockIdx.x] = bi;
    }
  }
}

template <int MT, int NTB, int NW, int U, int WB, int PRO, int EPI, int KVF32, int H = 1, int OCC = 1, int LEAN = 0, int NOH = kMaxOHeads>
__global__ __launch_bounds__(NW * 64, OCC) void k_gemm(GemmP p) {
  if constexpr (LEAN == 2) smi_kernarg_lines(p);
  gemm_body<MT, NTB, NW, U, WB, PRO, EPI, KVF32, H, OCC, LEAN, NOH>(p);
}
// Hot entry of the one-row QKV (PRO_NORM: a = XS, b = sspart, c = rows, n = npart) and gate_up (PRO_FUSEDO: a = part_o, b = hres,
// c = gam, n = n_oheads) kernels: 13 dwords (ldsb: left in the struct, the compiler fetches it at entry together with a helper
// field and the work path then waits for that load in front of its first loads)
template <int MT, int NTB, int NW, int U, int WB, int PRO, int EPI, int KVF32, int H = 1, int OCC = 1, int LEAN = 0, int NOH = kMaxOHeads>
__global__ __launch_bounds__(NW * 64, OCC) void k_gemm_hot(const uint4* W, const void* a, const void* b, const void* c, int KT, int NT,
                                                           int work_blocks, int n, int ldsb, GemmP p) {
  static_assert(LEAN == 2 && (PRO == PRO_FUSEDO || (PRO == PRO_NORM && EPI == EPI_QKV)), "hot entries: the one-row QKV and gate_up kernels");
  GemmP q = p;
  q.W = W; q.KT = KT; q.NT = NT; q.work_blocks = work_blocks; q.ldsb = ldsb;
  if constexpr (PRO == PRO_FUSEDO) { q.part_o = (const float*)a; q.hres = (const float*)b; q.gam = (const float*)c; q.n_oheads = n; }
  else { q.XS = (const unsigned char*)a; q.sspart = (const float*)b; q.rows = (const RowDesc*)c; q.npart = n; }
  gemm_body<MT, NTB, NW, U, WB, PRO, EPI, KVF32, H, OCC, LEAN, NOH>(q);
}
// the hot entry's launch: the hot values come from the struct that travels behind them
template <int MT, int NTB, int NW, int U, int WB, int PRO, int EPI, int KVF32, int H, int OCC, int NOH = kMaxOHeads>
void launch_gemm_hot(const GemmP& p, dim3 grid, size_t lds, hipStream_t st) {
  if constexpr (PRO == PRO_FUSEDO)
    hipLaunchKernelGGL((k_gemm_hot<MT, NTB, NW, U, WB, PRO, EPI, KVF32, H, OCC, 2, NOH>), grid, dim3(NW * 64), lds, st, p.W, (const void*)p.part_o,
                       (const void*)p.hres, (const void*)p.gam, p.KT, p.NT, p.work_blocks, p.n_oheads, p.ldsb, p);
  else
    hipLaunchKernelGGL((k_gemm_hot<MT, NTB, NW, U, WB, PRO, EPI, KVF32, H, OCC, 2, NOH>), grid, dim3(NW * 64), lds, st, p.W, (const void*)p.XS,
                       (const void*)p.sspart, (const void*)p.rows, p.KT, p.NT, p.work_blocks, p.npart, p.ldsb, p);
}

// ------------------------------------------------------------------------------------------
// One-row RESID GEMV with four row parts per weight tile (down_proj at batch 1), FULL load instructions.
// k_gemm<.., H = 4> gives each of 16 waves one chain (k tiles kt mod 16) and, a part being 4 of a tile's 16 rows, loads with
// 16 of its 64 lanes: 160 quarter-full load instructions per block.  Here a wave owns FOUR chains and advances them with one
// MFMA: A row 4s + r = weight row r of the part in the k tile of chain 4 * wave + s, B column 3s + c = split c (hi, mid, lo)
// of that tile's operand; the four 4 x 3 diagonal blocks of D are the four chains' accumulators (the other blocks mix tiles
// and are never read).  One load instruction then carries 1 KiB (W_down is stored row-part-major: the part's 16 pieces of a
// k tile are 256 contiguous bytes), 40 per block.  A chain's sum, (lo + mid) + hi, and the in-order sum over the 16 chains are
// k_gemm's, so the result is the same bit for bit; measured on the stand-alone probe (tools/gemv_ab.py, csrc/diag/
// diag_gemv.hip): 5.92 -> 3.98 us per launch.  TPC = k tiles per chain the registers hold (KT <= 16 * TPC).
// ------------------------------------------------------------------------------------------
template <int TPC>
__device__ __forceinline__ void down1_body(const GemmP& p) {
  __shared__ __attribute__((aligned(16))) float red[16 * 4];   // read and written as float4
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= p.work_blocks) {
    pf_run(p.pf, (int)blockIdx.x - p.work_blocks, (int)gridDim.x - p.work_blocks, tid, 256);
    return;
  }
  const int KT = p.KT, NT = p.NT;
  const int nt = (int)blockIdx.x % NT, part = (int)blockIdx.x / NT;   // part r of tile t is block r * NT + t (same XCD for all r)
  const uint4* wt = p.W + (size_t)nt * KT * 64;
  const int row = lane & 15, k8 = lane >> 4;
  const int sa = row >> 2, r = row & 3;                                   // A: chain slot and weight row of this lane's row
  const int sb = row < 12 ? row / 3 : 0, c = row < 12 ? row % 3 : 0;      // B: chain slot and split term of this lane's column
  const int piece = p.wperm ? part * 16 + k8 * 4 + r : k8 * 16 + part * 4 + r;
  // the epilogue's operands (one lane per block owns the part's 4 output columns) are requested first: they are L2 hits
  // and must not queue behind the cold weight tiles
  const int n = nt * 16 + part * 4;
  float4 epre = make_float4(0.f, 0.f, 0.f, 0.f), egam = epre;
  if (tid == 0) {
    epre = *(const float4*)((p.Yin ? p.Yin : p.Y) + n);
    egam = *(const float4*)(p.gamma_next + n);
  }
  uint4 w[TPC];
  bf16x8 b[TPC];
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    int t = 4 * wave + sa + 16 * u;
    const bool ok = t < KT;
    t = ok ? t : KT - 1;
    w[u] = smi_ldw(wt + (size_t)t * 64 + piece);
    if (!ok) w[u] = make_uint4(0u, 0u, 0u, 0u);   // a chain's missing last tile adds zeros
  }
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    int t = 4 * wave + sb + 16 * u;
    t = t < KT ? t : KT - 1;
    b[u] = *(const bf16x8*)(p.XS + xs_off(t, c, k8, 0, 1));
  }
  __builtin_amdgcn_sched_barrier(0);   // every load of the wave is requested before the first MFMA's wait
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < TPC; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w[u]), b[u], acc, 0, 0, 0);
  // D: lane (col = lane & 15, g = lane >> 4) holds rows 4g .. 4g + 3 of column col; chain slot s is row group s, columns 3s .. 3s + 2
  float t4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) t4[e] = (smi_dpp<0x102>(acc[e]) + smi_dpp<0x101>(acc[e])) + acc[e];   // (lo + mid) + hi
  if (row == 3 * k8) *(float4*)(red + (4 * wave + k8) * 4) = make_float4(t4[0], t4[1], t4[2], t4[3]);
  __syncthreads();
  if (tid == 0) {
    float4 sres = *(const float4*)red;
#pragma unroll
    for (int ch = 1; ch < 16; ++ch) {   // the 16 chains in order, as k_gemm sums its 16 waves
      const float4 q = *(const float4*)(red + ch * 4);
      sres.x += q.x; sres.y += q.y; sres.z += q.z; sres.w += q.w;
    }
    // RESID epilogue of k_gemm for row 0, columns n .. n + 3
    float4 h = epre;
    h.x += sres.x; h.y += sres.y; h.z += sres.z; h.w += sres.w;
    *(float4*)(p.Y + n) = h;
    const float ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
    const float tv[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
    uint32_t hi[4], mi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split3(tv[e], hi[e], mi[e], lo[e]);
    const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, 0, 1) + ((n >> 2) & 1) * 8;
    const size_t pl = (size_t)4 * 16;
    *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
    *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
    p.ssout[(size_t)nt * 4 + part] = ssq;
  }
}
// The one entry, a hot one (12 dwords): the weight and operand addresses, the epilogue's two early loads (res = the residual row's source,
// Yin or else Y) and the helper test
template <int TPC>
__global__ __launch_bounds__(256) void k_down1_hot(const uint4* W, const unsigned char* XS, const float* res, const float* gamma_next, int KT,
                                                   int NT, int work_blocks, int wperm, GemmP p) {
  GemmP q = p;
  q.W = W; q.XS = XS; q.Yin = res; q.gamma_next = gamma_next; q.KT = KT; q.NT = NT; q.work_blocks = work_blocks; q.wperm = wperm;
  __builtin_assume(q.Yin != nullptr);
  down1_body<TPC>(q);
}
template <int TPC>
void launch_down1_hot(const GemmP& p, int grid, hipStream_t st) {
  hipLaunchKernelGGL(k_down1_hot<TPC>, dim3(grid), dim3(256), 0, st, p.W, p.XS, (const float*)(p.Yin ? p.Yin : p.Y), p.gamma_next, p.KT, p.NT,
                     p.work_blocks, p.wperm, p);
}

// The same for 2 .. 8 rows (k_downS<TPC, MG>, rows in MG groups of four): a wave's load instruction still carries four chains'
// parts; B column 4s + j = row 4g + j of the tile of chain slot s, one MFMA per split term and row group (3 * MG per step
// instead of 12 with quarter-full loads), accumulators and summation order as k_gemm's -- (lo + mid) + hi per chain, chains in
// order -- so a row's result stays bit-identical whatever the batch.  All operands of a wave are in flight at once (one wave
// per SIMD: up to 512 registers).
template <int TPC, int MG>
__global__ __launch_bounds__(256) void k_downS(GemmP p) {
  __shared__ __attribute__((aligned(16))) float red[16 * 4 * MG * 4];   // [chain][row][4 columns]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, NT = p.NT, M = p.M;
  const int nt = (int)blockIdx.x % NT, part = (int)blockIdx.x / NT;
  const uint4* wt = p.W + (size_t)nt * KT * 64;
  const int row = lane & 15, k8 = lane >> 4;
  const int sa = row >> 2, r = row & 3;      // A: chain slot and weight row of this lane's row; B: chain slot and row inside its group of four
  const int piece = p.wperm ? part * 16 + k8 * 4 + r : k8 * 16 + part * 4 + r;
  const int n = nt * 16 + part * 4;
  float4 epre = make_float4(0.f, 0.f, 0.f, 0.f), egam = epre;
  if (tid < M) {
    epre = *(const float4*)((p.Yin ? p.Yin : p.Y) + (size_t)tid * (NT * 16) + n);
    egam = *(const float4*)(p.gamma_next + n);
  }
  uint4 w[TPC];
  bf16x8 b[TPC][3][MG];
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    int t = 4 * wave + sa + 16 * u;
    const bool ok = t < KT;
    t = ok ? t : KT - 1;
    w[u] = smi_ldw(wt + (size_t)t * 64 + piece);
    if (!ok) w[u] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    int t = 4 * wave + sa + 16 * u;
    t = t < KT ? t : KT - 1;
#pragma unroll
    for (int g = 0; g < MG; ++g) {
      int m = 4 * g + r;
      m = m < M ? m : M - 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) b[u][c][g] = *(const bf16x8*)(p.XS + xs_off(t, c, k8, m, M));
    }
  }
  __builtin_amdgcn_sched_barrier(0);   // every load of the wave is requested before the first MFMA's wait
  f32x4 acc[3][MG];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int g = 0; g < MG; ++g) acc[c][g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    const bf16x8 a = __builtin_bit_cast(bf16x8, w[u]);
#pragma unroll
    for (int g = 0; g < MG; ++g) {
      acc[2][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u][2][g], acc[2][g], 0, 0, 0);
      acc[1][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u][1][g], acc[1][g], 0, 0, 0);
      acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u][0][g], acc[0][g], 0, 0, 0);
    }
  }
  // D: lane (col, rg = lane >> 4) holds weight rows 0..3 of chain slot rg for column col; the slot's own columns are 4 rg .. 4 rg + 3
  if (sa == k8) {
#pragma unroll
    for (int g = 0; g < MG; ++g) {
      const f32x4 t = (acc[2][g] + acc[1][g]) + acc[0][g];   // (lo + mid) + hi
      *(float4*)(red + ((4 * wave + k8) * 4 * MG + 4 * g + r) * 4) = make_float4(t[0], t[1], t[2], t[3]);
    }
  }
  __syncthreads();
  if (tid < M) {
    const int m = tid;
    float4 sres = *(const float4*)(red + m * 4);
#pragma unroll
    for (int ch = 1; ch < 16; ++ch) {   // the 16 chains in order
      const float4 q = *(const float4*)(red + (ch * 4 * MG + m) * 4);
      sres.x += q.x; sres.y += q.y; sres.z += q.z; sres.w += q.w;
    }
    float4 h = epre;   // RESID epilogue of k_gemm for row m, columns n .. n + 3
    h.x += sres.x; h.y += sres.y; h.z += sres.z; h.w += sres.w;
    *(float4*)(p.Y + (size_t)m * (NT * 16) + n) = h;
    const float ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
    const float tv[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
    uint32_t hi[4], mi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split3(tv[e], hi[e], mi[e], lo[e]);
    const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
    const size_t pl = (size_t)4 * M * 16;
    *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
    *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
    p.ssout[((size_t)m * NT + nt) * 4 + part] = ssq;
  }
}

// ------------------------------------------------------------------------------------------
// Exact-weights verification mode (smi_llm_cfg.weights_exact = 1; round 4).  The reference loads the checkpoint as saved
// (cli/SparkTTS.py:48-51) and the published LLM/model.safetensors is fp32: the bf16 arena rounds it (logits move ~1e-2, a
// tenth of the greedy decisions of a synthetic model change).  In this mode the arena holds the matrices as fp32 [N][K]
// (same row / column orders as the bf16 tiles) and every GEMM of the path runs here: one wave per (16-row weight tile, 16-row
// m-tile), v_mfma_f32_16x16x4_f32 -- an exact fp32 fused multiply-add chain over k, like the CPU's -- on operands rebuilt
// exactly from the triples (x = hi + mid + lo), with k_gemm's own prologue scalars and epilogues (RMSNorm factor, bias, RoPE,
// KV append, residual, SwiGLU, arg-max partials, the next operand's triples).  Throughput is not a goal (a weight byte is
// read once per 16 rows through 64-byte row segments: ~1.5 ms per step at one row); north_star's acceptance sentence --
// waveform within 1e-3 of the PyTorch CPU path for fixed greedy seeds -- on an fp32-saved checkpoint is.
// ------------------------------------------------------------------------------------------
template <int PRO, int EPI, int KVF32>
__global__ __launch_bounds__(256) void k_gemm_x(GemmP p, const float* W32) {
  static_assert(EPI == EPI_QKV || KVF32 == 0, "the cache type is a parameter of the kernels that write the cache");
  __shared__ float bestv[4][16];
  __shared__ int besti[4][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, K = KT * 32, M = p.M, NT = p.NT, N = NT * 16;
  const int nt = (int)blockIdx.x * 4 + wave, mbase = (int)blockIdx.y * 16;
  const int em = lane & 15, kq = lane >> 4;
  const int m = mbase + em, mc = m < M ? m : M - 1;
  const bool live = nt < NT;                       // wave-uniform
  const int ntc = live ? nt : NT - 1;
  // ---- y[n][m] = sum_k W[n][k] x[m][k]: 16 k per step, lane (kq, i) holds W[16 nt + i][k0 + 4 kq .. + 3] and x[m = i][same k]
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* wrow = W32 + (size_t)(ntc * 16 + em) * K + 4 * kq;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const float4 wv = *(const float4*)(wrow + k0);
    const int k = k0 + 4 * kq;                     // this lane's four k: tile k >> 5, octet (k >> 3) & 3, elements k & 7 .. + 3
    const unsigned char* xp = p.XS + xs_off(k >> 5, 0, (k >> 3) & 3, mc, M) + (k & 7) * 2;
    const size_t pl = (size_t)4 * M * 16;
    const uint2 h2 = *(const uint2*)xp, m2 = *(const uint2*)(xp + pl), l2 = *(const uint2*)(xp + 2 * pl);
    const uint32_t hb[4] = {h2.x << 16, h2.x & 0xffff0000u, h2.y << 16, h2.y & 0xffff0000u};
    const uint32_t mb[4] = {m2.x << 16, m2.x & 0xffff0000u, m2.y << 16, m2.y & 0xffff0000u};
    const uint32_t lb[4] = {l2.x << 16, l2.x & 0xffff0000u, l2.y << 16, l2.y & 0xffff0000u};
    const float wa[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = (__uint_as_float(hb[c]) + __uint_as_float(mb[c])) + __uint_as_float(lb[c]);   // exact: the split terms do not overlap
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[c], x, acc, 0, 0, 0);
    }
  }
  // ---- k_gemm's epilogue for (tile nt, rows mbase ..): lane (g = lane >> 4, m) holds columns n .. n + 3 of row m
  float4 s = make_float4(acc[0], acc[1], acc[2], acc[3]);
  const int n = ntc * 16 + 4 * (lane >> 4);
  const bool valid = live && m < M;
  if (PRO == PRO_NORM) {
    // every lane needs ITS row's factor: rows differ across the 16 lanes of a group, so each row is summed by the whole wave in turn
    float r = 0.f;
    for (int j = 0; j < 16; ++j) {
      const int mj = mbase + j < M ? mbase + j : M - 1;
      float vj = smi_ss_lane_sum(p.sspart + (size_t)mj * p.npart, p.npart, lane);
      vj = smi_wave_sum(vj);
      const float rj = 1.0f / sqrtf(vj / (float)K + p.eps);
      r = em == j ? rj : r;
    }
    s.x *= r; s.y *= r; s.z *= r; s.w *= r;
  }
  if (EPI == EPI_RESID) {
    if (valid) {
      const float4 egam = *(const float4*)(p.gamma_next + n);
      float4 h = *(const float4*)((p.Yin ? p.Yin : p.Y) + (size_t)m * N + n);
      h.x += s.x; h.y += s.y; h.z += s.z; h.w += s.w;
      *(float4*)(p.Y + (size_t)m * N + n) = h;
      const float ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
      const float t[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
      uint32_t hi[4], mi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split3(t[e], hi[e], mi[e], lo[e]);
      const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
      const size_t pl = (size_t)4 * M * 16;
      *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
      *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
      *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
      p.ssout[((size_t)m * NT + nt) * 4 + (lane >> 4)] = ssq;
    }
  } else if (EPI == EPI_SWIGLU) {
    if (valid) {
      const float a0 = (s.x / (1.0f + expf(-s.x))) * s.y;
      const float a1 = (s.z / (1.0f + expf(-s.z))) * s.w;
      uint32_t h0, m0, l0, h1, m1, l1;
      split3(a0, h0, m0, l0);
      split3(a1, h1, m1, l1);
      const int k = n >> 1;
      const size_t o = xs_off(k >> 5, 0, (k >> 3) & 3, m, M) + ((k >> 1) & 3) * 4;
      const size_t pl = (size_t)4 * M * 16;
      *(uint32_t*)(p.XSout + o) = h0 | (h1 << 16);
      *(uint32_t*)(p.XSout + o + pl) = m0 | (m1 << 16);
      *(uint32_t*)(p.XSout + o + 2 * pl) = l0 | (l1 << 16);
    }
  } else if (EPI == EPI_QKV) {
    if (valid) {
      const float4 b = *(const float4*)(p.bias + n);
      s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
      const RowDesc rd = p.rows[m];
      if (n < p.q_dim + p.kv_dim) {
        const int i0 = (n & 63) >> 1;
        const float2 c0 = p.rope[(size_t)rd.pos * 32 + i0], c1 = p.rope[(size_t)rd.pos * 32 + i0 + 1];
        float4 r;
        r.x = __fadd_rn(__fmul_rn(s.x, c0.x), __fmul_rn(-s.y, c0.y));
        r.y = __fadd_rn(__fmul_rn(s.y, c0.x), __fmul_rn(s.x, c0.y));
        r.z = __fadd_rn(__fmul_rn(s.z, c1.x), __fmul_rn(-s.w, c1.y));
        r.w = __fadd_rn(__fmul_rn(s.w, c1.x), __fmul_rn(s.z, c1.y));
        s = r;
      }
      if (n < p.q_dim) {
        *(float4*)(p.Y + (size_t)m * p.q_dim + n) = s;
      } else {
        const bool isk = n < p.q_dim + p.kv_dim;
        const int c = n - p.q_dim - (isk ? 0 : p.kv_dim);
        const size_t off = kv_row(p.km, rd.slot, c >> 6, p.n_kv, p.max_pos, rd.pos) * 64 + (c & 63);
        void* base = isk ? p.kcache : p.vcache;
        if (KVF32) {
          *(float4*)((float*)base + off) = s;
        } else {
          uint2 pk;
          pk.x = smi_f32_to_bf16(s.x) | (smi_f32_to_bf16(s.y) << 16);
          pk.y = smi_f32_to_bf16(s.z) | (smi_f32_to_bf16(s.w) << 16);
          *(uint2*)((uint16_t*)base + off) = pk;
        }
      }
    }
  } else {  // EPI_LM
    if (valid && p.Y) {
      float* y = p.Y + (size_t)m * p.V + n;
      if (n + 0 < p.V) y[0] = s.x;
      if (n + 1 < p.V) y[1] = s.y;
      if (n + 2 < p.V) y[2] = s.z;
      if (n + 3 < p.V) y[3] = s.w;
    }
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (live && n + r < p.V && sv[r] > bv) { bv = sv[r]; bi = n + r; }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane < 16) { bestv[wave][lane] = bv; besti[wave][lane] = bi; }
    __syncthreads();
    if (tid < 16 && mbase + tid < M) {
      bv = bestv[0][tid]; bi = besti[0][tid];
#pragma unroll
      for (int w2 = 1; w2 < 4; ++w2) {
        const float ov = bestv[w2][tid];
        const int oi = besti[w2][tid];
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      p.pval[(size_t)(mbase + tid) * gridDim.x + blockIdx.x] = bv;
      p.pidx[(size_t)(mbase + tid) * gridDim.x + blockIdx.x] = bi;
    }
  }
}

// the embedding row of `token` from the fp32 lm_head of the exact-weights arena ([vocab padded][K] row-major): h, the first
// norm's operand triples and the row's sum of squares, as embed_row leaves them
__device__ __forceinline__ void embed_row_x(const float* W32, int KT, int token, int m, int M, const float* gamma,
                                            float* h, unsigned char* xs, float* sspart, int npart, int lane) {
  const int K = KT * 32;
  float ss = 0.f;
  for (int pc = lane; pc < KT * 4; pc += 64) {
    const float4 a = *(const float4*)(W32 + (size_t)token * K + pc * 8), b = *(const float4*)(W32 + (size_t)token * K + pc * 8 + 4);
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float* dst = h + (size_t)m * K + pc * 8;
    *(float4*)dst = a;
    *(float4*)(dst + 4) = b;
    const float4 g0 = *(const float4*)(gamma + pc * 8), g1 = *(const float4*)(gamma + pc * 8 + 4);
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    uint32_t hi[8], mi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ss += x[e] * x[e]; split3(g[e] * x[e], hi[e], mi[e], lo[e]); }
    const size_t o = xs_off(pc >> 2, 0, pc & 3, m, M);
    const size_t pl = (size_t)4 * M * 16;
    *(uint4*)(xs + o) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
    *(uint4*)(xs + o + pl) = make_uint4(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16), mi[4] | (mi[5] << 16), mi[6] | (mi[7] << 16));
    *(uint4*)(xs + o + 2 * pl) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
  }
  ss = smi_wave_sum(ss);
  for (int i = lane; i < npart; i += 64) sspart[(size_t)m * npart + i] = i == 0 ? ss : 0.f;
}

// ------------------------------------------------------------------------------------------
// down_proj at 9 .. 64 rows: the 16 chains go to 16 DIFFERENT blocks (round 4).
// k_gemm<.., H> gives a block all 16 chains of its rows of a weight tile, so every block pulls the WHOLE operand of its 16 rows
// (K = 4864: 467 KB of triples per block at 32 rows, 105 MB of L2 -> CU traffic per launch: its loads land 5.6 us after the
// first wave starts, profiles/r03_stamps_batch.txt) and the two 16-row block rows both stream the weights from HBM (16.6 MB for
// 8.7 MB, r03_pmc_traffic_g_b32.json).  Here block (column group cg, chain c) takes chain c's k tiles (kt = c, c + 16, ...) of
// four weight tiles for ALL rows: 40 KB of weights (every weight byte leaves HBM once per launch) and 1/16 of the operand
// (61 KB at 32 rows), staged once per block in LDS.  A wave owns one weight tile -- no cross-wave reduction -- and leaves the
// chain's sum, (lo + mid) + hi exactly as k_gemm forms it, in `part` [chain][n tile][m tile][lane] (the accumulator's own
// layout: 1-KiB stores).  k_resid_comb then adds the 16 chains IN ORDER and runs the RESID epilogue: the same sums in the same
// order as k_gemm<RESID, NW = 16> / k_downS / k_down1, so a row keeps its bits whatever the batch.  Blocks of one chain sit on
// one XCD (block id = cg * 16 + c): they share the operand slice through one L2.
// ------------------------------------------------------------------------------------------
struct DownCP {
  const uint4* W; int NT, KT, M, wperm;
  const unsigned char* XS;          // act triples [KT][3][4][M][16 B]
  float4* part;                     // [16][NT][MTN][64]
  // combine
  float* Y; const float* Yin; const float* gamma_next; unsigned char* XSout; float* ssout;
};

template <int TPC, int MTN>
__global__ __launch_bounds__(256) void k_downC(DownCP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [tiles of the chain][12 * M] 16-byte operand pieces
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, M = p.M, NT = p.NT;
  const int c = (int)blockIdx.x & 15, cg = (int)blockIdx.x >> 4;
  const int ntile = c < KT ? (KT - c + 15) >> 4 : 0;    // k tiles of this chain
  if (ntile == 0) {   // block-uniform: fewer than 16 k tiles -- this chain adds zeros, as an idle wave of k_gemm does
    const int nt0 = cg * 4 + (tid >> 6);
    if (nt0 < NT)
      for (int mt = 0; mt < MTN; ++mt) p.part[(((size_t)c * NT + nt0) * MTN + mt) * 64 + (tid & 63)] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int pm = 12 * M, npieces = ntile * pm;
  const float pm_inv = 1.0f / (float)pm;
  // ---- operand slice: every piece requested before the weights (L2 hits; loads return in issue order)
  constexpr int PPT = (TPC * 12 * MTN * 16 + 255) / 256; // pieces per thread at most
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 pc[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    int q = tid + 256 * i;
    q = q < npieces ? q : npieces - 1;
    const int u = (int)(((float)q + 0.5f) * pm_inv), r = q - u * pm;   // q / pm, exact: q < 2^13, (q + 0.5) / pm is never within 6e-4 of an integer
    pc[i] = *(const u32x4*)(p.XS + ((size_t)(c + 16 * u) * pm + r) * 16);
  }
  // ---- this wave's weight tile, chain c's k tiles: full 1-KiB loads, all in flight
  const int nt = cg * 4 + wave;
  const int ntc = nt < NT ? nt : NT - 1;
  const int wl = smi_wlane(lane, p.wperm);
  uint4 w[TPC];
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    const int t = c + 16 * u;
    w[u] = smi_ldw(p.W + ((size_t)ntc * KT + (t < KT ? t : KT - 1)) * 64 + wl);
  }
#pragma unroll
  for (int i = 0; i < PPT; ++i) asm volatile("" : "+v"(pc[i]));   // the loads above stay above (not sunk into the guarded stores)
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int q = tid + 256 * i;
    if (q < npieces) *(u32x4*)(smem + (size_t)q * 16) = pc[i];
  }
  __syncthreads();
  f32x4 acc[3][MTN];
#pragma unroll
  for (int s2 = 0; s2 < 3; ++s2)
#pragma unroll
    for (int mt = 0; mt < MTN; ++mt) acc[s2][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int k8 = lane >> 4, em = lane & 15;
#pragma unroll
  for (int u = 0; u < TPC; ++u) {
    if (u < ntile) {   // block-uniform
      const bf16x8 a = __builtin_bit_cast(bf16x8, w[u]);
#pragma unroll
      for (int mt = 0; mt < MTN; ++mt) {
        int m = mt * 16 + em;
        m = m < M ? m : M - 1;
        const unsigned char* bp = smem + ((size_t)u * pm + (size_t)k8 * M + m) * 16;
        const bf16x8 b0 = *(const bf16x8*)bp, b1 = *(const bf16x8*)(bp + (size_t)4 * M * 16), b2 = *(const bf16x8*)(bp + (size_t)8 * M * 16);
        acc[2][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b2, acc[2][mt], 0, 0, 0);
        acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[1][mt], 0, 0, 0);
        acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[0][mt], 0, 0, 0);
      }
    }
  }
  if (nt < NT) {
#pragma unroll
    for (int mt = 0; mt < MTN; ++mt) {
      const f32x4 t = (acc[2][mt] + acc[1][mt]) + acc[0][mt];   // (lo + mid) + hi
      p.part[(((size_t)c * NT + nt) * MTN + mt) * 64 + lane] = make_float4(t[0], t[1], t[2], t[3]);
    }
  }
}

// One wave per (n tile, m tile): the S partial sums in order, then the RESID epilogue (residual add, h, the next norm's operand
// triples and partial sums of squares).  Two producers: k_downC (S = 16 chains; the running sum starts from chain 0's term, as
// k_gemm's cross-wave reduction does; one partial sum of squares per 4 columns) and k_pgemm's split-K form (S segments; ZI: the
// running sum starts from zero, as its in-block fold does; SSTILE: one partial per n tile, combined across the lanes exactly
// as k_pgemm's epilogue combines them) -- in both cases the same sums in the same order as the single-launch form.
template <int ZI, int SSTILE>
__global__ __launch_bounds__(64) void k_resid_comb(DownCP p, int S, int MTN) {
  const int lane = threadIdx.x, unit = (int)blockIdx.x;
  const int nt = unit / MTN, mt = unit - nt * MTN;
  const int NT = p.NT, M = p.M, N = NT * 16;
  const int m = mt * 16 + (lane & 15), n = nt * 16 + 4 * (lane >> 4);
  const bool valid = m < M;
  const int mc = valid ? m : M - 1;
  const float4 egam = *(const float4*)(p.gamma_next + n);
  const float4 epre = *(const float4*)((p.Yin ? p.Yin : p.Y) + (size_t)mc * N + n);
  float4 q[16];
#pragma unroll
  for (int ch = 0; ch < 16; ++ch) q[ch] = p.part[(((size_t)(ch < S ? ch : S - 1) * NT + nt) * MTN + mt) * 64 + lane];
  float4 s = ZI ? make_float4(0.f, 0.f, 0.f, 0.f) : q[0];
#pragma unroll
  for (int ch = ZI ? 0 : 1; ch < 16; ++ch)
    if (ch < S) { s.x += q[ch].x; s.y += q[ch].y; s.z += q[ch].z; s.w += q[ch].w; }   // wave-uniform
  float ssq = 0.f;
  if (valid) {
    float4 h = epre;
    h.x += s.x; h.y += s.y; h.z += s.z; h.w += s.w;
    *(float4*)(p.Y + (size_t)m * N + n) = h;
    ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
    const float t[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
    uint32_t hi[4], mi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split3(t[e], hi[e], mi[e], lo[e]);
    const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
    const size_t pl = (size_t)4 * M * 16;
    *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
    *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
  }
  if (SSTILE) {   // k_pgemm's epilogue: the tile's four column groups of a row added across the lanes, one partial per (row, n tile)
    ssq += __shfl_xor(ssq, 16, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    if (lane < 16 && valid) p.ssout[(size_t)m * NT + nt] = ssq;
  } else if (valid) {
    p.ssout[((size_t)m * NT + nt) * 4 + (lane >> 4)] = ssq;
  }
}

// ------------------------------------------------------------------------------------------
// Prefill GEMM: many rows (a whole batch of prompts) against one weight matrix, no split-K.
// Block = 4 waves = 8 weight tiles (128 output columns) x 128 rows; each wave owns 2 weight tiles
// (A operands straight from HBM, used for all 8 m-tiles) and the block shares the rows' operand
// triples through a double-buffered LDS image (24 KB per k tile), so a weight tile is read once per
// 128 rows and an operand piece once per 128 output columns.  One accumulator per (tile, m-tile),
// terms in the order lo, mid, hi per k tile: a row's result does not depend on M or on the batch.
// ------------------------------------------------------------------------------------------
// WR = 2: the waves form a 2 x 2 grid (row half x column half) -- a wave reads only its 64 rows' pieces from LDS (half the LDS
// bytes per MFMA of WR = 1, where every wave reads all 128 rows) and each weight tile is requested by the two waves of a column half.
// One LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global addresses to LDS bytes [lds_dst + 16 * lane) (lds_dst
// wave-uniform).  Inline asm, M0 written in the statement that reads it: hipcc waits vmcnt(0) in front of every ds_read while an
// LDS-DMA it knows of (the builtin) is pending; these it does not see, the counted waits are written by hand.
__device__ __forceinline__ void smi_glds16(const void* gsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

__device__ __forceinline__ void smi_keep4(const uint4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }   // (ablation builds: keeps a value live)

// RING >= 3: both operands of a k tile arrive by LDS-DMA (global_load_lds_dwordx4, no staging registers) in a ring of RING slots,
// RING - 1 tiles requested ahead of the one being multiplied; a counted vmcnt + one raw barrier per k tile (the loads of the
// tiles ahead stay in flight across it).  The register-staged form (RING = 0) waits a whole L2 / HBM round trip per k tile.
// XMAP (few column blocks per row block: QKV, o_proj, down): the launch is one-dimensional and a block's (column, row)
// block comes from its position in its XCD's share of the grid (blocks go to XCD id mod 8), so that the column blocks of a row
// block run on one XCD side by side: an operand piece then comes from the Infinity Cache once and from that XCD's L2 for the
// others (as launched, x fastest, the 6-7 column blocks of a row block sat on 6-7 different XCDs and every operand byte
// was served at the Infinity-Cache rate: down_proj 7.3 TB/s of L2 -> LDS traffic; a workgroup reads ~33 GB/s from there, ~70 from L2).
// TWO (RING = 2): two blocks per CU -- 80 KiB of LDS and at most 256 registers each -- instead of one with a deeper ring: one
// block's prologue, epilogue and barrier stalls are covered by the other's MFMAs (gate_up: 2432 blocks of 128 x 256 in 9.5 rounds,
// 10 us of un-overlapped prologue + epilogue per round at one block per CU).  One fragment set, the ring's other slot one k
// tile ahead, and the RMSNorm factors are computed after the k loop into the ring's memory (no LDS left for them beside it).
// MTB (ring form only): m-tiles per block, 8 (128 rows) or 4 (64 rows: the few-row shapes -- twice the blocks for a 127-row prompt).
template <int PRO, int EPI, int KVF32, int NTW = 2, int WR = 1, int RING = 0, int XMAP = 0, int TWO = 0, int MTB = 8>
__global__ __launch_bounds__(256, TWO ? 2 : 1) void k_pgemm(GemmP p) {
  static_assert(EPI == EPI_QKV || KVF32 == 0, "the cache type is a parameter of the kernels that write the cache");
  static_assert(MTB == 8 || (MTB == 4 && RING >= 3 && !TWO), "64-row tiles: ring form");
  constexpr int ROWS = MTB * 16, PIECES = 3 * 4 * ROWS;   // 1536 (768) 16-byte pieces per k tile; NTW weight tiles per wave
  constexpr int MTW = MTB / WR, NWC = 4 / WR;                      // m-tiles per wave, waves across the block's columns
  constexpr int CT = NWC * NTW;                                    // weight tiles per block
  constexpr int SLOT = PIECES + CT * 64;                           // RING: 16-byte pieces per ring slot (operand image, then weight tiles)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* Bs = (uint4*)smem;                              // [2][PIECES], or [RING][SLOT]
  float* rarr = TWO ? (float*)smem : (float*)(smem + (size_t)(RING ? RING * SLOT : 2 * PIECES) * 16);  // [ROWS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, M = p.M, NT = p.NT;
  int bx = blockIdx.x, by = blockIdx.y;
  if constexpr (XMAP) {   // bijective for any grid size: XCD c owns a contiguous range of (row block, column block) pairs, column fastest
    const int gx = (NT + CT - 1) / CT, nb = gridDim.x, q = nb >> 3, r = nb & 7, c = bx & 7;
    const int v = (c < r ? c * (q + 1) : r * (q + 1) + (c - r) * q) + (bx >> 3);
    by = v / gx;
    bx = v - by * gx;
  }
  const int m0 = by * ROWS;
  const int k8 = lane >> 4, em = lane & 15;
  const int wr = wave % WR, wc = wave / WR, mt0 = wr * MTW;
  int nts[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i) { const int nt = (bx * NWC + wc) * NTW + i; nts[i] = nt < NT ? nt : NT - 1; }

  f32x4 acc[NTW][MTW];
#pragma unroll
  for (int a = 0; a < NTW; ++a)
#pragma unroll
    for (int b = 0; b < MTW; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // K segments (RESID, ring form): in-block -- `tot` takes each finished segment's sum, in order; split-K -- this block sums
  // segment blockIdx.y only and leaves it in p.slab
  constexpr bool SEG = EPI == EPI_RESID && RING >= 3 && !TWO && XMAP;
  const int kseg = SEG ? p.kseg : 0;
  const bool part = SEG && p.slab != nullptr;
  const int k_lo = part ? (int)blockIdx.y * kseg : 0;
  const int k_hi = part ? (k_lo + kseg < KT ? k_lo + kseg : KT) : KT;
  f32x4 tot[SEG ? NTW : 1][SEG ? MTW : 1];
  if constexpr (SEG) {
#pragma unroll
    for (int a = 0; a < NTW; ++a)
#pragma unroll
      for (int b = 0; b < MTW; ++b) tot[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  auto fold = [&]() {   // a segment is complete: total += segment sum (0 + s0, then + s1, ...: the order k_resid_comb adds the slab in)
    if constexpr (SEG) {
#pragma unroll
      for (int a = 0; a < NTW; ++a)
#pragma unroll
        for (int b = 0; b < MTW; ++b) { tot[a][b] = tot[a][b] + acc[a][b]; acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    }
  };
  if constexpr (RING != 0) {
    static_assert((TWO ? RING == 2 : RING >= 3) && CT % 4 == 0, "ring form: a wave-instruction moves one weight tile, four per pass of the block");
    constexpr int NI = PIECES / 256, PPI = 256 / ROWS;   // operand issues per thread and k tile; (split, octet) planes one issue covers
    constexpr int GA = CT / 4, G = NI + GA;              // LDS-DMA instructions per thread and k tile
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t lbase = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lptr_t)smem);
    int brow = m0 + (tid & (ROWS - 1));
    brow = brow < M ? brow : M - 1;
    const unsigned char* bsrc = p.XS + ((size_t)(tid / ROWS) * M + brow) * 16;   // issue i of k tile kt: + ((kt * 12 + PPI i) * M) * 16
    const uint4* asrc[GA];
#pragma unroll
    for (int a = 0; a < GA; ++a) {
      const int nt = bx * CT + 4 * a + wv;
      asrc[a] = p.W + (size_t)(nt < NT ? nt : NT - 1) * KT * 64 + smi_wlane(lane, p.wperm);
    }
    auto issue = [&](int kt, int slot) {                 // tile kt (clamped: the extra requests of the last iterations keep the count uniform) -> ring slot
      const int kc = kt < k_hi ? kt : k_hi - 1;
      const uint32_t d = lbase + (uint32_t)(slot * SLOT + wv * 64) * 16;
#pragma unroll
      for (int i = 0; i < NI; ++i) smi_glds16(bsrc + ((size_t)(kc * 12 + PPI * i) * M) * 16, d + 256 * 16 * i);
#pragma unroll
      for (int a = 0; a < GA; ++a) smi_glds16(asrc[a] + (size_t)kc * 64, d + (uint32_t)(PIECES + 4 * a * 64) * 16);
    };
#pragma unroll
    for (int t = 0; t < RING - 1; ++t) issue(k_lo + t, t);
    // RMSNorm factors of the block's rows.  A wave takes 32 rows with all their loads in flight together (one row after the
    // other: 32 dependent L2 round trips, ~50 us in front of the k loop); per row the order of smi_ss_lane_sum + smi_wave_sum.
    constexpr int RPN = ROWS / 4;                       // rows whose factor a wave computes
    auto norm_factors = [&]() {
      const int np = p.npart, last = np - 1;
      if (np <= 64) {                                     // (the prefill GEMM's own RESID epilogue: one partial per n tile)
        float a[RPN];
        const int i0 = lane < np ? lane : last;
#pragma unroll
        for (int j = 0; j < RPN; ++j) {
          int m = m0 + wave * RPN + j;
          m = m < M ? m : M - 1;
          a[j] = p.sspart[(size_t)m * np + i0];
        }
#pragma unroll
        for (int j = 0; j < RPN; ++j) {
          float v = 0.f;
          v += lane < np ? a[j] : 0.f;
          v = smi_wave_sum(v);
          if (lane == 0) rarr[wave * RPN + j] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
        }
      } else if (np <= 256) {
        int idx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) idx[q] = lane + 64 * q < np ? lane + 64 * q : last;
        for (int r0 = wave * RPN; r0 < wave * RPN + RPN; r0 += 8) {
          float a[8][4];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int m = m0 + r0 + j;
            m = m < M ? m : M - 1;
            const float* sp = p.sspart + (size_t)m * np;
#pragma unroll
            for (int q = 0; q < 4; ++q) a[j][q] = sp[idx[q]];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) v += lane + 64 * q < np ? a[j][q] : 0.f;
            v = smi_wave_sum(v);
            if (lane == 0) rarr[r0 + j] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
          }
        }
      } else {
        for (int r = wave * RPN; r < wave * RPN + RPN; ++r) {
          int m = m0 + r;
          m = m < M ? m : M - 1;
          float v = smi_ss_lane_sum(p.sspart + (size_t)m * np, np, lane);
          v = smi_wave_sum(v);
          if (lane == 0) rarr[r] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
        }
      }
    };
    if (PRO == PRO_NORM && !TWO) norm_factors();
    // Fragment registers of two k tiles: tile kt + 1's are read from LDS while tile kt's feed the MFMAs (every wave of the block
    // reads at the same time -- right behind the barrier -- so without the second set the LDS phase and the MFMA phase of
    // an iteration add up instead of overlapping: measured 2060 cycles per k tile for 768 of MFMAs).
    struct Frag { uint4 a[NTW]; uint4 b[MTW][3]; };
    Frag f0, f1;
    auto fread = [&](Frag& f, int slot) {
      const uint4* Bb = Bs + (size_t)slot * SLOT;
#pragma unroll
      for (int i = 0; i < NTW; ++i) f.a[i] = Bb[PIECES + (wc * NTW + i) * 64 + lane];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int s = 0; s < 3; ++s) f.b[mt][s] = Bb[(s * 4 + k8) * ROWS + (mt0 + mt) * 16 + em];
    };
    auto fmma = [&](const Frag& f) {
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        const bf16x8 b0 = __builtin_bit_cast(bf16x8, f.b[mt][0]), b1 = __builtin_bit_cast(bf16x8, f.b[mt][1]), b2 = __builtin_bit_cast(bf16x8, f.b[mt][2]);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, f.a[i]);
          acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b2, acc[i][mt], 0, 0, 0);
          acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[i][mt], 0, 0, 0);
          acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[i][mt], 0, 0, 0);
        }
      }
    };
    // Iteration kt: read tile kt + 1's fragments (slot rn: landed before the last barrier), request tile kt + RING - 1 into
    // the slot of tile kt - 1 (its reads were waited for before the last barrier), multiply tile kt.  Then: this thread's
    // part of tile kt + 2 has landed (counted vmcnt: the RING - 3 tiles behind it stay in flight across the raw barrier; a
    // __syncthreads would drain them), this wave's LDS reads are done (lgkmcnt(0)), barrier.
#define SMI_PG_SYNC() asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((RING - 3) * G) : "memory")
#ifndef SMI_PG_ABL
#define SMI_PG_ABL 0   // timing-only builds (tools/pg_ablate.sh): 1 no MFMAs, 2 no LDS-DMA in the loop, 4 no epilogue, 8 no fragment reads
#endif
#define SMI_PG_STEP(cur_, nxt_, kt_) do { \
      if (!(SMI_PG_ABL & 8)) fread(nxt_, rn); \
      if (!(SMI_PG_ABL & 2)) issue((kt_) + RING - 1, ws); \
      if (!(SMI_PG_ABL & 1)) fmma(cur_); else { _Pragma("unroll") for (int i_ = 0; i_ < NTW; ++i_) smi_keep4((cur_).a[i_]); _Pragma("unroll") for (int m_ = 0; m_ < MTW; ++m_) { smi_keep4((cur_).b[m_][0]); smi_keep4((cur_).b[m_][1]); smi_keep4((cur_).b[m_][2]); } } \
      if (SEG && !part && kseg > 0 && ((kt_) + 1) % kseg == 0) fold();   /* (block-uniform) a segment ends with this tile */ \
      SMI_PG_SYNC(); \
      rn = rn + 1 == RING ? 0 : rn + 1; \
      ws = ws + 1 == RING ? 0 : ws + 1; \
    } while (0)
    if (SMI_PG_ABL & 8) { f0 = Frag{}; f1 = Frag{}; }
    if constexpr (TWO) {
      // tile kt from slot kt & 1 while tile kt + 1 arrives in the other slot (free: its reads were waited for before the last barrier)
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");     // tile 0
      for (int kt = 0; kt < KT; ++kt) {
        issue(kt + 1, (kt + 1) & 1);
        fread(f0, kt & 1);
        fmma(f0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      if (PRO == PRO_NORM) {                               // the ring is idle now (every request landed, every read done): its memory takes the factors
        norm_factors();
        __syncthreads();
      }
    } else {
    SMI_PG_SYNC();                                        // tiles 0 and 1 (rarr: the fence below)
    __syncthreads();
    fread(f0, 0);
    int rn = 1, ws = RING - 1;
    for (int kt = k_lo; kt < k_hi; kt += 2) {
      SMI_PG_STEP(f0, f1, kt);
      if (kt + 1 < k_hi) SMI_PG_STEP(f1, f0, kt + 1);
      else f0 = f1;                                       // (odd count: the loop ends here; keeps the two paths' live sets alike)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the clamped extra requests: nothing may still write LDS when the block ends
    if constexpr (SEG) {
      if (!part && kseg > 0) {
        if (KT % kseg) fold();                            // the last, shorter segment
#pragma unroll
        for (int a = 0; a < NTW; ++a)
#pragma unroll
          for (int b = 0; b < MTW; ++b) acc[a][b] = tot[a][b];
      }
    }
    }
#undef SMI_PG_STEP
#undef SMI_PG_SYNC
  } else {
  // The six staged pieces are named registers, not an array: as `uint4 sreg[6]` the compiler left them in scratch
  // memory (ScratchSize 112), which put a wait for the global loads right behind their issue -- in front of the k
  // tile's MFMAs instead of behind them.
  static_assert(PIECES / 256 == 6, "six staged pieces per thread");
  uint4 sr0, sr1, sr2, sr3, sr4, sr5;
  auto piece = [&](int kt, int i) -> uint4 {
    const int q = tid + 256 * i;                         // [s][k8][row]
    int row = m0 + (q & (ROWS - 1));
    row = row < M ? row : M - 1;
    return *(const uint4*)(p.XS + xs_off(kt, q / (4 * ROWS), (q / ROWS) & 3, row, M));
  };
#define stage_load(kt_) do { sr0 = piece((kt_), 0); sr1 = piece((kt_), 1); sr2 = piece((kt_), 2); sr3 = piece((kt_), 3); sr4 = piece((kt_), 4); sr5 = piece((kt_), 5); } while (0)
#define stage_store(buf_) do { uint4* d_ = Bs + (buf_) * PIECES + tid; d_[0] = sr0; d_[256] = sr1; d_[512] = sr2; d_[768] = sr3; d_[1024] = sr4; d_[1280] = sr5; } while (0)
  stage_load(0);
  if (PRO == PRO_NORM) {
    for (int r = wave; r < ROWS; r += 4) {
      int m = m0 + r;
      m = m < M ? m : M - 1;
      float v = smi_ss_lane_sum(p.sspart + (size_t)m * p.npart, p.npart, lane);
      v = smi_wave_sum(v);
      if (lane == 0) rarr[r] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
    }
  }
  stage_store(0);
  __syncthreads();
  // Weight tiles run two k tiles ahead of the MFMAs (HBM / L2 latency hidden behind 96 MFMAs per wave).  Three
  // register sets take the roles (in use, next, in flight) in turn -- the k loop is unrolled by three so that no
  // set is ever copied: with `wA = wB; wB = wC` at the loop end the compiler waited for the loads it had just issued.
  uint4 w0[NTW], w1[NTW], w2[NTW];
  const int wl_ = smi_wlane(lane, p.wperm);
#define wload(w_, kt_) do { const int kc_ = (kt_) < KT ? (kt_) : KT - 1; _Pragma("unroll") for (int i = 0; i < NTW; ++i) (w_)[i] = p.W[((size_t)nts[i] * KT + kc_) * 64 + wl_]; } while (0)
#define ktile(kt_, wuse_, wld_) do { \
    const int kq_ = (kt_); \
    wload(wld_, kq_ + 2); \
    stage_load(kq_ + 1 < KT ? kq_ + 1 : KT - 1);         /* in flight during this tile's MFMAs: unconditional (behind a branch the compiler waited for them in front of the MFMAs) and fenced (without the fence it sinks them below the MFMAs) */ \
    __builtin_amdgcn_sched_barrier(0); \
    const uint4* Bb = Bs + (kq_ & 1) * PIECES; \
    /* operand pieces of m-tile mt + 1 are read from LDS while the MFMAs of m-tile mt run */ \
    uint4 bq[2][3]; \
    _Pragma("unroll") for (int s = 0; s < 3; ++s) bq[0][s] = Bb[(s * 4 + k8) * ROWS + mt0 * 16 + em]; \
    _Pragma("unroll") for (int mt = 0; mt < MTW; ++mt) { \
      if (mt + 1 < MTW) { \
        _Pragma("unroll") for (int s = 0; s < 3; ++s) bq[(mt + 1) & 1][s] = Bb[(s * 4 + k8) * ROWS + (mt0 + mt + 1) * 16 + em]; \
      } \
      const bf16x8 b0 = __builtin_bit_cast(bf16x8, bq[mt & 1][0]), b1 = __builtin_bit_cast(bf16x8, bq[mt & 1][1]), \
                   b2 = __builtin_bit_cast(bf16x8, bq[mt & 1][2]); \
      _Pragma("unroll") for (int i = 0; i < NTW; ++i) { \
        const bf16x8 a = __builtin_bit_cast(bf16x8, (wuse_)[i]); \
        acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b2, acc[i][mt], 0, 0, 0); \
        acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[i][mt], 0, 0, 0); \
        acc[i][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[i][mt], 0, 0, 0); \
      } \
    } \
    if (kq_ + 1 < KT) { \
      stage_store((kq_ & 1) ^ 1);                        /* the other buffer was last read two barriers ago */ \
      __syncthreads(); \
    } \
  } while (0)
  wload(w0, 0);
  wload(w1, 1);
  for (int kt = 0; kt < KT; kt += 3) {
    ktile(kt, w0, w2);
    if (kt + 1 < KT) ktile(kt + 1, w1, w0);
    if (kt + 2 < KT) ktile(kt + 2, w2, w1);
  }
#undef ktile
#undef wload
#undef stage_load
#undef stage_store
  }   // RING == 0
#ifdef SMI_PG_ABL
  if (RING != 0 && (SMI_PG_ABL & 4)) {
#pragma unroll
    for (int i = 0; i < NTW; ++i)
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) asm volatile("" ::"v"(acc[i][mt]));
    return;
  }
#endif
  if constexpr (SEG) {
    if (part) {   // split-K form: this segment's sums as they lie in the accumulators (1-KiB stores); k_resid_comb finishes the rows
#pragma unroll
      for (int i = 0; i < NTW; ++i) {
        const int nt = (bx * NWC + wc) * NTW + i;
        if (nt >= NT) continue;   // wave-uniform
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
          const int mtile = (m0 >> 4) + mt0 + mt;
          if (mtile < p.slab_mt)
            p.slab[(((size_t)blockIdx.y * NT + nt) * p.slab_mt + mtile) * 64 + lane] = make_float4(acc[i][mt][0], acc[i][mt][1], acc[i][mt][2], acc[i][mt][3]);
        }
      }
      return;
    }
  }
  // ---- epilogue (same arithmetic as k_gemm's).  Its loads first, all together and from clamped addresses: written inside the
  // `if (valid)` bodies hipcc branched around every load and waited for it on the spot (QKV: 137 `s_waitcnt vmcnt(0)`, three
  // dependent round trips -- bias, row descriptor, RoPE pair -- for each of the 24 (tile, m-tile) pairs of a wave).
  const int N = NT * 16;
  int mrow[MTW];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) { const int m = m0 + (mt0 + mt) * 16 + em; mrow[mt] = m < M ? m : M - 1; }
  int ncol[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i) { const int nt = (bx * NWC + wc) * NTW + i; ncol[i] = (nt < NT ? nt : NT - 1) * 16 + 4 * (lane >> 4); }
  float4 pre_h[EPI == EPI_RESID ? NTW : 1][EPI == EPI_RESID ? MTW : 1], pre_g[EPI != EPI_SWIGLU ? NTW : 1];
  RowDesc pre_rd[EPI == EPI_QKV ? MTW : 1];
  float2 pre_c[EPI == EPI_QKV ? NTW : 1][EPI == EPI_QKV ? MTW : 1][2];
  if constexpr (EPI == EPI_RESID) {
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
      pre_g[i] = *(const float4*)(p.gamma_next + ncol[i]);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) pre_h[i][mt] = *(const float4*)(p.Y + (size_t)mrow[mt] * N + ncol[i]);
    }
  } else if constexpr (EPI == EPI_QKV) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) pre_rd[mt] = p.rows[mrow[mt]];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
      pre_g[i] = *(const float4*)(p.bias + ncol[i]);
      const int i0 = (ncol[i] & 63) >> 1;
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        pre_c[i][mt][0] = p.rope[(size_t)pre_rd[mt].pos * 32 + i0];
        pre_c[i][mt][1] = p.rope[(size_t)pre_rd[mt].pos * 32 + i0 + 1];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int nt = (bx * NWC + wc) * NTW + i;
    if (nt >= NT) continue;   // wave-uniform
    const int n = nt * 16 + 4 * (lane >> 4);
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      const int m = m0 + (mt0 + mt) * 16 + em;
      const bool valid = m < M;
      float4 s = make_float4(acc[i][mt][0], acc[i][mt][1], acc[i][mt][2], acc[i][mt][3]);
      if (PRO == PRO_NORM) {
        const float r = rarr[(mt0 + mt) * 16 + em];
        s.x *= r; s.y *= r; s.z *= r; s.w *= r;
      }
      if (EPI == EPI_RESID) {
        float ssq = 0.f;
        if (valid) {
          float4 h = pre_h[i][mt];
          h.x += s.x; h.y += s.y; h.z += s.z; h.w += s.w;
          *(float4*)(p.Y + (size_t)m * N + n) = h;
          ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
          const float4 g = pre_g[i];
          const float t[4] = {g.x * h.x, g.y * h.y, g.z * h.z, g.w * h.w};
          uint32_t hi[4], mi[4], lo[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split3(t[e], hi[e], mi[e], lo[e]);
          const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
          const size_t pl = (size_t)4 * M * 16;
          *(uint2*)(p.XSout + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
          *(uint2*)(p.XSout + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
          *(uint2*)(p.XSout + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
        }
        ssq += __shfl_xor(ssq, 16, 64);
        ssq += __shfl_xor(ssq, 32, 64);
        if (lane < 16 && valid) p.ssout[(size_t)m * NT + nt] = ssq;
      } else if (EPI == EPI_SWIGLU) {
        if (valid) {
          const float a0 = (s.x / (1.0f + expf(-s.x))) * s.y;
          const float a1 = (s.z / (1.0f + expf(-s.z))) * s.w;
          uint32_t h0, q0, l0, h1, q1, l1;
          split3(a0, h0, q0, l0);
          split3(a1, h1, q1, l1);
          const int k = n >> 1;
          const size_t o = xs_off(k >> 5, 0, (k >> 3) & 3, m, M) + ((k >> 1) & 3) * 4;
          const size_t pl = (size_t)4 * M * 16;
          *(uint32_t*)(p.XSout + o) = h0 | (h1 << 16);
          *(uint32_t*)(p.XSout + o + pl) = q0 | (q1 << 16);
          *(uint32_t*)(p.XSout + o + 2 * pl) = l0 | (l1 << 16);
        }
      } else if (EPI == EPI_QKV) {
        if (valid) {
          const float4 b = pre_g[i];
          s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
          const RowDesc rd = pre_rd[mt];
          if (n < p.q_dim + p.kv_dim) {
            const float2 c0 = pre_c[i][mt][0], c1 = pre_c[i][mt][1];
            float4 r;
            r.x = __fadd_rn(__fmul_rn(s.x, c0.x), __fmul_rn(-s.y, c0.y));
            r.y = __fadd_rn(__fmul_rn(s.y, c0.x), __fmul_rn(s.x, c0.y));
            r.z = __fadd_rn(__fmul_rn(s.z, c1.x), __fmul_rn(-s.w, c1.y));
            r.w = __fadd_rn(__fmul_rn(s.w, c1.x), __fmul_rn(s.z, c1.y));
            s = r;
          }
          if (n < p.q_dim) {
            *(float4*)(p.Y + (size_t)m * p.q_dim + n) = s;
          } else {
            const bool isk = n < p.q_dim + p.kv_dim;
            const int c = n - p.q_dim - (isk ? 0 : p.kv_dim);
            const size_t off = kv_row(p.km, rd.slot, c >> 6, p.n_kv, p.max_pos, rd.pos) * 64 + (c & 63);
            void* base = isk ? p.kcache : p.vcache;
            if (KVF32) {
              *(float4*)((float*)base + off) = s;
            } else {
              uint2 pk;
              pk.x = smi_f32_to_bf16(s.x) | (smi_f32_to_bf16(s.y) << 16);
              pk.y = smi_f32_to_bf16(s.z) | (smi_f32_to_bf16(s.w) << 16);
              *(uint2*)((uint16_t*)base + off) = pk;
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// lm_head for up to 16 rows: persistent blocks.  The activation triples of the wave's k tiles are
// loaded once and stay in registers; the block then streams groups of two 16-row vocabulary tiles
// (next group's weights requested as soon as the MFMAs have consumed the current ones) and keeps
// a running arg-max per row.  Same k-tile -> wave map, accumulator chains and reduction order as
// k_gemm<EPI_LM>, so the logits are bit-identical to the two-m-tile path.
// ------------------------------------------------------------------------------------------
// HV = 2: two groups of four waves share a block and the weight stream (the second group's tile loads hit L2); group h
// owns rows m0 + 16 h .. and does exactly what the HV = 1 kernel does for 16 rows, so the logits are the same bits.
// RT = 1 (restricted lm_head, every row of the step constrained): group g's two vocabulary tiles are entries 2g, 2g + 1 of the
// device tile list p.tlist (the union of the rows' allowed tiles) instead of tiles 2g, 2g + 1; the group count is read from the
// list.  A tile's chains, wave map and reduction are those of the full kernel, so every logit computed is the same bits; the
// epilogue then sets the ids outside the row's own ranges to -inf before the logits store and the running arg-max.
// Clamped list entries: lm_tile.
__device__ __forceinline__ int lm_tile(const int* tlist, int idx) {
  const int c = tlist[0];
  idx = idx < c ? idx : c - 1;
  return tlist[1 + (idx > 0 ? idx : 0)];
}
// the screen's list (k_lm_select): entry idx of a list of c entries (c already clamped to NT), the tile index clamped as well
__device__ __forceinline__ int lm_tile_scr(const int* tlist, int idx, int c, int NT) {
  idx = idx < c ? idx : c - 1;
  const int t = tlist[1 + (idx > 0 ? idx : 0)];
  return t < 0 ? 0 : t < NT ? t : NT - 1;
}
// RT epilogue: the four logits of ids n .. n + 3 of the row in `slot`, outside its ranges -> -inf
__device__ __forceinline__ void lm_mask4(const Ctl* ctl, int slot, int n, float4& s) {
  const AllowRec* a = &ctl->allow[slot];
  if (!allow_has(a, n + 0)) s.x = -INFINITY;
  if (!allow_has(a, n + 1)) s.y = -INFINITY;
  if (!allow_has(a, n + 2)) s.z = -INFINITY;
  if (!allow_has(a, n + 3)) s.w = -INFINITY;
}
// NM = 1 (with RT): the list is the int8 screen's (k_lm_select) -- the row is unconstrained, so the epilogue masks nothing, and the
// list's count is clamped to NT.
template <int HV, int RT = 0, int NM = 0>
__global__ __launch_bounds__(256 * HV) void k_lm(GemmP p, int ngroups_arg, int m0_launch) {
  constexpr int NTB = 2, NW = 4, U = 8, MT = 1;
  constexpr size_t kHalfBytes = (size_t)NW * NTB * MT * 1024 + 32 * 4 + NTB * 32 * 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
  const int half = HV == 2 ? (int)threadIdx.x >> 8 : 0;
  unsigned char* smem = smem_all + half * kHalfBytes;
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, NT = p.NT;
  const int m0 = m0_launch + 16 * half;
  const int M = p.M - m0 < 16 ? (p.M - m0 > 0 ? p.M - m0 : 0) : 16;   // this wave group: rows m0 .. m0 + M - 1 (none: it only keeps the barriers)
  const int ntl = !RT ? 0 : NM ? (p.tlist[0] < NT ? p.tlist[0] : NT) : p.tlist[0];   // RT: vocabulary tiles in the list
  const int ngroups = RT ? (ntl + NTB - 1) / NTB : ngroups_arg;
  float4* red = (float4*)smem;                                   // [NW][NTB][64]
  float* rarr = (float*)(smem + (size_t)NW * NTB * MT * 1024);
  float* bestv = rarr + 32;                                      // [NTB][32] running best of this block
  int* besti = (int*)(bestv + NTB * 32);
  const int k8 = lane >> 4, em = lane & 15;
  const int mrow = em < M ? em : (M > 0 ? M - 1 : 0);
  const int xrow = m0 + mrow < p.M ? m0 + mrow : p.M - 1;
  bf16x8 bf[U][3];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int j = wave + u * NW;
    j = j < KT ? j : KT - 1;
#pragma unroll
    for (int s = 0; s < 3; ++s) bf[u][s] = *(const bf16x8*)(p.XS + xs_off(j, s, k8, xrow, p.M));
  }
  uint4 w[U][NTB];
  auto load_w = [&](int g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int j = wave + u * NW;
      j = j < KT ? j : KT - 1;
#pragma unroll
      for (int nb = 0; nb < NTB; ++nb) {
        int nt = g * NTB + nb;
        nt = !RT ? (nt < NT ? nt : NT - 1) : NM ? lm_tile_scr(p.tlist, nt, ntl, NT) : lm_tile(p.tlist, nt);
        w[u][nb] = smi_ldw(&p.W[((size_t)nt * KT + j) * 64 + lane]);
      }
    }
  };
  int g = blockIdx.x;
  if (g < ngroups) load_w(g);
  for (int m = wave; m < M; m += NW) {
    float v = smi_ss_lane_sum(p.sspart + (size_t)(m0 + m) * p.npart, p.npart, lane);
    v = smi_wave_sum(v);
    if (lane == 0) rarr[m] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
  }
  for (int i = tid; i < NTB * 32; i += 256) { bestv[i] = -INFINITY; besti[i] = 0x7fffffff; }
  __syncthreads();
  const float rn = rarr[mrow];
  for (; g < ngroups; g += gridDim.x) {
    f32x4 acc[3][NTB];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < NTB; ++a) acc[c][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (wave + u * NW < KT) {
#pragma unroll
        for (int nb = 0; nb < NTB; ++nb) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, w[u][nb]);
          acc[2][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][2], acc[2][nb], 0, 0, 0);
          acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][1], acc[1][nb], 0, 0, 0);
          acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][0], acc[0][nb], 0, 0, 0);
        }
      }
    }
    const int gn = g + gridDim.x;
    if (gn < ngroups) load_w(gn);          // overlaps the reduction and the epilogue below
#pragma unroll
    for (int nb = 0; nb < NTB; ++nb) {
      const f32x4 t = (acc[2][nb] + acc[1][nb]) + acc[0][nb];
      red[(wave * NTB + nb) * 64 + lane] = make_float4(t[0], t[1], t[2], t[3]);
    }
    __syncthreads();
    if (wave < NTB) {
      const int nb = wave, nt = RT ? (g * NTB + nb < ntl ? p.tlist[1 + g * NTB + nb] : NT) : g * NTB + nb;
      if (nt < NT && (!NM || nt >= 0)) {
        float4 s = red[(0 * NTB + nb) * 64 + lane];
#pragma unroll
        for (int wv = 1; wv < NW; ++wv) {
          const float4 t = red[(wv * NTB + nb) * 64 + lane];
          s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        s.x *= rn; s.y *= rn; s.z *= rn; s.w *= rn;
        const int n = nt * 16 + 4 * (lane >> 4);
        const bool valid = em < M;
        if (RT && !NM && valid) lm_mask4(p.ctl, p.rows[m0 + em].slot, n, s);
        if (valid && p.Y) {
          float* y = p.Y + (size_t)(m0 + em) * p.V + n;
          if (n + 0 < p.V) y[0] = s.x;
          if (n + 1 < p.V) y[1] = s.y;
          if (n + 2 < p.V) y[2] = s.z;
          if (n + 3 < p.V) y[3] = s.w;
        }
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.V && sv[r] > bv) { bv = sv[r]; bi = n + r; }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane < 16 && valid) {
          const float cv = bestv[nb * 32 + em];
          const int ci = besti[nb * 32 + em];
          if (bv > cv || (bv == cv && bi < ci)) { bestv[nb * 32 + em] = bv; besti[nb * 32 + em] = bi; }
        }
      }
    }
    __syncthreads();   // red is rewritten by the next group
  }
  if (tid < M) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int nb = 0; nb < NTB; ++nb) {
      const float ov = bestv[nb * 32 + tid];
      const int oi = besti[nb * 32 + tid];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    p.pval[(size_t)(m0 + tid) * gridDim.x + blockIdx.x] = bv;
    p.pidx[(size_t)(m0 + tid) * gridDim.x + blockIdx.x] = bi;
  }
}


// ------------------------------------------------------------------------------------------
// One-row greedy lm_head behind an int8 screen.  The step needs one number of the 297 MB matrix: the lowest id
// of the maximum.  An int8 copy of the matrix (half the bytes; built once per handle by k_lm_pack8) proves for all but a few
// 16-row vocabulary tiles that they cannot hold it; k_lm<1, RT, NM> then computes the listed tiles with the full kernel's chains
// and order, so the partials that reach k_finalize hold the same maximum bits and the same lowest id.
//   copy:    row v:  s_v = max_k |w_vk| / 127,  q_vk = rint(w_vk / s_v) (int8),  Q_v = sum_k |q_vk|;  tiles of 16 rows x 64 k
//            (1 KiB, lane l holds row l & 15, k = 16 (l >> 4) .. + 15: the A operand of v_mfma_i32_16x16x64_i8), K zero-padded
//   operand: x = a X1 + b X2 + r,  a = max|x| / 127,  b = a / 254,  X1, X2 int8,  |r_k| <= b / 2 (columns 0 and 1 of the B operand)
//   screen:  S_v = s_v (a A1 + b A2),  A1 = sum q X1, A2 = sum q X2 exact in int32;
//            |S_v - sum_k w_vk x_k| <= B_v = (s_v / 2) |x|_1 + (s_v Q_v) b / 2 + 2^-12 (s_v Q_v) max|x|   (the last term: fp32 rounding
//            of S_v, of B_v and of k_lm's own sums)
//   out:     per tile max (S_v + B_v) over its ids below V, per block max (S_v - B_v): a tile is a candidate when its upper bound
//            reaches the largest lower bound (k_lm_select).  The RMSNorm factor is a positive common factor of the row and is left out.
// A non-finite operand or max|x| = 0 marks every tile (upper bounds +inf, lower bounds -inf): the recompute then walks them all.
// ------------------------------------------------------------------------------------------
struct ScreenP {
  const uint4* Q8;           // [NT][KT64][64] 16-byte lane pieces of the int8 copy
  const float* s8;           // [NT * 16] s_v
  const float* sq8;          // [NT * 16] s_v Q_v
  const unsigned char* XS;   // the operand's triples (row 0 of M)
  int M, NT, KT, KT64, V;
  float* ub;                 // [NT] per-tile upper bounds
  float* lb;                 // [nlb] per-block lower bounds
  int nlb;
  int* list;                 // {count, tiles ascending}
  int* log;                  // diagnostics: {n, the counts of the last 4096 selections}, or null
};
constexpr int kScrKT = 16;   // k tiles of 64 a wave holds: K <= 1024 (the persistent lm_head's range)

// The copy of one vocabulary tile per block (once per handle, outside any capture): thread (r = tid & 15, c = tid >> 4) walks
// k = c, c + 16, .. of row r of the bf16 tile (lane piece ((k >> 3) & 3) * 16 + r of k tile k >> 5).
__global__ __launch_bounds__(256) void k_lm_pack8(const uint16_t* W, int KT, int KT64, int V, unsigned char* Q8, float* s8, float* sq8) {
  __shared__ float smx[4][16];
  __shared__ int sqs[4][16];
  const int nt = blockIdx.x, tid = threadIdx.x, r = tid & 15, c = tid >> 4, wave = tid >> 6, K = KT * 32;
  const int row = nt * 16 + r;
  auto elem = [&](int k) {
    return smi_bf16_to_f32(W[(((size_t)nt * KT + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + r) * 8 + (k & 7)]);
  };
  float mx = 0.f;
  for (int k = c; k < K; k += 16) mx = fmaxf(mx, fabsf(elem(k)));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if ((tid & 63) < 16) smx[wave][r] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(smx[0][r], smx[1][r]), fmaxf(smx[2][r], smx[3][r]));
  if (row >= V) mx = 0.f;   // rows past the vocabulary never count
  const float s = mx / 127.0f;
  int qs = 0;
  for (int k = c; k < K; k += 16) {
    float q = s > 0.f ? rintf(elem(k) / s) : 0.f;
    q = fminf(fmaxf(q, -127.f), 127.f);
    const int qi = (int)q;
    qs += qi < 0 ? -qi : qi;
    Q8[((size_t)nt * KT64 + (k >> 6)) * 1024 + (((k & 63) >> 4) * 16 + r) * 16 + (k & 15)] = (unsigned char)(signed char)qi;
  }
  qs += __shfl_xor(qs, 16, 64);
  qs += __shfl_xor(qs, 32, 64);
  if ((tid & 63) < 16) sqs[wave][r] = qs;
  __syncthreads();
  if (tid < 16) {
    const int Qv = sqs[0][r] + sqs[1][r] + sqs[2][r] + sqs[3][r];
    s8[row] = s;
    sq8[row] = s * (float)Qv;
  }
}

// U = kScrKT: any K (loads and MFMAs of k tiles past KT64 are skipped, wave-uniform); otherwise KT64 == U exactly.
template <int U>
__global__ __launch_bounds__(256) void k_lm_screen(ScreenP p) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  constexpr bool ANY = U == kScrKT;
  __shared__ float xf[kScrKT * 64];
  __shared__ __attribute__((aligned(16))) signed char x1[kScrKT * 64];
  __shared__ __attribute__((aligned(16))) signed char x2[kScrKT * 64];
  __shared__ float rmx[4], rl1[4], rlo[4];
  __shared__ int rbad[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = p.NT, KT64 = p.KT64;
  const int nw = (int)gridDim.x * 4, gw = (int)blockIdx.x * 4 + wave;
  const int g4 = lane >> 4, c = lane & 15;
  // the wave's first two tiles leave before anything else
  uint4 wA[U], wB[U];
  float4 sA, qA, sB, qB;
  auto load = [&](uint4 (&w)[U], float4& s, float4& q, int t) {
    t = t < NT ? t : NT - 1;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (!ANY || u < KT64) w[u] = smi_ldw(&p.Q8[((size_t)t * KT64 + u) * 64 + lane]);
    s = *(const float4*)(p.s8 + (size_t)t * 16 + 4 * g4);
    q = *(const float4*)(p.sq8 + (size_t)t * 16 + 4 * g4);
  };
  if (gw < NT) load(wA, sA, qA, gw);
  if (gw + nw < NT) load(wB, sB, qB, gw + nw);
  // ---- the operand: rebuilt from its triples (exact), max|x|, |x|_1, finite?
  float mx = 0.f, l1 = 0.f;
  int bad = 0;
  for (int i = tid; i < kScrKT * 8; i += 256) {   // pieces of 8 k
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (i < p.KT * 4) {
      const uint4 h = *(const uint4*)(p.XS + xs_off(i >> 2, 0, i & 3, 0, p.M));
      const uint4 m = *(const uint4*)(p.XS + xs_off(i >> 2, 1, i & 3, 0, p.M));
      const uint4 l = *(const uint4*)(p.XS + xs_off(i >> 2, 2, i & 3, 0, p.M));
      const uint32_t hu[4] = {h.x, h.y, h.z, h.w}, mu[4] = {m.x, m.y, m.z, m.w}, lu[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[2 * e] = (__uint_as_float(hu[e] << 16) + __uint_as_float(mu[e] << 16)) + __uint_as_float(lu[e] << 16);
        v[2 * e + 1] = (__uint_as_float(hu[e] & 0xffff0000u) + __uint_as_float(mu[e] & 0xffff0000u)) + __uint_as_float(lu[e] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float av = fabsf(v[e]);
      bad |= !(av <= 3.4028234664e38f);   // NaN or inf
      mx = fmaxf(mx, av);
      l1 += av;
      xf[i * 8 + e] = v[e];
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    l1 += __shfl_xor(l1, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (lane == 0) { rmx[wave] = mx; rl1[wave] = l1; rbad[wave] = bad; }
  __syncthreads();
  mx = fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
  l1 = (rl1[0] + rl1[1]) + (rl1[2] + rl1[3]);
  const float a = mx / 127.0f, b = a / 254.0f;
  const bool allc = (rbad[0] | rbad[1] | rbad[2] | rbad[3]) != 0 || !(b > 0.f);   // every tile a candidate (max|x| = 0, or so small that b underflows)
  for (int k = tid; k < kScrKT * 64; k += 256) {
    float X1 = 0.f, X2 = 0.f;
    if (!allc) {
      const float x = xf[k];
      X1 = fminf(fmaxf(rintf(x / a), -127.f), 127.f);
      X2 = fminf(fmaxf(rintf(fmaf(-a, X1, x) / b), -127.f), 127.f);
    }
    x1[k] = (signed char)(int)X1;
    x2[k] = (signed char)(int)X2;
  }
  __syncthreads();
  i32x4 bq[U];   // B operand: column 0 = X1, column 1 = X2, the rest zero; lane (c, g4) holds k = 16 g4 .. + 15 of each k tile
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const i32x4 z = {0, 0, 0, 0};
    bq[u] = c == 0 ? *(const i32x4*)(x1 + u * 64 + 16 * g4) : c == 1 ? *(const i32x4*)(x2 + u * 64 + 16 * g4) : z;
  }
  const float hl1 = 0.5f * l1, hb = 0.5f * b, slack = mx * 0.000244140625f;   // 2^-12 max|x|
  float lo_run = -INFINITY;
  auto tile = [&](uint4 (&w)[U], float4& sv, float4& qv, int t) {
    i32x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (!ANY || u < KT64) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, w[u]), bq[u], acc, 0, 0, 0);
    const float4 s4 = sv, q4 = qv;
    const int tn = t + 2 * nw;
    if (tn < NT) load(w, sv, qv, tn);   // the tile after next: in flight under the epilogue and the other buffer's MFMAs
    // lanes c == 0 hold A1 of rows 4 g4 + r, lanes c == 1 A2
    const float s[4] = {s4.x, s4.y, s4.z, s4.w}, q[4] = {q4.x, q4.y, q4.z, q4.w};
    float up = -INFINITY, lo = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a2 = __shfl_down(acc[r], 1, 64);
      const float S = s[r] * (a * (float)acc[r] + b * (float)a2);
      const float Bd = (s[r] * hl1 + q[r] * hb) + q[r] * slack;
      if (c == 0 && t * 16 + 4 * g4 + r < p.V) { up = fmaxf(up, S + Bd); lo = fmaxf(lo, S - Bd); }
    }
    up = fmaxf(up, __shfl_xor(up, 16, 64));
    up = fmaxf(up, __shfl_xor(up, 32, 64));
    lo = fmaxf(lo, __shfl_xor(lo, 16, 64));
    lo = fmaxf(lo, __shfl_xor(lo, 32, 64));
    if (lane == 0) p.ub[t] = allc ? INFINITY : up;
    lo_run = fmaxf(lo_run, lo);
  };
  for (int t = gw; t < NT; t += 2 * nw) {
    tile(wA, sA, qA, t);
    if (t + nw < NT) tile(wB, sB, qB, t + nw);
  }
  if (lane == 0) rlo[wave] = lo_run;
  __syncthreads();
  if (tid == 0 && (int)blockIdx.x < p.nlb) p.lb[blockIdx.x] = allc ? -INFINITY : fmaxf(fmaxf(rlo[0], rlo[1]), fmaxf(rlo[2], rlo[3]));
}

// One block: thr = the largest block lower bound; the tiles whose upper bound reaches it, ascending, as {count, tiles}.  A NaN
// bound lists its tile.  Thread i owns the tiles i * per .. : counts, a block-wide exclusive scan, then the writes.
__global__ __launch_bounds__(1024) void k_lm_select(ScreenP p) {
  __shared__ float sthr[16];
  __shared__ int scnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = p.NT;
  float thr = -INFINITY;
  for (int i = tid; i < p.nlb; i += 1024) thr = fmaxf(thr, p.lb[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) thr = fmaxf(thr, __shfl_xor(thr, o, 64));
  if (lane == 0) sthr[wave] = thr;
  __syncthreads();
  thr = sthr[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) thr = fmaxf(thr, sthr[i]);
  const int per = (NT + 1023) / 1024, t0 = tid * per, t1 = t0 + per < NT ? t0 + per : NT;
  int n = 0;
  for (int t = t0; t < t1; ++t) n += !(p.ub[t] < thr);
  int inc = n;   // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) scnt[wave] = inc;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) { base += i < wave ? scnt[i] : 0; total += scnt[i]; }
  int o = base + inc - n;
  for (int t = t0; t < t1; ++t)
    if (!(p.ub[t] < thr)) p.list[1 + o++] = t;
  if (tid == 0) {
    p.list[0] = total;
    if (p.log) { const int i = p.log[0]; p.log[1 + (i & 4095)] = total; p.log[0] = i + 1; }
  }
}

// lm_head for 17..32 rows per pass: ONE 4-wave group streams the weights once for both m-tiles.  Rows m0..m0+15 keep their
// operand triples in registers exactly as in k_lm<1>; rows m0+16..m0+31 keep theirs in LDS (86 KB at K = 896: [k tile][3][4][16][16 B]),
// read as MFMA B operands straight from there (3 KB of LDS reads per 1 KB weight tile -- far below the LDS rate).  k_lm<2>
// gave each 16-row group its own four waves, i.e. every weight tile was pulled into registers twice per CU (72 us at 32
// rows); here it is pulled once.  Same k-tile -> wave map, chains and reduction order per row as k_lm<1>: same logits bits.
// Round 4: TWO weight register sets (one wave per SIMD: the 512-register budget holds them).  With one set a group's tiles were
// requested only after the previous group's 84 MFMAs per wave had consumed the registers, so the stream stood still during the
// MFMAs, the reduction and the epilogue (3.2 us per group against 2.3 us for the 56 KB at the CU's share of the HBM rate); now
// the tiles of group g + 2 are requested as soon as group g's MFMAs are issued and the tiles of g + 1 are already in flight.
// UW = k tiles per wave (ceil(KT / 4)): no clamped duplicate loads (U = 8 at KT = 28 re-requested tile 27 once per wave and n tile).
// RT = 1: the restricted form, as k_lm's (groups through the tile list, the rows' own ranges masked in the epilogue).
template <int UW, int RT = 0>
__global__ __launch_bounds__(256) void k_lm32(GemmP p, int ngroups_arg, int m0) {
  constexpr int NTB = 2, NW = 4, U = UW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KT = p.KT, NT = p.NT;
  const int ntl = RT ? p.tlist[0] : 0;
  const int ngroups = RT ? (ntl + NTB - 1) / NTB : ngroups_arg;
  const int M = p.M - m0 < 32 ? p.M - m0 : 32;                    // rows of this pass (>= 1)
  float4* red = (float4*)smem;                                     // [NW][NTB][2][64]
  float* rarr = (float*)(smem + (size_t)NW * NTB * 2 * 1024);      // [32]
  float* bestv = rarr + 32;                                        // [NTB][32]
  int* besti = (int*)(bestv + NTB * 32);
  uint4* xl = (uint4*)(smem + (size_t)NW * NTB * 2 * 1024 + 32 * 4 + NTB * 32 * 8);   // [KT][3][4][16]
  const int k8 = lane >> 4, em = lane & 15;
  const int row0 = m0 + (em < M ? em : M - 1);                     // m-tile 0 row of this lane (clamped)
  // ---- prologue: EVERY load of it is requested before anything waits -- the RMSNorm partials of this wave's rows (8 rows x 4
  // dwords), the m-tile-0 operand registers, the 21 pieces per thread of m-tile 1's LDS image, then the first two groups' weight
  // tiles.  As first written (round 3) the image was copied load -> wait -> ds_write per piece and the partials row by row: 29
  // dependent round trips behind the cold weight tiles, 14 of the kernel's 65 us (round-4 stamps: block 0 streams its 20 groups
  // in 50 us).  Loads return in issue order, so the small L2-resident ones go first.
  constexpr int RPW = 8;                                           // rows per wave (32 / NW)
  float ssv[RPW][4];
  const bool ss_early = p.npart <= 256;
  if (ss_early) {
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      int mr = m0 + wave + i * NW;
      mr = mr < p.M ? mr : p.M - 1;
      const float* sp = p.sspart + (size_t)mr * p.npart;
      const int last = p.npart - 1;
      ssv[i][0] = sp[lane < last ? lane : last]; ssv[i][1] = sp[lane + 64 < last ? lane + 64 : last];
      ssv[i][2] = sp[lane + 128 < last ? lane + 128 : last]; ssv[i][3] = sp[lane + 192 < last ? lane + 192 : last];
    }
  }
  bf16x8 bf[U][3];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int j = wave + u * NW;
    j = j < KT ? j : KT - 1;
#pragma unroll
    for (int s = 0; s < 3; ++s) bf[u][s] = *(const bf16x8*)(p.XS + xs_off(j, s, k8, row0, p.M));
  }
  constexpr int XPT = (UW * NW * 12 * 16 + 255) / 256;             // LDS-image pieces per thread (KT <= UW * NW)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 xpc[XPT];
  const int nxl = KT * 12 * 16;
#pragma unroll
  for (int q = 0; q < XPT; ++q) {
    int i = tid + 256 * q;
    i = i < nxl ? i : nxl - 1;
    const int r = i & 15, pcx = i >> 4;                            // pcx = (kt * 3 + s) * 4 + k8
    int mr = m0 + 16 + r;
    mr = mr < p.M ? mr : p.M - 1;
    xpc[q] = *(const u32x4*)(p.XS + ((size_t)pcx * p.M + mr) * 16);
  }
  uint4 w0[U][NTB], w1[U][NTB];
  // EVERY request below is unconditional (group and tile indices are clamped, a block's surplus requests re-read the last group
  // out of L2): with `if (gn < ngroups) load_w(..)` the number of loads in flight depends on the path, the compiler's counted
  // waits must assume the smallest -- and the wait for one register set then drained the other set's requests too (round-3's
  // "two register sets change nothing", and this kernel's first round-4 build: s_waitcnt vmcnt(13) .. vmcnt(0) in front of a
  // group's MFMAs with 28 loads outstanding).
  auto load_w = [&](uint4 (&w)[U][NTB], int gq) {
    const int g = gq < ngroups ? gq : ngroups - 1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int j = wave + u * NW;
      j = j < KT ? j : KT - 1;
#pragma unroll
      for (int nb = 0; nb < NTB; ++nb) {
        int nt = g * NTB + nb;
        nt = RT ? lm_tile(p.tlist, nt) : (nt < NT ? nt : NT - 1);
        w[u][nb] = smi_ldw(&p.W[((size_t)nt * KT + j) * 64 + lane]);
      }
    }
  };
  const int G = (int)gridDim.x;
  int g = blockIdx.x;
  load_w(w0, g);
  load_w(w1, g + G);
  // m-tile 1's operand pieces -> LDS (rows beyond M repeat the last row; their results are never stored)
#pragma unroll
  for (int q = 0; q < XPT; ++q) asm volatile("" : "+v"(xpc[q]));   // (the loads stay above the weight requests, not sunk into the guarded stores)
#pragma unroll
  for (int q = 0; q < XPT; ++q) {
    const int i = tid + 256 * q;
    if (i < nxl) *(u32x4*)&xl[i] = xpc[q];
  }
  if (ss_early) {   // same order as smi_ss_lane_sum + smi_wave_sum
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int m = wave + i * NW;
      float v = lane < p.npart ? ssv[i][0] : 0.f;
      v += lane + 64 < p.npart ? ssv[i][1] : 0.f;
      v += lane + 128 < p.npart ? ssv[i][2] : 0.f;
      v += lane + 192 < p.npart ? ssv[i][3] : 0.f;
      v = smi_wave_sum(v);
      if (lane == 0 && m < M) rarr[m] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
    }
  } else {
    for (int m = wave; m < M; m += NW) {
      float v = smi_ss_lane_sum(p.sspart + (size_t)(m0 + m) * p.npart, p.npart, lane);
      v = smi_wave_sum(v);
      if (lane == 0) rarr[m] = 1.0f / sqrtf(v / (float)(KT * 32) + p.eps);
    }
  }
  for (int i = tid; i < NTB * 32; i += 256) { bestv[i] = -INFINITY; besti[i] = 0x7fffffff; }
  __syncthreads();
  const int nb_e = wave & 1, mt_e = wave >> 1;                     // the (n tile, m tile) this wave finishes
  const int ml = mt_e * 16 + em;                                   // its row (local)
  const float rn = rarr[ml < M ? ml : 0];
  int gi = 0;   // (diagnostics) groups this block has finished
#ifdef SMI_DIAG
#define SMI_LMSTAMP(i) do { if (p.stamps && blockIdx.x == 0 && tid == 0 && gi < 32) p.stamps[gi * 4 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SMI_LMSTAMP(i) do { } while (0)
#endif
  auto group = [&](uint4 (&w)[U][NTB], int gcur) {
    SMI_LMSTAMP(0);
    f32x4 acc[3][NTB][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int a = 0; a < NTB; ++a) { acc[c][a][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[c][a][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = wave + u * NW;
      if (j < KT) {
        bf16x8 b1[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) b1[s] = __builtin_bit_cast(bf16x8, xl[((j * 3 + s) * 4 + k8) * 16 + em]);
#pragma unroll
        for (int nb = 0; nb < NTB; ++nb) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, w[u][nb]);
          acc[2][nb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][2], acc[2][nb][0], 0, 0, 0);
          acc[1][nb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][1], acc[1][nb][0], 0, 0, 0);
          acc[0][nb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[u][0], acc[0][nb][0], 0, 0, 0);
          acc[2][nb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1[2], acc[2][nb][1], 0, 0, 0);
          acc[1][nb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1[1], acc[1][nb][1], 0, 0, 0);
          acc[0][nb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1[0], acc[0][nb][1], 0, 0, 0);
        }
      }
    }
    load_w(w, gcur + 2 * G);               // this set's registers are free again: the group after next, while the other set's tiles are in flight
#pragma unroll
    for (int nb = 0; nb < NTB; ++nb)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const f32x4 t = (acc[2][nb][mt] + acc[1][nb][mt]) + acc[0][nb][mt];
        red[((wave * NTB + nb) * 2 + mt) * 64 + lane] = make_float4(t[0], t[1], t[2], t[3]);
      }
    SMI_LMSTAMP(1);
    __syncthreads();
    SMI_LMSTAMP(2);
    {
      const int nt = RT ? (gcur * NTB + nb_e < ntl ? p.tlist[1 + gcur * NTB + nb_e] : NT) : gcur * NTB + nb_e;
      if (nt < NT) {
        float4 s = red[((0 * NTB + nb_e) * 2 + mt_e) * 64 + lane];
#pragma unroll
        for (int wv = 1; wv < NW; ++wv) {
          const float4 t = red[((wv * NTB + nb_e) * 2 + mt_e) * 64 + lane];
          s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        s.x *= rn; s.y *= rn; s.z *= rn; s.w *= rn;
        const int n = nt * 16 + 4 * (lane >> 4);
        const bool valid = ml < M;
        if (RT && valid) lm_mask4(p.ctl, p.rows[m0 + ml].slot, n, s);
        if (valid && p.Y) {
          float* y = p.Y + (size_t)(m0 + ml) * p.V + n;
          if (n + 0 < p.V) y[0] = s.x;
          if (n + 1 < p.V) y[1] = s.y;
          if (n + 2 < p.V) y[2] = s.z;
          if (n + 3 < p.V) y[3] = s.w;
        }
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.V && sv[r] > bv) { bv = sv[r]; bi = n + r; }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane < 16 && valid) {
          const float cv = bestv[nb_e * 32 + ml];
          const int ci = besti[nb_e * 32 + ml];
          if (bv > cv || (bv == cv && bi < ci)) { bestv[nb_e * 32 + ml] = bv; besti[nb_e * 32 + ml] = bi; }
        }
      }
    }
    __syncthreads();   // red is rewritten by the next group
    SMI_LMSTAMP(3);
    ++gi;
    (void)gi;
  };
#undef SMI_LMSTAMP
  for (; g < ngroups; g += 2 * G) {   // block-uniform trip counts (every wave keeps the barriers); a group beyond the last stores nothing
    group(w0, g);
    group(w1, g + G);
  }
  if (tid < M) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int nb = 0; nb < NTB; ++nb) {
      const float ov = bestv[nb * 32 + tid];
      const int oi = besti[nb * 32 + tid];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    p.pval[(size_t)(m0 + tid) * gridDim.x + blockIdx.x] = bv;
    p.pidx[(size_t)(m0 + tid) * gridDim.x + blockIdx.x] = bi;
  }
}

struct AttnP {
  const float* q;      // [M][q_dim]
  const void* kcache;  // layer base
  const void* vcache;
  const RowDesc* rows;
  unsigned char* xs_out;  // o_proj operand: exact bf16 triples [q_dim/32][3][4][M][16 B]
  int M;
  int q_dim, n_kv, group, max_pos, n_heads;
  KvMap km;            // paged KV cache (ptab null: contiguous slots); every form reads through it -- the slot_is_row kernels in their PG instantiations
  int slot_is_row;     // every row m lives in KV slot m (decode): addresses need no descriptor
  int work_blocks;     // = n_heads * M * nseg; later blocks are prefetch helpers
  PfDesc pf;
  // long contexts: the keys are cut into fixed segments of kAttnSeg tokens, one block per (head, row, segment); each
  // block leaves (max, sum, out[64]) in `part` and k_attn_merge combines a row's segments in order.  nseg == 1: no split.
  int nseg;
  float* part;         // [M][n_heads][nseg][66]
  // fused o_proj (one-row kernel): this head's two k tiles of W_o against its own output -> per-head partial of the o_proj
  const uint4* Wo;     // [NTo][2 * n_heads][64] tiles (head-interleaved k order)
  int NTo;             // n tiles of W_o (hidden / 16)
  float* part_o;       // [n_heads][NTo * 16] f32 (FUSE = 2: [row][n_heads][NTo * 16])
  // FUSE = 2 (2 .. 8 rows): the last of a (row, quarter)'s n_heads blocks to arrive adds the heads' partials in order and runs
  // the RESID epilogue of the o_proj for that quarter of the row's columns
  unsigned int* cnt;   // [rows][kFuseQB] arrival counters (zero between launches: the last arriver resets its counter)
  float* h;            // [rows][hidden] residual stream: read and rewritten (h += o_proj)
  const float* gamma_next;   // the post-attention norm's weight
  unsigned char* xs_next;    // its operand triples [hidden / 32][3][4][M][16 B]
  float* ssout;        // [rows][NTo * 4] partial sums of squares of the new residual rows
};

constexpr int kAttnWaves = 8;
constexpr int kAttnSeg = 1024;   // tokens per segment (a multiple of the chunk of either KV type)
constexpr int kFuseQB = 4;       // fused o_proj: blocks per head -- each repeats the head's attention (latency-bound, the CUs are idle anyway)
                                 // and takes a quarter of W_o's n tiles: a CU pulls 28 KB of cold weights instead of 112 KB
constexpr int kFuse2Max = 8;     // rows up to which several live rows take the fused attention + o_proj (FUSE = 2: last-arriver head sum)
constexpr int kFuseMaxPos = 1 << 23;   // positions per slot up to which the one-row fused kernel runs: 2^23 * 64 dims * 4 B < 2^32 (32-bit K / V piece offsets)
constexpr int kFuseOT = 2;      // W_o n tiles per wave (8 waves x 2 x 4 blocks x 16 = hidden sizes up to 1024)

// k_attn's merge step 2, across the waves, for head dim d: each wave's sums rescaled to the block maximum and added in wave
// order.  Every form of the kernel runs this one piece of code (the fused one-row kernel in each of its o_proj waves), so the
// sums are the same everywhere.  (pw is requested behind the maximum; its round trip hides under the eight exp2f.)
__device__ __forceinline__ void attn_merge(const float* wmax, const float (*pw)[kHeadDim], const float* pl, int d,
                                           float& bm, float& O, float& Ls) {
  constexpr float LOG2E = 1.4426950408889634f;
  float wm[kAttnWaves], po[kAttnWaves], pls[kAttnWaves];
#pragma unroll
  for (int w = 0; w < kAttnWaves; ++w) { wm[w] = wmax[w]; po[w] = pw[w][d]; pls[w] = pl[w]; }
  bm = wm[0];
#pragma unroll
  for (int w = 1; w < kAttnWaves; ++w) bm = fmaxf(bm, wm[w]);
  O = 0.f; Ls = 0.f;
#pragma unroll
  for (int w = 0; w < kAttnWaves; ++w) {
    const float sc = exp2f((wm[w] - bm) * LOG2E);   // 0 for a wave that saw no valid token (m_run = NEG)
    O += po[w] * sc; Ls += pls[w] * sc;
  }
}

// ... and the head's output O / Ls of dim d as exact bf16 triples
__device__ __forceinline__ void attn_merge_split(const float* wmax, const float (*pw)[kHeadDim], const float* pl, int d,
                                                 uint32_t& hi, uint32_t& mi, uint32_t& lo) {
  float bm, O, Ls;
  attn_merge(wmax, pw, pl, d, bm, O, Ls);
  split3(O / Ls, hi, mi, lo);
}

// fused o_proj: dim d's triple into the B-operand pieces of the head's 64 values, [half][split][k8][8 bf16]
__device__ __forceinline__ void attn_put_pieces(unsigned char* xs, int d, uint32_t hi, uint32_t mi, uint32_t lo) {
  unsigned char* q = xs + (size_t)((d >> 5) * 12 + ((d >> 3) & 3)) * 16 + (d & 7) * 2;
  *(uint16_t*)q = (uint16_t)hi;
  *(uint16_t*)(q + 64) = (uint16_t)mi;
  *(uint16_t*)(q + 128) = (uint16_t)lo;
}

// 8 waves; a group of LPT lanes owns one token per pass (16-byte K and V pieces per lane, dot product
// reduced on the DPP path), UNR passes of loads in flight together (256 tokens per chunk with bf16
// KV).  Softmax runs per chunk against a block-wide running max (one LDS word per wave, one barrier),
// so every lane accumulates at the same scale; the final merge is a plain sum: inside the wave through
// its private LDS slice, across waves through one more barrier.  Little redundant work per thread:
// with one block per head the kernel is bound by instruction issue of its own waves.
// ONE == 1: exactly one live row in KV slot 0 and one context segment (batch-1 decode): index arithmetic folded at compile
// time.  ONE == 2: several rows, row m in KV slot m, one context segment (plain batched decode): the K/V addresses do not
// depend on the row descriptor, so descriptor, q and the first K/V chunk travel together as in the one-row kernel.
// FUSE (with ONE == 1): the block goes on to multiply its head's output with that head's two k tiles of W_o (requested at
// kernel entry, in flight under the whole attention) and leaves a per-head partial of the o_proj; the consumer
// (k_gemm<PRO_FUSEDO>: gate_up) adds the heads in order, which is the order k_gemm<RESID> with NW = n_heads sums its waves in:
// one kernel boundary and one cold weight stream less per layer, same bits.
// The W_o tiles are held by eight EXTRA waves (8..15): they request their tiles at entry, sit at the block's merge barrier
// while waves 0..7 run the attention exactly as in the plain kernel, then each runs the cross-wave merge (step 2) for itself
// into a slice of LDS of its own -- no second barrier, the attention waves end at the first -- and multiplies and stores.  (Issued
// by the attention waves themselves, the cold weight loads either hold q / K / V back -- loads return in issue order -- or,
// issued behind them, are caught by the compiler's counted waits for K / V.)
// PG (with ONE != 0): the KV cache is paged -- a token's row comes through the slot's page-table row (one more dependent,
// cache-resident load in front of the K/V loads; every table entry is a valid page at all times, so the unconditional first
// chunk stays safe), everything else as the slot == row kernels.
// FUSE == 2 (with ONE == 2; round 4): the fused o_proj for 2 .. 8 live rows.  Four blocks per (row, head) as at one row; a block
// leaves its per-head partial of a quarter of the row's columns in part_o with write-through (sc1) stores, drains them, and -- behind
// a workgroup barrier -- one lane counts the block in on the (row, quarter)'s counter with an agent-scope atomic add.  The block whose
// add returns n_heads - 1 is the last: its first 56 lanes read the n_heads partials of their 4 columns with sc1 loads (the guide's
// hand-off form: every payload byte stored sc1 and drained before the count, every read of it an sc1 load behind the add), add
// them in head order -- the order k_gemm<RESID> with NW = n_heads adds its waves, and gate_up's one-row prologue its partials --
// and run the RESID epilogue (residual add, h, the next norm's operand triples, partial sums of squares).  No block ever waits for
// another: nothing can dead-lock and there is nothing to time out.  The o_proj launch (and its boundary) is gone for these row
// counts; gate_up reads an ordinary operand (with more rows the per-head partials would be re-read by every gate_up block).
template <int KVF32, int ONE = 0, int FUSE = 0, int PG = 0>
__device__ __forceinline__ void attn_body(const AttnP& p) {
  static_assert(!FUSE || (FUSE == 1 && ONE == 1) || (FUSE == 2 && ONE == 2), "fused o_proj: one row (per-head partials for gate_up) or 2..8 rows (last-arriver head sum)");
  constexpr int LPT = KVF32 ? 16 : 8;   // lanes per token row (each lane 16 bytes)
  constexpr int DPL = kHeadDim / LPT;   // dims per lane
  constexpr int TPW = 64 / LPT;         // tokens per wave per pass
  constexpr int NGRP = kAttnWaves * TPW;  // tokens per block per pass
  constexpr int UNR = 4;                // passes whose K/V loads are issued together
  constexpr float NEG = -1e30f;
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ float wmax[kAttnWaves];
  __shared__ __attribute__((aligned(16))) float so[kAttnWaves][TPW][kHeadDim];   // wave-private merge slices
  __shared__ float sl[kAttnWaves][TPW];
  __shared__ float pw[kAttnWaves][kHeadDim], pl[kAttnWaves];
  // FUSE: this head's output as B-operand pieces (FUSE == 1: one copy per o_proj wave, each wave merges for itself)
  __shared__ __attribute__((aligned(16))) unsigned char xsl[FUSE == 1 ? kAttnWaves * 2 * 3 * 4 * 16 : FUSE ? 2 * 3 * 4 * 16 : 16];
  __shared__ unsigned int s_last;   // FUSE == 2: this block was the last of its (row, quarter) to arrive
  // AHOT: the one-row fused kernel.  The wave index is a scalar (the o_proj waves' tile addresses and the attention waves' token
  // index are then scalar base + lane offset), and the block id is split into (quarter, head) and the head into its KV head
  // by compare-and-subtract on the scalar unit instead of three integer divisions in front of the q / K / V requests.
  constexpr bool AHOT = ONE == 1 && FUSE == 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = AHOT ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  if ((int)blockIdx.x >= p.work_blocks) {
    pf_run(p.pf, (int)blockIdx.x - p.work_blocks, (int)gridDim.x - p.work_blocks, tid, (FUSE ? 2 : 1) * kAttnWaves * 64);
    return;
  }
  int a_head = (int)blockIdx.x, a_q = 0, a_kvh = 0;   // AHOT: work_blocks = kFuseQB * n_heads, block = quarter * n_heads + head
  if constexpr (AHOT) {
    static_assert(kFuseQB == 4, "the quarter of a block id is found in two steps");
    if (a_head >= 2 * p.n_heads) { a_head -= 2 * p.n_heads; a_q = 2; }
    if (a_head >= p.n_heads) { a_head -= p.n_heads; a_q += 1; }
    for (int h = a_head; h >= p.group; h -= p.group) ++a_kvh;   // head / group: at most n_kv - 1 trips
  }
  // FUSE == 2: natural block order (row, quarter, head), head fastest -- the 7 query heads of a KV group and the four quarter
  // blocks of a row are neighbours; XCD x takes the x-th contiguous eighth of it (as the unfused batched kernel does)
  unsigned fbid = blockIdx.x;
  if constexpr (FUSE == 2) {
    const unsigned total = (unsigned)p.work_blocks, xcd = fbid & 7u, slot = fbid >> 3, q8 = total >> 3, r8 = total & 7u;
    fbid = xcd * q8 + (xcd < r8 ? xcd : r8) + slot;
  }
  const int f_head = AHOT ? a_head : FUSE ? (int)(fbid % (unsigned)p.n_heads) : 0,
            f_q = AHOT ? a_q : FUSE ? (int)(fbid / (unsigned)p.n_heads) % kFuseQB : 0,
            f_row = FUSE == 2 ? (int)(fbid / (unsigned)(p.n_heads * kFuseQB)) : 0;
  if constexpr (FUSE) {
    if (wave >= kAttnWaves) {   // the o_proj waves: tiles (nt, half * n_heads + head), nt = fq * fper + (wave - 8) + 8 i
      const int fq = f_q, fper = p.NTo / kFuseQB, fh = f_head;
      const int ow = wave - kAttnWaves, KTo = 2 * p.n_heads;
      uint4 wo[kFuseOT][2];
#pragma unroll
      for (int i = 0; i < kFuseOT; ++i) {
        int nl = ow + kAttnWaves * i;
        nl = nl < fper ? nl : fper - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) wo[i][j] = smi_ldw(&p.Wo[((size_t)(fq * fper + nl) * KTo + j * p.n_heads + fh) * 64 + lane]);
      }
      __syncthreads();   // the attention waves' merge barrier
      unsigned char* xo = xsl;
      if constexpr (FUSE == 1) {   // this wave runs the cross-wave merge itself (lane = dim) into its own slice: no second barrier
        xo = xsl + ow * (2 * 3 * 4 * 16);
        uint32_t hi, mi, lo;
        attn_merge_split(wmax, pw, pl, lane, hi, mi, lo);
        attn_put_pieces(xo, lane, hi, mi, lo);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own LDS writes have landed
      } else {
        __syncthreads();   // the head's output is in xsl
      }
      // MFMA columns 0 / 1 / 2 are the row's hi / mid / lo split terms (one MFMA per k tile instead of three; k_gemm LEAN == 2)
      bf16x8 bo[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bo[j] = *(const bf16x8*)(xo + (size_t)((j * 3 + ((lane & 15) < 3 ? (lane & 15) : 0)) * 4 + (lane >> 4)) * 16);
#pragma unroll
      for (int i = 0; i < kFuseOT; ++i) {
        const int nl = ow + kAttnWaves * i, nt = fq * fper + nl;
        if (nl < fper) {   // wave-uniform
          f32x4 a0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 2; ++j)   // the order of k_gemm's chains: tile by tile, lo / mid / hi in their own accumulators (here: columns)
            a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wo[i][j]), bo[j], a0, 0, 0, 0);
          f32x4 t;
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = (smi_dpp<0x102>(a0[r]) + smi_dpp<0x101>(a0[r])) + a0[r];   // (lo + mid) + hi
          if ((lane & 15) == 0) {
            float* dst = p.part_o + ((size_t)f_row * p.n_heads + fh) * (p.NTo * 16) + nt * 16 + 4 * (lane >> 4);
            if constexpr (FUSE == 2) {   // write-through: the last arriver reads these from another CU inside this launch
#pragma unroll
              for (int r = 0; r < 4; ++r) __hip_atomic_store((uint32_t*)dst + r, __float_as_uint(t[r]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
              *(float4*)dst = make_float4(t[0], t[1], t[2], t[3]);
            }
          }
        }
      }
      if constexpr (FUSE != 2) return;
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partial stores have left before the block is counted in
    }
  }
  if (!FUSE || wave < kAttnWaves) {   // ---- the attention waves (FUSE == 2: the o_proj waves skip to the arrival protocol below)
  // Several rows: the query heads of one KV group (and a row's segments) are neighbours in the natural block order, but
  // consecutive block ids go to the 8 XCDs round-robin, so each of a group's 7 heads would pull the same K/V rows into a
  // different L2.  Re-number: XCD x works through the x-th contiguous eighth of the natural order.
  unsigned bid = blockIdx.x;
  if (ONE != 1) {
    const unsigned total = (unsigned)p.work_blocks, xcd = bid & 7u, slot = bid >> 3, q8 = total >> 3, r8 = total & 7u;
    bid = xcd * q8 + (xcd < r8 ? xcd : r8) + slot;
  }
  const int head = (FUSE == 2 || AHOT) ? f_head : ONE == 1 ? (FUSE ? (int)bid % p.n_heads : (int)bid) : ONE == 2 ? (int)bid % p.n_heads : (int)(bid / p.nseg) % p.n_heads,
            m = FUSE == 2 ? f_row : ONE == 1 ? 0 : ONE == 2 ? (int)bid / p.n_heads : (int)bid / (p.nseg * p.n_heads),
            seg = ONE ? 0 : (int)bid % p.nseg;
  const int tl = lane / LPT, dl = lane % LPT;
  const int grp = wave * TPW + tl;
  const RowDesc rd = p.rows[m];
  const int kvh = AHOT ? a_kvh : head / p.group;
  // decode rows use slot == row, so the K/V addresses do not depend on the descriptor and the first
  // chunk's loads leave together with it (positions beyond ctx are valid cache memory, masked later)
  const bool sir = ONE || p.slot_is_row;
  const int slot = sir ? m : rd.slot;
  const size_t rowbase = ((size_t)slot * p.n_kv + kvh) * p.max_pos;
  const int ctx_all = rd.pos + 1;
  int ctx = ctx_all < (seg + 1) * kAttnSeg ? ctx_all : (seg + 1) * kAttnSeg;   // this block: keys [seg * kAttnSeg, ctx)
  if (!ONE && seg * kAttnSeg >= ctx_all) return;   // block-uniform: this row has no such segment (ONE: a single segment -- and no wait for the descriptor before the q / K / V loads are requested)

  // q is requested here but first USED after the chunk's K/V loads have been requested (the scaling sits in the loop behind
  // an opaque asm so that it is not hoisted back): descriptor, q and the first K/V chunk share one memory round trip
  // instead of queueing up as descriptor -> q -> K/V
  float qraw[DPL];
  {
    const float* qp = p.q + (size_t)m * p.q_dim + head * kHeadDim + dl * DPL;
#pragma unroll
    for (int i = 0; i < DPL; ++i) qraw[i] = qp[i];
  }
  float m_run = NEG, lrun = 0.f, o[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) o[i] = 0.f;

  int c0 = seg * kAttnSeg;
  do {   // block-uniform trip count; the first chunk never waits for ctx before its loads
    uint4 kr[UNR], vr[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = c0 + u * NGRP + grp;
      const int tc = sir ? (t < p.max_pos ? t : p.max_pos - 1) : (t < ctx ? t : ctx - 1);
      if constexpr (AHOT && !PG) {   // the (slot 0, KV head) row's base is a scalar; a token's piece is a 32-bit offset from it
        constexpr uint32_t ES = KVF32 ? 4u : 2u;   // (max_pos * 64 * ES < 2^32: smi_llm_create leaves fuse_o off beyond kFuseMaxPos positions)
        const uint32_t o = ((uint32_t)tc * kHeadDim + (uint32_t)(dl * DPL)) * ES;
        kr[u] = *(const uint4*)((const unsigned char*)p.kcache + rowbase * (kHeadDim * ES) + o);
        vr[u] = *(const uint4*)((const unsigned char*)p.vcache + rowbase * (kHeadDim * ES) + o);
        continue;
      }
      const size_t off = ((ONE && !PG) ? rowbase + tc : kv_row(p.km, slot, kvh, p.n_kv, p.max_pos, tc)) * kHeadDim + dl * DPL;
      if (KVF32) {
        kr[u] = *(const uint4*)((const float*)p.kcache + off);
        vr[u] = *(const uint4*)((const float*)p.vcache + off);
      } else {
        kr[u] = *(const uint4*)((const uint16_t*)p.kcache + off);
        vr[u] = *(const uint4*)((const uint16_t*)p.vcache + off);
      }
    }
    if (ONE) {   // the descriptor is first looked at here, behind the loads above (same opaque-asm device as for q below)
      int pr = rd.pos;
      asm volatile("" : "+v"(pr));
      ctx = pr + 1 < kAttnSeg ? pr + 1 : kAttnSeg;
    }
    float qv[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      float t = qraw[i];
      asm volatile("" : "+v"(t));
      qv[i] = t * 0.125f;  // head_dim^-0.5, exact
    }
    float sc[UNR];
    float lmax = NEG;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const uint32_t ku[4] = {kr[u].x, kr[u].y, kr[u].z, kr[u].w};
      float d = 0.f;
      if (KVF32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) d += qv[i % DPL] * __uint_as_float(ku[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d += qv[(2 * i) % DPL] * __uint_as_float(ku[i] << 16);
          d += qv[(2 * i + 1) % DPL] * __uint_as_float(ku[i] & 0xffff0000u);
        }
      }
      d = KVF32 ? smi_sum16(d) : smi_sum8(d);
      sc[u] = (c0 + u * NGRP + grp < ctx) ? d : NEG;
      lmax = fmaxf(lmax, sc[u]);
    }
    // wave max: inside a 16-lane row on the DPP path, across the four rows by readlane
    lmax = fmaxf(lmax, smi_dpp<0x128>(lmax));   // row_ror:8
    const float wm = fmaxf(fmaxf(smi_readlane(lmax, 0), smi_readlane(lmax, 16)), fmaxf(smi_readlane(lmax, 32), smi_readlane(lmax, 48)));
    // running max per WAVE (wave-uniform, no LDS, no barrier in the chunk loop); the waves' streams are brought to a
    // common scale once, in the final merge
    const float mn = fmaxf(m_run, wm);
    const float a = exp2f((m_run - mn) * LOG2E);
    lrun *= a;
#pragma unroll
    for (int i = 0; i < DPL; ++i) o[i] *= a;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const float e = sc[u] > 0.5f * NEG ? exp2f((sc[u] - mn) * LOG2E) : 0.f;
      const uint32_t vu[4] = {vr[u].x, vr[u].y, vr[u].z, vr[u].w};
      lrun += e;
      if (KVF32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i % DPL] += e * __uint_as_float(vu[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[(2 * i) % DPL] += e * __uint_as_float(vu[i] << 16);
          o[(2 * i + 1) % DPL] += e * __uint_as_float(vu[i] & 0xffff0000u);
        }
      }
    }
    m_run = mn;
    c0 += NGRP * UNR;
  } while (c0 < ctx);
  // every stream of a wave is at that wave's scale exp(-m_run): plain sums in fixed order inside the wave (step 1);
  // across the waves (step 2) each wave's sums are rescaled to the block maximum.
#pragma unroll
  for (int i = 0; i < DPL; i += 4)
    *(float4*)&so[wave][tl][dl * DPL + i] = make_float4(o[i], o[i + 1], o[i + 2], o[i + 3]);
  if (dl == 0) sl[wave][tl] = lrun;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own LDS writes have landed
  {
    float O = 0.f, Ls = 0.f;
#pragma unroll
    for (int g = 0; g < TPW; ++g) { O += so[wave][g][lane]; Ls += sl[wave][g]; }
    pw[wave][lane] = O;
    if (lane == 0) { pl[wave] = Ls; wmax[wave] = m_run; }
  }
  __syncthreads();
  if constexpr (FUSE == 1) return;   // step 2 runs in each o_proj wave (attn_merge_split), the attention waves are done
  if (tid < kHeadDim) {   // step 2, across the waves
    if (!ONE && p.nseg > 1) {   // segment partial at scale exp(-bm); k_attn_merge finishes the row
      float bm, O, Ls;
      attn_merge(wmax, pw, pl, tid, bm, O, Ls);
      float* pp = p.part + (((size_t)m * p.n_heads + head) * p.nseg + seg) * 66;
      pp[2 + tid] = O;
      if (tid == 0) { pp[0] = bm; pp[1] = Ls; }
      return;
    }
    uint32_t hi, mi, lo;
    attn_merge_split(wmax, pw, pl, tid, hi, mi, lo);
    if constexpr (FUSE) {
      attn_put_pieces(xsl, tid, hi, mi, lo);
    } else {
      const int Mx = ONE == 1 ? 1 : p.M;
      const size_t ob = xs_off(o_ktile(head, tid, p.n_heads), 0, (tid >> 3) & 3, m, Mx) + (tid & 7) * 2;
      const size_t pl2 = (size_t)4 * Mx * 16;
      *(uint16_t*)(p.xs_out + ob) = (uint16_t)hi;
      *(uint16_t*)(p.xs_out + ob + pl2) = (uint16_t)mi;
      *(uint16_t*)(p.xs_out + ob + 2 * pl2) = (uint16_t)lo;
    }
  }
  if constexpr (FUSE == 2) __syncthreads();   // the o_proj waves take over: xsl holds this head's output
  }   // attention waves
  if constexpr (FUSE == 2) {
    __syncthreads();                          // every o_proj wave of this block has drained its partial stores (vmcnt(0) above)
    unsigned int* cnt = p.cnt + f_row * kFuseQB + f_q;
    if (tid == 0) s_last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(p.n_heads - 1);
    __syncthreads();                          // (the adding lane joins only after its add has returned)
    if (!s_last) return;                      // block-uniform
    const int H = p.NTo * 16, ncol4 = H / kFuseQB / 4;     // float4 column groups of this quarter (56 at 0.5B)
    if (tid < ncol4) {
      const int n = f_q * (H / kFuseQB) + 4 * tid, m = f_row, M = p.M;
      // the heads in order (k_gemm<RESID, NW = n_heads>'s wave order, k_gemm<PRO_FUSEDO>'s partial order), every read an sc1 load
      // (ALL reads are requested before the first is used: as a loop over the heads they were 14 dependent memory round trips --
      // write-through stores leave no copy in any L2 -- and the kernel took 17 us at 8 rows)
      uint32_t pv[kMaxOHeads][4];
#pragma unroll
      for (int hd = 0; hd < kMaxOHeads; ++hd) {
        const uint32_t* src = (const uint32_t*)(p.part_o + ((size_t)m * p.n_heads + (hd < p.n_heads ? hd : p.n_heads - 1)) * H + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) pv[hd][r] = __hip_atomic_load(src + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = __uint_as_float(pv[0][r]);
#pragma unroll
      for (int hd = 1; hd < kMaxOHeads; ++hd)
        if (hd < p.n_heads) {   // uniform
#pragma unroll
          for (int r = 0; r < 4; ++r) y[r] += __uint_as_float(pv[hd][r]);
        }
      // k_gemm's RESID epilogue for row m, columns n .. n + 3
      const float4 egam = *(const float4*)(p.gamma_next + n);
      float4 h = *(const float4*)(p.h + (size_t)m * H + n);
      h.x += y[0]; h.y += y[1]; h.z += y[2]; h.w += y[3];
      *(float4*)(p.h + (size_t)m * H + n) = h;
      const float ssq = (h.x * h.x + h.y * h.y) + (h.z * h.z + h.w * h.w);
      const float t[4] = {egam.x * h.x, egam.y * h.y, egam.z * h.z, egam.w * h.w};
      uint32_t hi[4], mi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) split3(t[e], hi[e], mi[e], lo[e]);
      const size_t o = xs_off(n >> 5, 0, (n >> 3) & 3, m, M) + ((n >> 2) & 1) * 8;
      const size_t pl = (size_t)4 * M * 16;
      *(uint2*)(p.xs_next + o) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
      *(uint2*)(p.xs_next + o + pl) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
      *(uint2*)(p.xs_next + o + 2 * pl) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
      p.ssout[((size_t)m * p.NTo + (n >> 4)) * 4 + ((n >> 2) & 3)] = ssq;
    }
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
  }
}
template <int KVF32, int ONE = 0, int FUSE = 0, int PG = 0>
__global__ __launch_bounds__((FUSE ? 2 : 1) * kAttnWaves * 64) void k_attn(AttnP p) {
  if constexpr (ONE == 1) {
    // one row: every 64-byte line of kernel arguments the block reads is requested at entry, together (the compiler asked
    // for them one after the other -- the helper test, then q / K / V's addresses -- three scalar round trips in a row in
    // front of the first global load)
    if constexpr (FUSE) asm volatile("" ::"s"(p.q), "s"(p.work_blocks), "s"(p.Wo), "s"(gridDim.x));
    else asm volatile("" ::"s"(p.q), "s"(p.work_blocks), "s"(gridDim.x));
  }
  attn_body<KVF32, ONE, FUSE, PG>(p);
}
// Hot entry of the one-row fused attention + o_proj (contiguous KV slots), 14 dwords: the descriptor, q, K, V and W_o
// addresses, the helper test and the ints of the address arithmetic (hg = n_heads | group << 16: one dword for two small counts)
template <int KVF32>
__global__ __launch_bounds__(2 * kAttnWaves * 64) void k_attn_hot(const float* q, const void* kcache, const void* vcache, const RowDesc* rows,
                                                                  const uint4* Wo, int work_blocks, int max_pos, int NTo, int hg, AttnP p) {
  AttnP a = p;
  a.q = q; a.kcache = kcache; a.vcache = vcache; a.rows = rows; a.Wo = Wo; a.work_blocks = work_blocks; a.max_pos = max_pos; a.NTo = NTo;
  a.n_heads = hg & 0xffff; a.group = hg >> 16;
  attn_body<KVF32, 1, 1, 0>(a);
}
template <int KVF32>
void launch_attn_hot(const AttnP& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL(k_attn_hot<KVF32>, dim3(grid), dim3(2 * kAttnWaves * 64), 0, st, a.q, a.kcache, a.vcache, a.rows, a.Wo, a.work_blocks,
                     a.max_pos, a.NTo, a.n_heads | (a.group << 16), a);
}

// Prompt rows (prefill of more than one chunk): one WAVE per (row, head), eight consecutive rows of one head per
// block.  A prompt row's context is short on average (half the prompt) and thousands of rows arrive together, so the
// decode kernel's shape -- eight waves and two barriers around one 256-token chunk -- is mostly idle lanes and merge
// overhead there (199 us per layer for 32 x 127 rows).  Here a wave walks its row's keys 32 (bf16 KV) at a time
// with the same per-token arithmetic, keeps its own running max, and merges its token streams through a private LDS
// slice; nothing is shared between waves, so there is no barrier and no context segmentation.  Neighbouring rows of
// a sequence read the same K/V lines out of L1/L2.
template <int KVF32>
__global__ __launch_bounds__(kAttnWaves * 64) void k_attn_pf(AttnP p) {
  constexpr int LPT = KVF32 ? 16 : 8;
  constexpr int DPL = kHeadDim / LPT;
  constexpr int TPW = 64 / LPT;
  constexpr int UNR = 4;
  constexpr float NEG = -1e30f;
  constexpr float LOG2E = 1.4426950408889634f;
  __shared__ __attribute__((aligned(16))) float so[kAttnWaves][TPW][kHeadDim];
  __shared__ float sl[kAttnWaves][TPW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // natural order: the 14 heads of a row tile are neighbours; XCD x takes the x-th contiguous eighth of it (see k_attn)
  const unsigned total = gridDim.x * gridDim.y, pb = blockIdx.x + gridDim.x * blockIdx.y;
  const unsigned lb = (pb & 7u) * (total >> 3) + ((pb & 7u) < (total & 7u) ? (pb & 7u) : (total & 7u)) + (pb >> 3);
  const int head = (int)(lb % gridDim.y), m = (int)(lb / gridDim.y) * kAttnWaves + wave;
  if (m >= p.M) return;   // wave-uniform; the kernel has no barrier
  const int tl = lane / LPT, dl = lane % LPT;
  const RowDesc rd = p.rows[m];
  const int kvh = head / p.group;
  const int ctx = rd.pos + 1;
  float qv[DPL];
  {
    const float* qp = p.q + (size_t)m * p.q_dim + head * kHeadDim + dl * DPL;
#pragma unroll
    for (int i = 0; i < DPL; ++i) qv[i] = qp[i] * 0.125f;  // head_dim^-0.5, exact
  }
  float m_run = NEG, lrun = 0.f, o[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) o[i] = 0.f;
  for (int c0 = 0; c0 < ctx; c0 += TPW * UNR) {
    uint4 kr[UNR], vr[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int t = c0 + u * TPW + tl;
      const size_t off = kv_row(p.km, rd.slot, kvh, p.n_kv, p.max_pos, t < ctx ? t : ctx - 1) * kHeadDim + dl * DPL;
      if (KVF32) {
        kr[u] = *(const uint4*)((const float*)p.kcache + off);
        vr[u] = *(const uint4*)((const float*)p.vcache + off);
      } else {
        kr[u] = *(const uint4*)((const uint16_t*)p.kcache + off);
        vr[u] = *(const uint4*)((const uint16_t*)p.vcache + off);
      }
    }
    float sc[UNR];
    float lmax = NEG;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const uint32_t ku[4] = {kr[u].x, kr[u].y, kr[u].z, kr[u].w};
      float d = 0.f;
      if (KVF32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) d += qv[i % DPL] * __uint_as_float(ku[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d += qv[(2 * i) % DPL] * __uint_as_float(ku[i] << 16);
          d += qv[(2 * i + 1) % DPL] * __uint_as_float(ku[i] & 0xffff0000u);
        }
      }
      d = KVF32 ? smi_sum16(d) : smi_sum8(d);
      sc[u] = (c0 + u * TPW + tl < ctx) ? d : NEG;
      lmax = fmaxf(lmax, sc[u]);
    }
    lmax = fmaxf(lmax, smi_dpp<0x128>(lmax));   // row_ror:8
    const float wm = fmaxf(fmaxf(smi_readlane(lmax, 0), smi_readlane(lmax, 16)), fmaxf(smi_readlane(lmax, 32), smi_readlane(lmax, 48)));
    const float mn = fmaxf(m_run, wm);
    const float a = exp2f((m_run - mn) * LOG2E);
    lrun *= a;
#pragma unroll
    for (int i = 0; i < DPL; ++i) o[i] *= a;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const float e = sc[u] > 0.5f * NEG ? exp2f((sc[u] - mn) * LOG2E) : 0.f;
      const uint32_t vu[4] = {vr[u].x, vr[u].y, vr[u].z, vr[u].w};
      lrun += e;
      if (KVF32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i % DPL] += e * __uint_as_float(vu[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[(2 * i) % DPL] += e * __uint_as_float(vu[i] << 16);
          o[(2 * i + 1) % DPL] += e * __uint_as_float(vu[i] & 0xffff0000u);
        }
      }
    }
    m_run = mn;
  }
  // the wave's token streams are all at scale exp(-m_run): plain sums in fixed order
#pragma unroll
  for (int i = 0; i < DPL; i += 4)
    *(float4*)&so[wave][tl][dl * DPL + i] = make_float4(o[i], o[i + 1], o[i + 2], o[i + 3]);
  if (dl == 0) sl[wave][tl] = lrun;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own LDS writes have landed
  float O = 0.f, Ls = 0.f;
#pragma unroll
  for (int g = 0; g < TPW; ++g) { O += so[wave][g][lane]; Ls += sl[wave][g]; }
  uint32_t hi, mi, lo;
  split3(O / Ls, hi, mi, lo);
  const size_t ob = xs_off(o_ktile(head, lane, p.n_heads), 0, (lane >> 3) & 3, m, p.M) + (lane & 7) * 2;
  const size_t pl2 = (size_t)4 * p.M * 16;
  *(uint16_t*)(p.xs_out + ob) = (uint16_t)hi;
  *(uint16_t*)(p.xs_out + ob + pl2) = (uint16_t)mi;
  *(uint16_t*)(p.xs_out + ob + 2 * pl2) = (uint16_t)lo;
}


// ------------------------------------------------------------------------------------------
// Prefill attention on the matrix pipes (bf16 KV cache): one wave per (tile of up to 16 consecutive rows of one prompt,
// head).  k_attn_pf gives every (row, head) its own wave, which re-reads the head's K/V for every row (8 x 460-token prompts:
// 3 GB of L2 traffic and 210 us per layer, the largest prefill kernel there); here the 16 queries of a tile share each K/V load.
//   scores, transposed: S^T[key][query] = K (A operand: a key's 8 consecutive dims per lane, straight from the cache row) x
//     q^T (B operand: the query's dims, fp32 -> exact bf16 triple, three MFMAs lo/mid/hi) -- v_mfma_f32_16x16x32_bf16;
//   its accumulator layout (lane (g, query): keys 4g .. 4g+3) IS the A operand layout of v_mfma_f32_16x16x4_f32 over those
//     keys, so P = exp2((S - max) log2 e) feeds P x V in fp32 with no shuffle; V rows are read as they lie (lane (g, n): dims
//     4n .. 4n+3 of key 4g + t), output column n of tile d standing for dim 4n + d.
// Two passes over the keys (row maxima, then P and P x V: the scores are recomputed bit for bit), so no running rescale;
// causal mask key <= query position; per query the sum of P and the division happen once at the end.
// ------------------------------------------------------------------------------------------
struct PfTile { int32_t m0, n, slot, pos0; };   // rows m0 .. m0+n-1 are tokens pos0 .. pos0+n-1 of KV slot `slot`

__global__ __launch_bounds__(256) void k_attn_pf2(AttnP p, const PfTile* tiles, int ntiles) {
  constexpr float NEG = -1e30f;
  constexpr float LOG2E = 1.4426950408889634f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int task = (int)blockIdx.x * 4 + wave;
  const int ti = task / p.n_heads, head = task - ti * p.n_heads;
  if (ti >= ntiles) return;   // wave-uniform; the kernel has no barrier
  const PfTile t = tiles[ti];
  const int g = lane >> 4, j = lane & 15;
  const int kvh = head / p.group;
  const uint16_t* Kc = (const uint16_t*)p.kcache;
  const uint16_t* Vc = (const uint16_t*)p.vcache;
  // q^T operand: query j's dims s*32 + g*8 .. +8, scaled by head_dim^-0.5 (exact), as bf16 triples
  bf16x8 qh[2], qm[2], ql[2];
  {
    const float* qp = p.q + (size_t)(t.m0 + (j < t.n ? j : t.n - 1)) * p.q_dim + head * kHeadDim + g * 8;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const float4 a = *(const float4*)(qp + s2 * 32), b = *(const float4*)(qp + s2 * 32 + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      uint32_t hi[8], mi[8], lo[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) split3(v[e] * 0.125f, hi[e], mi[e], lo[e]);
      const uint4 H = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
      const uint4 Mi = make_uint4(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16), mi[4] | (mi[5] << 16), mi[6] | (mi[7] << 16));
      const uint4 Lo = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
      qh[s2] = __builtin_bit_cast(bf16x8, H); qm[s2] = __builtin_bit_cast(bf16x8, Mi); ql[s2] = __builtin_bit_cast(bf16x8, Lo);
    }
  }
  const int nkeys = t.pos0 + t.n;                 // keys 0 .. nkeys-1; query j sees keys <= pos0 + j
  const int nblk = (nkeys + 15) >> 4;
  const int qlast = t.pos0 + j;
  struct KReg { uint4 a, b; };
  auto kload = [&](int kb) -> KReg {              // A operand of block kb: this lane holds key kb*16 + j's dims g*8 .. +8 of both halves
    int key = kb * 16 + j;
    key = key < nkeys ? key : nkeys - 1;
    const uint16_t* kp = Kc + kv_row(p.km, t.slot, kvh, p.n_kv, p.max_pos, key) * kHeadDim + g * 8;
    return KReg{*(const uint4*)kp, *(const uint4*)(kp + 32)};
  };
  auto scores = [&](int kb, const KReg& kr) -> f32x4 {   // S^T block: lane (g, query j), register r: key kb*16 + 4g + r
    const bf16x8 k0 = __builtin_bit_cast(bf16x8, kr.a), k1 = __builtin_bit_cast(bf16x8, kr.b);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, ql[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, ql[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qm[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qm[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qh[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qh[1], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = (kb * 16 + 4 * g + r <= qlast) ? acc[r] : NEG;
    return acc;
  };
  // ---- pass 1: the queries' maxima (the next block's K rows are requested before this block's MFMAs)
  // (two register sets used in turn, two key blocks per trip: with one set and `kc = kn` at the end of a trip hipcc copies the registers
  // there and waits vmcnt(0) -- for the block it has just requested -- in front of the trip's last MFMA: round-4 ISA)
  float mx = NEG;
  {
    KReg ka = kload(0);
    for (int kb = 0; kb < nblk; kb += 2) {
      const KReg kbr = kload(kb + 1 < nblk ? kb + 1 : kb);
      const f32x4 sa = scores(kb, ka);
      mx = fmaxf(mx, fmaxf(fmaxf(sa[0], sa[1]), fmaxf(sa[2], sa[3])));
      ka = kload(kb + 2 < nblk ? kb + 2 : kb);
      if (kb + 1 < nblk) {
        const f32x4 sb = scores(kb + 1, kbr);
        mx = fmaxf(mx, fmaxf(fmaxf(sb[0], sb[1]), fmaxf(sb[2], sb[3])));
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // ---- pass 2: P and P x V
  f32x4 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float lsum = 0.f;
  struct VReg { uint2 v[4]; };
  auto vload = [&](int kb) -> VReg {
    VReg r;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      int key = kb * 16 + 4 * g + tt;
      key = key < nkeys ? key : nkeys - 1;
      r.v[tt] = *(const uint2*)(Vc + kv_row(p.km, t.slot, kvh, p.n_kv, p.max_pos, key) * kHeadDim + 4 * j);
    }
    return r;
  };
  auto pv = [&](int kb, const KReg& kr, const VReg& vr) {
    const f32x4 sc = scores(kb, kr);
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pr[r] = sc[r] > 0.5f * NEG ? exp2f((sc[r] - mx) * LOG2E) : 0.f;
      lsum += pr[r];
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const float v0 = __uint_as_float(vr.v[tt].x << 16), v1 = __uint_as_float(vr.v[tt].x & 0xffff0000u);
      const float v2 = __uint_as_float(vr.v[tt].y << 16), v3 = __uint_as_float(vr.v[tt].y & 0xffff0000u);
      o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[tt], v0, o[0], 0, 0, 0);
      o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[tt], v1, o[1], 0, 0, 0);
      o[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[tt], v2, o[2], 0, 0, 0);
      o[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[tt], v3, o[3], 0, 0, 0);
    }
  };
  KReg ka = kload(0);
  VReg va = vload(0);
  for (int kb = 0; kb < nblk; kb += 2) {     // sets A and B in turn (see pass 1); the key blocks are visited in the same order
    const int k1 = kb + 1 < nblk ? kb + 1 : kb, k2 = kb + 2 < nblk ? kb + 2 : kb;
    const KReg kbr = kload(k1);
    const VReg vbr = vload(k1);
    pv(kb, ka, va);
    ka = kload(k2);
    va = vload(k2);
    if (kb + 1 < nblk) pv(kb + 1, kbr, vbr);
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);               // lane (any g, j): the sum for query j
  // ---- output: lane (g, n) holds O[query 4g + r][dims 4n .. 4n+3] in o[0..3][r]
  const size_t pl2 = (size_t)4 * p.M * 16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = 4 * g + r;
    const float ls = __shfl(lsum, qi, 64);
    if (qi >= t.n) continue;
    uint32_t hi[4], mi[4], lo[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) split3(o[d][r] / ls, hi[d], mi[d], lo[d]);
    const size_t ob = xs_off(o_ktile(head, 4 * j, p.n_heads), 0, (j >> 1) & 3, t.m0 + qi, p.M) + (j & 1) * 8;
    *(uint2*)(p.xs_out + ob) = make_uint2(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16));
    *(uint2*)(p.xs_out + ob + pl2) = make_uint2(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16));
    *(uint2*)(p.xs_out + ob + 2 * pl2) = make_uint2(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16));
  }
}

// Combines a row's context segments in order (a row with one segment reproduces the unsplit result bit for bit:
// its scale factor is exp2(0) = 1).  One block per row, one thread per (head, dim).
__global__ __launch_bounds__(1024) void k_attn_merge(AttnP p) {
  constexpr float LOG2E = 1.4426950408889634f;
  const int m = blockIdx.x;
  const int ns = (p.rows[m].pos + 1 + kAttnSeg - 1) / kAttnSeg;
  for (int i = threadIdx.x; i < p.n_heads * kHeadDim; i += blockDim.x) {
    const int head = i / kHeadDim, d = i - head * kHeadDim;
    const float* pp = p.part + ((size_t)m * p.n_heads + head) * p.nseg * 66;
    float bm = pp[0];
    for (int s2 = 1; s2 < ns; ++s2) bm = fmaxf(bm, pp[s2 * 66]);
    float O = 0.f, Ls = 0.f;
    for (int s2 = 0; s2 < ns; ++s2) {
      const float sc = exp2f((pp[s2 * 66] - bm) * LOG2E);
      O += pp[s2 * 66 + 2 + d] * sc;
      Ls += pp[s2 * 66 + 1] * sc;
    }
    uint32_t hi, mi, lo;
    split3(O / Ls, hi, mi, lo);
    const size_t ob = xs_off(o_ktile(head, d, p.n_heads), 0, (d >> 3) & 3, m, p.M) + (d & 7) * 2;
    const size_t pl2 = (size_t)4 * p.M * 16;
    *(uint16_t*)(p.xs_out + ob) = (uint16_t)hi;
    *(uint16_t*)(p.xs_out + ob + pl2) = (uint16_t)mi;
    *(uint16_t*)(p.xs_out + ob + 2 * pl2) = (uint16_t)lo;
  }
}

// ------------------------------------------------------------------------------------------
// Token -> residual row.  One wave per row: gathers the embedding row from the tiled lm_head (tied
// weights), writes h (fp32), the first norm's operand (exact triples of gamma * h) and the row's
// sum of squares (partial slot 0; the other slots are zeroed so consumers sum a fixed count).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void embed_row(const uint16_t* Wlm, int KT, int token, int m, int M, const float* gamma,
                                          float* h, unsigned char* xs, float* sspart, int npart, int lane) {
  const int K = KT * 32, pieces = KT * 4;
  float ss = 0.f;
  for (int pc = lane; pc < pieces; pc += 64) {      // pc = k / 8
    const size_t tile = (size_t)(token >> 4) * KT + (pc >> 2);
    const uint4 v = *(const uint4*)(Wlm + tile * 512 + ((pc & 3) * 16 + (token & 15)) * 8);
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = __uint_as_float(u[e] << 16); x[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u); }
    float* dst = h + (size_t)m * K + pc * 8;
    *(float4*)dst = make_float4(x[0], x[1], x[2], x[3]);
    *(float4*)(dst + 4) = make_float4(x[4], x[5], x[6], x[7]);
    const float4 g0 = *(const float4*)(gamma + pc * 8), g1 = *(const float4*)(gamma + pc * 8 + 4);
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    uint32_t hi[8], mi[8], lo[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ss += x[e] * x[e]; split3(g[e] * x[e], hi[e], mi[e], lo[e]); }
    const size_t o = xs_off(pc >> 2, 0, pc & 3, m, M);
    const size_t pl = (size_t)4 * M * 16;
    *(uint4*)(xs + o) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
    *(uint4*)(xs + o + pl) = make_uint4(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16), mi[4] | (mi[5] << 16), mi[6] | (mi[7] << 16));
    *(uint4*)(xs + o + 2 * pl) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
  }
  ss = smi_wave_sum(ss);
  for (int i = lane; i < npart; i += 64) sspart[(size_t)m * npart + i] = i == 0 ? ss : 0.f;
}

// Drops the rows of the retired KV slots from the live row list, in place and in order (one block; B <= 64 rows).
__global__ __launch_bounds__(64) void k_rows_drop(RowDesc* rows, int B, unsigned long long drop_slots) {
  const int i = threadIdx.x;
  RowDesc rd = RowDesc{0, 0, 0, 0};
  bool keep = false;
  if (i < B) { rd = rows[i]; keep = !((drop_slots >> rd.slot) & 1ull); }
  const unsigned long long m = __ballot(keep);
  const int dst = __popcll(m & ((1ull << i) - 1ull));
  __syncthreads();   // (one wave: every row was read before any is overwritten)
  if (keep) rows[dst] = rd;
  else if (i < 64) { /* nothing: the tail beyond the new count is never read */ }
}

// Forked admission (smi_llm_admit_forked): copies cache positions [p0, p1) of a source slot into a destination slot, every
// layer, K and V, every kv head, for a flat work list of (src slot, dst slot, p0, p1) entries -- one per follower take.  A byte
// copy in 16-byte pieces addressed through KvMap on both sides, so bf16 / f32 and contiguous / paged caches run the same code.
// grid: x = (position, piece) of the longest entry, y = work entry, z = (layer, K / V, kv head).
struct ForkP {
  const int4* work;           // [gridDim.y] (src slot, dst slot, p0, p1)
  unsigned char* kcache;      // layer 0's K cache (layer l at + l * layer_bytes)
  unsigned char* vcache;
  size_t layer_bytes;
  int n_kv, max_pos;
  int piece_shift;            // log2(16-byte pieces per 64-element row): 3 (bf16) or 4 (f32)
  KvMap km;
};
__global__ __launch_bounds__(256) void k_kv_fork(ForkP p) {
  const int4 w = p.work[blockIdx.y];
  const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int pos = w.z + (u >> p.piece_shift), piece = u & ((1 << p.piece_shift) - 1);
  if (pos >= w.w) return;
  const int kvh = (int)blockIdx.z % p.n_kv, isv = ((int)blockIdx.z / p.n_kv) & 1, layer = (int)blockIdx.z / (2 * p.n_kv);
  unsigned char* base = (isv ? p.vcache : p.kcache) + (size_t)layer * p.layer_bytes;
  const size_t rb = (size_t)16 << p.piece_shift;   // bytes of one row
  const uint4* s = (const uint4*)(base + kv_row(p.km, w.x, kvh, p.n_kv, p.max_pos, pos) * rb) + piece;
  uint4* d = (uint4*)(base + kv_row(p.km, w.y, kvh, p.n_kv, p.max_pos, pos) * rb) + piece;
  *d = *s;
}

__global__ __launch_bounds__(256) void k_embed(const uint16_t* Wlm, int KT, const RowDesc* rows, int M, const float* gamma,
                                               float* h, unsigned char* xs, float* sspart, int npart, int exact) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int m = blockIdx.x * 4 + wave; m < M; m += gridDim.x * 4) {
    if (exact) embed_row_x((const float*)Wlm, KT, rows[m].token, m, M, gamma, h, xs, sspart, npart, lane);   // exact-weights arena: fp32 [vocab][K]
    else embed_row(Wlm, KT, rows[m].token, m, M, gamma, h, xs, sspart, npart, lane);
  }
}

#ifdef SMI_DIAG
// Tests (smi_llm_debug_layer): caller-given fp32 residual rows -> the state a layer starts from (h, the first norm's operand
// triples, the row's sum of squares in partial slot 0), exactly as embed_row leaves it for an embedding row.
__global__ __launch_bounds__(256) void k_load_hidden(const float* src, int KT, int M, const float* gamma, float* h, unsigned char* xs,
                                                     float* sspart, int npart) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = KT * 32;
  for (int m = blockIdx.x * 4 + wave; m < M; m += gridDim.x * 4) {
    float ss = 0.f;
    for (int pc = lane; pc < KT * 4; pc += 64) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = src[(size_t)m * K + pc * 8 + e];
      float* dst = h + (size_t)m * K + pc * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[e] = x[e];
      uint32_t hi[8], mi[8], lo[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { ss += x[e] * x[e]; split3(gamma[pc * 8 + e] * x[e], hi[e], mi[e], lo[e]); }
      const size_t o = xs_off(pc >> 2, 0, pc & 3, m, M);
      const size_t pl = (size_t)4 * M * 16;
      *(uint4*)(xs + o) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
      *(uint4*)(xs + o + pl) = make_uint4(mi[0] | (mi[1] << 16), mi[2] | (mi[3] << 16), mi[4] | (mi[5] << 16), mi[6] | (mi[7] << 16));
      *(uint4*)(xs + o + 2 * pl) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
    }
    ss = smi_wave_sum(ss);
    for (int i = lane; i < npart; i += 64) sspart[(size_t)m * npart + i] = i == 0 ? ss : 0.f;
  }
}
#endif

// ------------------------------------------------------------------------------------------
// Sampling (the reference's default: do_sample=True, top_k=50, top_p=0.95, temperature=0.8 at
// cli/SparkTTS.py:166-168,197-204).  Restates the HF warper chain: logits / T -> keep top k ->
// nucleus (drop the low tail whose cumulative probability <= 1 - top_p, keep >= 1) -> softmax ->
// one multinomial draw.  The draw uses a counter-based Philox4x32-10 stream keyed by
// (seed; the sequence's own token index, its admission number), so a run is reproducible but not
// bit-identical to torch.multinomial.  What a row does comes from its slot's record (Ctl::samp): the handle's settings
// (inherit), arg-max (greedy: the sampler kernels leave the row to k_finalize) or its own T / k / p and stream.
// ------------------------------------------------------------------------------------------
struct SampleP {
  const float* logits;  // [M][V]
  int V, top_k;         // top_k, inv_temp, top_p: the handle's settings (rows whose record inherits)
  float inv_temp, top_p;
  int hs;               // the handle samples (smi_llm_set_sampling(do_sample = 1))
  const Ctl* ctl;        // seed and the per-slot admission numbers
  const RowDesc* rows;   // the live rows: (slot, ..., flags = tokens this sequence has emitted so far)
  int* tok;             // [kMaxRows] sampled token per row
  const float* pval;    // [M][nblk] the lm_head blocks' best logits (a bound for the top-k threshold) or null
  int nblk;
  // candidates at or above the bound, collected by k_sample_scan: [kMaxRows][kCandCap] values / indices, [kMaxRows] counts
  float* cand_v; int* cand_i; unsigned int* cand_n;
};

// Order-preserving key of a float.  -0.0 takes +0.0's key: the bound path compares floats (v >= thr), to which the two zeros
// are equal, and TopKLogitsWarper (`scores < kth`) keeps both when they tie at the k-th value; a key of its own would put
// -0.0 below a +0.0 threshold on the radix path alone.  No other float's key changes.
__device__ __forceinline__ uint32_t sortable(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ inline uint32_t philox_u32(unsigned long long seed, uint32_t c0, uint32_t c1) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t x0 = c0, x1 = c1, x2 = 0x5eed5eedu, x3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * x0, p1 = (unsigned long long)0xCD9E8D57u * x2;
    const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1;
    const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
    x0 = y0; x1 = y1; x2 = y2; x3 = y3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return x0;
}

constexpr int kSampleCap = 256;  // top_k upper bound
constexpr uint32_t kSeededStream = 0xFFFFFFFFu;   // admission-number word of a seeded record's stream (admission numbers are < 2^31)

__device__ __forceinline__ bool rec_samples(const SampRec& r, int hs) {
  return r.mode == SMI_SAMPLING_SAMPLE || (r.mode == SMI_SAMPLING_INHERIT && hs);
}

// Row m's selection: on = it draws a token; its top_k / 1/T / top_p; the Philox key and the counter word beside the token index
struct RowSel {
  bool on;
  int top_k;
  float inv_temp, top_p;
  unsigned long long seed;
  uint32_t c1;
};
__device__ __forceinline__ RowSel row_sel(const SampleP& p, int m) {
  const int sl = p.rows[m].slot;
  const SampRec& r = p.ctl->samp[sl];
  RowSel s;
  s.on = rec_samples(r, p.hs);
  const bool own = r.mode == SMI_SAMPLING_SAMPLE;
  s.top_k = own ? r.top_k : p.top_k;
  s.inv_temp = own ? r.inv_temp : p.inv_temp;
  s.top_p = own ? r.top_p : p.top_p;
  const bool seeded = own && r.has_seed;
  s.seed = seeded ? r.seed : p.ctl->seed;
  s.c1 = seeded ? kSeededStream : (uint32_t)p.ctl->seqid[sl];
  return s;
}
constexpr int kCandCap = 1024;   // candidates at or above the threshold taken from the lm_head blocks' maxima

// Exact key of the k-th largest logit by 4 passes of 8-bit radix selection (fallback path: one block walks
// the whole row 4 times, with LDS-atomic histograms).
__device__ uint32_t radix_kth_key(const float* lg, int V, int top_k, unsigned int* hist, unsigned int* s_prefix, unsigned int* s_need) {
  const int tid = threadIdx.x;
  if (tid == 0) { *s_prefix = 0; *s_need = (unsigned)top_k; }
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = *s_prefix;
    const uint32_t mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
    for (int i = tid; i < V; i += 1024) {
      const uint32_t k = sortable(lg[i]);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned need = *s_need;
      int b = 255;
      for (; b > 0; --b) {
        if (hist[b] >= need) break;
        need -= hist[b];
      }
      *s_need = need;                       // rank inside bin b
      *s_prefix = prefix | ((uint32_t)b << shift);
    }
    __syncthreads();
  }
  return *s_prefix;
}

constexpr int kScanBlocks = 16;  // blocks per row in k_sample_scan

// The top_k-th largest of the lm_head blocks' maxima is a lower bound of the top_k-th largest logit (those maxima are
// top_k distinct logits at or above it), so ONE pass over the row collects a short candidate list that contains the
// whole top-k.  kScanBlocks blocks per row share that pass (one CU pulls a 664 KB row at ~150 GB/s: 25 us for a
// single block); each finds the bound itself and appends its candidates to the row's global list.  The list order
// depends on the race, the result does not: k_sample rank-sorts the list by (value, index).
__global__ __launch_bounds__(256) void k_sample_scan(SampleP p) {
  __shared__ float s_thr;
  const int m = blockIdx.y, tid = threadIdx.x;
  const RowSel rs = row_sel(p, m);   // per row: greedy rows leave at once, and the bound path is chosen by the row's own top_k
  if (!rs.on || !(p.pval && p.nblk <= kCandCap && p.nblk >= rs.top_k)) return;   // no usable bound: k_sample selects by radix
  // the bound, by ONE wave: each lane holds up to 16 of the (<= 1024) maxima as order-preserving keys and the answer is
  // built bit by bit from ballots (K = max{x : #{keys >= x} >= top_k}) -- no LDS, no barrier
  if (tid < 64) {
    uint32_t key[kCandCap / 64];
#pragma unroll
    for (int i = 0; i < kCandCap / 64; ++i) {
      const int j = tid + 64 * i;
      key[i] = j < p.nblk ? sortable(p.pval[(size_t)m * p.nblk + j]) : 0u;   // 0 sorts below every float
    }
    uint32_t K = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t t = K | (1u << bit);
      int c = 0;
#pragma unroll
      for (int i = 0; i < kCandCap / 64; ++i)
        if (i * 64 < p.nblk) c += __popcll(__ballot(key[i] >= t));   // uniform: slots beyond nblk hold no key
      if (c >= rs.top_k) K = t;   // wave-uniform
    }
    if (tid == 0) s_thr = __uint_as_float((K & 0x80000000u) ? (K ^ 0x80000000u) : ~K);
  }
  __syncthreads();
  const float thr = s_thr;
  const float* lg = p.logits + (size_t)m * p.V;
  // (a -inf logit has probability 0 and is never a candidate: a row with fewer than top_k finite logits -- a constrained row,
  // smi_llm_admit_constrained -- has the bound -inf, and its -inf ids would otherwise crowd the finite ones out of the list)
  auto take = [&](float v, int idx) {
    if (v >= thr && v != -INFINITY) {
      const unsigned pos = atomicAdd(&p.cand_n[m], 1u);
      if (pos < (unsigned)kCandCap) { p.cand_v[(size_t)m * kCandCap + pos] = v; p.cand_i[(size_t)m * kCandCap + pos] = idx; }
    }
  };
  if ((p.V & 3) == 0) {
    const float4* l4 = (const float4*)lg;
    const int n4 = p.V / 4, per = (n4 + kScanBlocks - 1) / kScanBlocks;
    const int lo = (int)blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
    constexpr int UL = 4;   // loads in flight per thread
    for (int base = lo; base < hi; base += 256 * UL) {
      float4 v[UL];
#pragma unroll
      for (int u = 0; u < UL; ++u) {
        const int i = base + u * 256 + tid;
        v[u] = i < hi ? l4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int u = 0; u < UL; ++u) {
        const int i = base + u * 256 + tid;
        take(v[u].x, 4 * i); take(v[u].y, 4 * i + 1); take(v[u].z, 4 * i + 2); take(v[u].w, 4 * i + 3);
      }
    }
  } else {
    const int per = (p.V + kScanBlocks - 1) / kScanBlocks;
    const int lo = (int)blockIdx.x * per, hi = lo + per < p.V ? lo + per : p.V;
    for (int i = lo + tid; i < hi; i += 256) take(lg[i], i);
  }
}

// One block per row: takes the candidates k_sample_scan collected (without a usable bound, or with more than kCandCap of
// them, it selects the top_k-th key exactly by radix and walks the row itself); the candidates are rank-sorted exactly
// (value descending, index ascending on ties), then temperature -> top-k -> top-p -> multinomial.
__global__ __launch_bounds__(1024) void k_sample(SampleP p) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_prefix, s_need, s_cnt;
  __shared__ int s_k;
  __shared__ float s_thr;
  __shared__ float cv[kCandCap], sv[kSampleCap];
  __shared__ int ci[kCandCap], si[kSampleCap];
  const int m = blockIdx.x, tid = threadIdx.x;
  const RowSel rs = row_sel(p, m);
  if (!rs.on) return;   // greedy row: k_finalize takes its arg-max
  const float* lg = p.logits + (size_t)m * p.V;
  if (tid == 0) { s_cnt = 0; s_thr = -INFINITY; s_k = 0; }
  __syncthreads();
  const bool bound_ok = p.pval && p.nblk <= kCandCap && p.nblk >= rs.top_k;   // the condition k_sample_scan ran under
  if (bound_ok) {
    if (tid == 0) { s_cnt = p.cand_n[m]; p.cand_n[m] = 0; s_thr = 0.f; }   // the counter is left at zero for the next step
    __syncthreads();
    const unsigned ng = s_cnt;
    if (ng <= (unsigned)kCandCap && tid < (int)ng) {
      cv[tid] = p.cand_v[(size_t)m * kCandCap + tid];
      ci[tid] = p.cand_i[(size_t)m * kCandCap + tid];
    }
    __syncthreads();
  }
  const float thr0 = s_thr;
  if (thr0 == -INFINITY || s_cnt > (unsigned)kCandCap) {
    // no usable bound (or a pathological row with > 1024 logits above it): exact radix selection of the k-th key
    __syncthreads();
    const uint32_t thr = radix_kth_key(lg, p.V, rs.top_k, hist, &s_prefix, &s_need);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid; i < p.V; i += 1024) {
      const float v = lg[i];
      if (sortable(v) >= thr && v != -INFINITY) {   // (-inf: probability 0, as in k_sample_scan)
        const unsigned pos = atomicAdd(&s_cnt, 1u);
        if (pos < kCandCap) { cv[pos] = v; ci[pos] = i; }
      }
    }
    __syncthreads();
  }
  const int n = s_cnt < (unsigned)kCandCap ? (int)s_cnt : kCandCap;
  // rank sort: descending value, ascending index on ties; only the first top_k ranks are kept
  if (tid < n) {
    const float v = cv[tid];
    const int ix = ci[tid];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (cv[j] > v) || (cv[j] == v && ci[j] < ix);
    if (r < kSampleCap) { sv[r] = v; si[r] = ix; }
  }
  __syncthreads();
  // TopKLogitsWarper removes what is strictly BELOW the k-th largest value (logits_process.py: `scores < topk[..., -1]`), so
  // every logit that ties with the k-th stays: the kept set is the sorted prefix of ranks < top_k plus the ranks behind it
  // that hold the same value (up to the kSampleCap ranks this kernel sorts)
  {
    const int nn = n < kSampleCap ? n : kSampleCap, kb = n < rs.top_k ? n : rs.top_k;
    if (tid < nn && (tid < kb || sv[tid] == sv[kb - 1])) atomicAdd(&s_k, 1);
  }
  __syncthreads();
  const int ktop = s_k;
  {   // softmax numerators of the top-k of logits / T (fp32, like the warpers), one per thread
    const int k = ktop;
    float e = 0.f;
    if (tid < k) e = expf(sv[tid] * rs.inv_temp - sv[0] * rs.inv_temp);
    __syncthreads();   // cv (the candidates) has been read by the rank sort
    if (tid < k) cv[tid] = e;
    __syncthreads();
  }
  // Nucleus cut and multinomial draw on ONE wave, four consecutive ranks per lane (top_k <= kSampleCap = 256): sums, suffix
  // sums and prefix sums come from shuffles instead of four serial loops with a division each on one thread (15 us).
  if (tid < 64) {
    static_assert(kSampleCap == 256, "four ranks per lane");
    const int k = ktop;
    const int i0 = tid * 4;
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = i0 + e < k ? cv[i0 + e] : 0.f;
    const float sum = smi_wave_sum((c[0] + c[1]) + (c[2] + c[3]));
    // token i is dropped when the probability mass from rank i on, sum_{j >= i} p_j, is <= 1 - top_p
    float sfx[4];
    sfx[3] = c[3] / sum;
    sfx[2] = c[2] / sum + sfx[3];
    sfx[1] = c[1] / sum + sfx[2];
    sfx[0] = c[0] / sum + sfx[1];
    float t = sfx[0];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float v = __shfl_down(t, d, 64);
      if (tid + d < 64) t += v;
    }
    float above = __shfl_down(t, 1, 64);   // mass of the lanes after this one
    if (tid == 63) above = 0.f;
    int best = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e >= 1 && i0 + e < k && sfx[e] + above > 1.0f - rs.top_p) best = i0 + e;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_xor(best, d, 64); best = v > best ? v : best; }
    const int keep = best + 1;   // rank 0 always stays
    // inverse-CDF draw over the kept ranks
    float pre[4];
    pre[0] = i0 < keep ? c[0] : 0.f;
    pre[1] = pre[0] + (i0 + 1 < keep ? c[1] : 0.f);
    pre[2] = pre[1] + (i0 + 2 < keep ? c[2] : 0.f);
    pre[3] = pre[2] + (i0 + 3 < keep ? c[3] : 0.f);
    float q = pre[3];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float v = __shfl_up(q, d, 64);
      if (tid >= d) q += v;
    }
    const float ksum = __shfl(q, 63, 64);
    float before = __shfl_up(q, 1, 64);
    if (tid == 0) before = 0.f;
    // one stream per SEQUENCE: (its admission number, its own token index) -- a request's draws do not depend on which
    // row it occupies, on what else is live or on when its neighbours were admitted; a seeded record: (its seed; its own
    // token index) -- nor on the admission order or the handle
    const RowDesc rd = p.rows[m];
    const uint32_t r = philox_u32(rs.seed, (uint32_t)rd.flags, rs.c1);
    const float u = (float)(r >> 8) * (1.0f / 16777216.0f) * ksum;
    int pick = keep - 1;
#pragma unroll
    for (int e = 3; e >= 0; --e)
      if (i0 + e < keep && u < before + pre[e]) pick = i0 + e;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_xor(pick, d, 64); pick = v < pick ? v : pick; }
    if (tid == 0) p.tok[m] = n > 0 ? si[pick] : 0;   // no finite logit (NaN weights / inputs): no candidate, token 0 as k_finalize's guard gives a greedy row
  }
}

// ------------------------------------------------------------------------------------------
// Logits penalties (smi_llm_admit_penalized; include/sparkmi.h states the semantics).  Per KV slot a history row
// uint16 [vocab]: bit 15 = the id is in the prompt, bits 0..14 = its count among the generated tokens (k_finalize adds one per
// token; 32 767 > max_positions, so it cannot saturate).  k_penalize runs between the lm_head and the sampler / k_finalize,
// on the logits rows the lm_head wrote: a penalised row's logits are processed (written back only when the row samples) and its
// nblk (value, id) maxima are rebuilt over the kernel's own partition of the vocabulary (set j = ids [j * per, (j + 1) * per)).
// k_finalize's arg-max and k_sample_scan's top-k bound hold for ANY partition into nblk disjoint sets; unpenalised rows leave
// at once and keep the lm_head's own maxima, so their bits do not change.
// ------------------------------------------------------------------------------------------
constexpr int kPenWaves = 4;   // sets per block: one wave per set

struct PenP {
  float* logits;          // [M][V] the lm_head's logits rows
  const uint16_t* hist;   // [max_slots][V]
  const Ctl* ctl;         // per-slot records, eos ids
  const RowDesc* rows;
  float* pval;            // [M][nblk]
  int* pidx;
  int V, nblk, per;       // per: ids per set, a multiple of 4 (per * nblk >= V)
  int hs;                 // the handle samples
  const SeqRec* seq;      // non-null (some live row has a bias entry): per-slot bias entries, stage 0b
  const int64_t* ghist;   // [max_steps][kMaxRows] generated tokens per slot (the context of stage 0b)
  int max_steps;
};

// Stage 0b (smi_llm_admit_biased) for one wave: lane e < n_bias takes entry e, decides whether it applies at this step (its first
// L - 1 ids against the context tail: the generated tokens, then the stored prompt tail) and adds up, for its last id, the
// applying entries' biases in the contract's order (the length-1 entry, then the longer ones in record order).  The first
// applying entry of every distinct id inside [i0, i1) then leaves (id, total) in the wave's LDS list; returns the list's length.
// *any: some entry of the row applies (the same in every wave of the row).
__device__ __forceinline__ int seq_bias_list(const SeqRec* sq, const RowDesc& rd, const int64_t* ghist, int max_steps, int lane,
                                             int i0, int i1, int* l_id, float* l_tot, bool* any) {
  const int nb = sq->n_bias, gen = rd.flags;
  bool app = false;
  int last = -1, len = 0;
  float bias = 0.f;
  if (lane < nb) {
    len = sq->blen[lane]; bias = sq->bias[lane]; last = sq->bids[lane][len - 1];
    app = len <= sq->plen + gen;
    for (int k = 1; k < len && app; ++k) {   // the context's k-th id from its end
      int c = -1;
      if (k <= gen) { if (gen - k < max_steps) c = (int)ghist[(size_t)(gen - k) * kMaxRows + rd.slot]; }
      else if (k - gen <= sq->n_ptail) c = sq->ptail[SMI_MAX_SEQ_LEN - 1 - (k - gen)];
      app = c == sq->bids[lane][len - 1 - k];
    }
  }
  const unsigned long long am = __ballot(app);
  *any = am != 0;
  if (!am) return 0;
  float tot = 0.f;
  bool first = true;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass)
    for (int f = 0; f < nb; ++f) {
      const int lf = __shfl(last, f, 64), nf = __shfl(len, f, 64);
      const float bf = __shfl(bias, f, 64);
      if (((am >> f) & 1ull) && lf == last) {
        if ((nf == 1) == (pass == 0)) tot += bf;
        if (f < lane) first = false;
      }
    }
  const bool own = app && first && last >= i0 && last < i1;
  const unsigned long long om = __ballot(own);
  if (own) {
    const int at = __popcll(om & ((1ull << lane) - 1ull));
    l_id[at] = last; l_tot[at] = tot;
  }
  __builtin_amdgcn_wave_barrier();
  return __popcll(om);
}

// stages 1..3 on one logit (fp32, each operation rounded on its own: the build compiles with -ffp-contract=off)
__device__ __forceinline__ float pen_logit(float x, uint32_t h, const PenRec& r, bool mask, int id, const int* eos) {
  const uint32_t c = h & 0x7fffu;
  if (c || (r.prompt && (h & 0x8000u))) x = x < 0.f ? x * r.rep : x / r.rep;
  x = x - (r.freq * (float)c + r.pres * (c ? 1.f : 0.f));
  if (mask) {
#pragma unroll
    for (int e = 0; e < SMI_MAX_EOS; ++e)
      if (id == eos[e]) x = -INFINITY;
  }
  return x;
}

__device__ __forceinline__ void pen_best(float v, int i, float& bv, int& bi) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// grid (ceil(nblk / kPenWaves), M) x 256: wave w of block x owns set x * kPenWaves + w of row blockIdx.y.  No barrier: a wave
// reads its set's logits and history entries once (float4 + 4 x uint16 when V % 4 == 0: sets start at multiples of 4), writes
// them back processed if the row samples, and leaves one (maximum, lowest id) pair.
// Stage 0 (smi_llm_admit_constrained) runs here too, first: a constrained row's ids outside its ranges become -inf (what the
// restricted lm_head leaves unwritten outside the union of the rows' tiles included), and the row's maxima are rebuilt over
// this kernel's partition -- so the sampler, k_logprob and k_finalize see the same dense row and the same maxima whichever
// lm_head form ran.  A constrained, unpenalised row takes stage 0 alone.
// Stage 0b (smi_llm_admit_biased) runs here as well, between stage 0 and the penalties: a row with bias entries takes this
// route, each wave works out the (id, total) pairs of its own set (seq_bias_list) and adds them as it passes the ids -- no extra
// pass over the row, nothing written that the row's consumers do not read, and the set's maximum is exact because it is taken
// after the add.  A row that has bias entries but none that applies at this step (and no other record) leaves like a plain row.
__global__ __launch_bounds__(256) void k_penalize(PenP p) {
  __shared__ int s_bid[kPenWaves][SMI_MAX_BIAS_SEQS];
  __shared__ float s_btot[kPenWaves][SMI_MAX_BIAS_SEQS];
  const int m = blockIdx.y;
  const RowDesc rd = p.rows[m];
  const PenRec r = p.ctl->pen[rd.slot];
  const AllowRec* al = &p.ctl->allow[rd.slot];
  const bool con = al->n > 0;
  const SeqRec* sq = p.seq ? &p.seq[rd.slot] : nullptr;
  const bool bia = sq && sq->n_bias > 0;
  const bool ngr = p.ctl->ngram[rd.slot] > 0;   // k_ngram_ban may have written -inf into the row: its maxima are rebuilt here
  if (!r.on && !con && !bia && !ngr) return;   // neither penalised, constrained, biased nor n-gram banned: the lm_head's maxima stand
  const int lane = threadIdx.x & 63, set = blockIdx.x * kPenWaves + (threadIdx.x >> 6);
  if (set >= p.nblk) return;
  int nbl = 0;   // stage 0b: ids of this wave's set whose logit takes a bias total at this step
  if (bia) {
    bool any;
    nbl = seq_bias_list(sq, rd, p.ghist, p.max_steps, lane, set * p.per, min(set * p.per + p.per, p.V), s_bid[threadIdx.x >> 6],
                        s_btot[threadIdx.x >> 6], &any);
    if (!any && !r.on && !con && !ngr) return;   // no entry applies at this step: the row is the lm_head's, its maxima stand
  }
  const int* l_id = s_bid[threadIdx.x >> 6];
  const float* l_tot = s_btot[threadIdx.x >> 6];
  // the sampler and k_logprob read the logits; k_finalize of a row that does neither only the maxima
  const bool wb = rec_samples(p.ctl->samp[rd.slot], p.hs) || p.ctl->lp[rd.slot];
  const bool mask = rd.flags < r.min_new;
  int eos[SMI_MAX_EOS];
#pragma unroll
  for (int e = 0; e < SMI_MAX_EOS; ++e) eos[e] = e < p.ctl->n_eos ? (int)p.ctl->eos[e] : -1;
  float* lg = p.logits + (size_t)m * p.V;
  const uint16_t* hs = p.hist + (size_t)rd.slot * p.V;
  const int i0 = set * p.per, i1 = min(i0 + p.per, p.V);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if ((p.V & 3) == 0) {   // i1 - i0 is a multiple of 4: every float4 / uint2 lies inside the set and is aligned
    for (int i = i0 + 4 * lane; i < i1; i += 256) {
      float4 x = *(const float4*)(lg + i);
      if (con) {
        if (!allow_has(al, i)) x.x = -INFINITY;
        if (!allow_has(al, i + 1)) x.y = -INFINITY;
        if (!allow_has(al, i + 2)) x.z = -INFINITY;
        if (!allow_has(al, i + 3)) x.w = -INFINITY;
      }
      for (int e = 0; e < nbl; ++e) {   // x + total: one fp32 add (an id outside the allowed set stays -inf)
        const int d = l_id[e] - i;
        const float t = l_tot[e];
        if (d == 0) x.x += t;
        if (d == 1) x.y += t;
        if (d == 2) x.z += t;
        if (d == 3) x.w += t;
      }
      if (r.on) {
        const uint2 hh = *(const uint2*)(hs + i);
        x.x = pen_logit(x.x, hh.x & 0xffffu, r, mask, i, eos);
        x.y = pen_logit(x.y, hh.x >> 16, r, mask, i + 1, eos);
        x.z = pen_logit(x.z, hh.y & 0xffffu, r, mask, i + 2, eos);
        x.w = pen_logit(x.w, hh.y >> 16, r, mask, i + 3, eos);
      }
      if (wb) *(float4*)(lg + i) = x;
      pen_best(x.x, i, bv, bi); pen_best(x.y, i + 1, bv, bi); pen_best(x.z, i + 2, bv, bi); pen_best(x.w, i + 3, bv, bi);
    }
  } else {
    for (int i = i0 + lane; i < i1; i += 64) {
      float x = lg[i];
      if (con && !allow_has(al, i)) x = -INFINITY;
      for (int e = 0; e < nbl; ++e)
        if (l_id[e] == i) x += l_tot[e];
      if (r.on) x = pen_logit(x, hs[i], r, mask, i, eos);
      if (wb) lg[i] = x;
      pen_best(x, i, bv, bi);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pen_best(__shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64), bv, bi);
  if (lane == 0) {
    p.pval[(size_t)m * p.nblk + set] = bv;   // an empty set (per * nblk > V): (-inf, no id), below every real entry
    p.pidx[(size_t)m * p.nblk + set] = bi;
  }
}

// ------------------------------------------------------------------------------------------
// no_repeat_ngram_size (smi_llm_admit_ngram; include/sparkmi.h states the semantics).  The context of the sequence in a slot is
// its prompt ids (the slot's row of the context store, written at admission) followed by the ids it has generated (the slot's
// column of the token history, which k_finalize writes); n and the prompt length are in Ctl.  k_ngram_ban runs after the
// lm_head and before k_penalize: grid (1, M) x 256, a row with n = 0 leaves at once.  A flagged row copies its context into
// LDS (or reads it in place when it does not fit), lane t takes the start positions t, t + 256, ...: where the n - 1 ids from
// there equal the context's last n - 1 ids, the id that followed gets -inf in the row's logits.  Plain stores: duplicates
// write the same value.  The stage only ever writes -inf, so the stages of k_penalize, which map -inf to -inf, give the same
// row whether they ran before or after it; k_penalize treats the row as active and rebuilds its maxima.
// ------------------------------------------------------------------------------------------
struct NgramP {
  float* logits;          // [M][V]
  const Ctl* ctl;         // per-slot n and prompt length
  const RowDesc* rows;
  const int32_t* pctx;    // [max_slots][max_pos] prompt ids per slot
  const int64_t* ghist;   // [max_steps][kMaxRows] generated tokens per slot
  int V, max_pos, max_steps;
  int lds_ids;            // ids the dynamic LDS holds beside the tail (0: the context is read in place)
};

__global__ __launch_bounds__(256) void k_ngram_ban(NgramP p) {
  extern __shared__ int32_t s_ng[];   // [SMI_MAX_NGRAM] tail, then [lds_ids] context
  const int m = blockIdx.y, tid = threadIdx.x;
  const RowDesc rd = p.rows[m];
  const int n = p.ctl->ngram[rd.slot];
  if (n <= 0 || n > SMI_MAX_NGRAM) return;
  const int plen = min(p.ctl->ngplen[rd.slot], p.max_pos), gen = min(rd.flags, p.max_steps);
  const int L = plen + gen;
  if (L + 1 < n) return;
  const int32_t* pc = p.pctx + (size_t)rd.slot * p.max_pos;
  const int64_t* gh = p.ghist + rd.slot;
  auto ctx_global = [&](int i) { return i < plen ? pc[i] : (int32_t)gh[(size_t)(i - plen) * kMaxRows]; };
  int32_t* s_tail = s_ng;
  int32_t* s_ctx = s_ng + SMI_MAX_NGRAM;
  const bool in_lds = L <= p.lds_ids;
  if (tid < n - 1) s_tail[tid] = ctx_global(L - n + 1 + tid);
  if (in_lds)
    for (int i = tid; i < L; i += 256) s_ctx[i] = ctx_global(i);
  __syncthreads();
  float* lg = p.logits + (size_t)m * p.V;
  for (int i = tid; i <= L - n; i += 256) {   // i + n - 1 <= L - 1: every read lies inside the context
    bool eq = true;
    if (in_lds) { for (int k = 0; k < n - 1 && eq; ++k) eq = s_ctx[i + k] == s_tail[k]; }
    else { for (int k = 0; k < n - 1 && eq; ++k) eq = ctx_global(i + k) == s_tail[k]; }
    if (eq) {
      const int id = in_lds ? s_ctx[i + n - 1] : ctx_global(i + n - 1);
      if ((unsigned)id < (unsigned)p.V) lg[id] = -INFINITY;
    }
  }
}

// admission of penalised prompts: idx[i] = slot * V + id for every prompt token of a record that penalises its prompt
__global__ __launch_bounds__(256) void k_pen_prompt(uint16_t* hist, const int32_t* idx, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[idx[i]] = 0x8000;   // (plain stores: duplicate ids write the same value; the row was zeroed before)
}

// ------------------------------------------------------------------------------------------
// Per-token log-probabilities (smi_llm_admit_logprobs; include/sparkmi.h states the semantics).  k_logprob runs after
// k_penalize and the sampler, before k_finalize, on the logits rows the lm_head wrote (a penalised flagged row's are the
// processed ones: k_penalize writes them back for flagged rows too).  Grid (kLpBlocks, M) x 256: block b of row m sums
// exp((x - max) * 1/T) over its fixed slice of the row and leaves one partial; k_finalize adds the kLpBlocks partials in block
// order and writes lp = (x[tok] - max) * 1/T - log(sum) beside the token.  max is the row maximum, taken from the nblk (value,
// id) maxima the lm_head (or k_penalize) left: exact, whatever partition produced them.  Fixed slices and a fixed reduction
// order (shuffles, then the waves in order; no atomics): a row's value depends on its own logits alone, not on the row count
// or its neighbours.  Unflagged rows leave at once.
// ------------------------------------------------------------------------------------------
constexpr int kLpBlocks = 64;   // blocks (partials) per row

struct LpP {
  const float* logits;    // [M][V]
  const Ctl* ctl;         // per-slot flags and sampling records
  const RowDesc* rows;
  const float* pval;      // [M][nblk] row maxima by sets
  int nblk, V, per;       // per: ids per block, a multiple of 4 (per * kLpBlocks >= V)
  float inv_temp;         // the handle's 1/T (inheriting rows of a sampling handle)
  int hs;                 // the handle samples
  float* part;            // [kMaxRows][kLpBlocks] partial sums
  float2* rowc;           // [kMaxRows] (max, 1/T) of each flagged row (block 0 writes it)
};

// 1/T of row m exactly as k_sample scales it (row_sel): its record's, the handle's for an inheriting row of a sampling
// handle; 1 for a row that does not sample
__device__ __forceinline__ float lp_inv_temp(const SampRec& r, int hs, float handle_inv_temp) {
  if (!rec_samples(r, hs)) return 1.f;
  return r.mode == SMI_SAMPLING_SAMPLE ? r.inv_temp : handle_inv_temp;
}

__global__ __launch_bounds__(256) void k_logprob(LpP p) {
  __shared__ float s_red[4];
  const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RowDesc rd = p.rows[m];
  if (!p.ctl->lp[rd.slot]) return;   // not flagged
  const float it = lp_inv_temp(p.ctl->samp[rd.slot], p.hs, p.inv_temp);
  float mx = -INFINITY;
  for (int j = tid; j < p.nblk; j += 256) mx = fmaxf(mx, p.pval[(size_t)m * p.nblk + j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();   // (s_red is reused below)
  const float* lg = p.logits + (size_t)m * p.V;
  const int i0 = (int)blockIdx.x * p.per, i1 = min(i0 + p.per, p.V);
  float s = 0.f;
  if ((p.V & 3) == 0) {   // i0 and i1 are multiples of 4: every float4 lies inside the slice and is aligned
    for (int i = i0 + 4 * tid; i < i1; i += 1024) {
      const float4 x = *(const float4*)(lg + i);
      s += (expf((x.x - mx) * it) + expf((x.y - mx) * it)) + (expf((x.z - mx) * it) + expf((x.w - mx) * it));
    }
  } else {
    for (int i = i0 + tid; i < i1; i += 256) s += expf((lg[i] - mx) * it);
  }
  s = smi_wave_sum(s);
  if (lane == 0) s_red[wave] = s;
  __syncthreads();
  if (tid == 0) {
    p.part[(size_t)m * kLpBlocks + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    if (blockIdx.x == 0) p.rowc[m] = make_float2(mx, it);
  }
}

struct FinP {
  const int* tok;       // non-null: tokens already chosen by k_sample for the rows that sample (rec_samples)
  int hs;               // the handle samples
  uint16_t* phist;      // non-null (some row is penalised): penalised rows count their token in their slot's history row
  float* lp;            // non-null (some row is flagged): [max_steps][kMaxRows] log-probabilities beside hist
  const float* lp_part; // [kMaxRows][kLpBlocks] k_logprob's partial sums
  const float2* lp_rowc;// [kMaxRows] (max, 1/T)
  const float* logits;  // [M][V]
  const float* pval;
  const int* pidx;
  int nblk, M, KT, V;
  RowDesc* rows;
  int64_t* hist;      // [max_steps][kMaxRows]
  int32_t* count;     // [kMaxRows] tokens counted per sequence
  int32_t* finished;  // [kMaxRows]
  int32_t* step;      // [1]
  const Ctl* ctl;     // eos ids
  const uint16_t* Wlm;
  float* h;
  int max_steps;
  const float* gamma0;   // first layer's input norm weight
  unsigned char* xs;     // first layer's operand
  float* sspart; int npart;
  int exact;             // exact-weights arena: Wlm is fp32 [vocab][K]
  const SeqRec* seq;     // non-null (some live row has a stop sequence): per-slot stop sequences
};

// The sequence in slot sl has just emitted `tok` as its token number `step` (0-based): some stop sequence of its record equals
// the last ids it has generated, and it has emitted at least min_new tokens (smi_llm_admit_biased).  The earlier tokens come
// from the slot's history, which earlier launches wrote.
__device__ __forceinline__ bool seq_stop(const SeqRec& q, const int64_t* hist, int sl, int step, int tok, int min_new, int max_steps) {
  bool stop = false;
  if (step + 1 < min_new) return false;
  for (int s = 0; s < q.n_stop; ++s) {
    const int L = q.slen[s];
    if (step + 1 < L || step >= max_steps) continue;
    bool eq = q.sids[s][L - 1] == tok;
    for (int k = 1; k < L && eq; ++k) eq = hist[(size_t)(step - k) * kMaxRows + sl] == (int64_t)q.sids[s][L - 1 - k];
    stop |= eq;
  }
  return stop;
}

// One block per row: arg-max over the lm_head blocks' partials (or the sampled token), per-row
// bookkeeping, and the next step's residual row / first-norm operand.  The per-row step index lives
// in the row descriptor (flags), so blocks never race on a shared counter; block 0 publishes it.
__global__ __launch_bounds__(256) void k_finalize(FinP p) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int tok_s;
  __shared__ float lp_sum;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  const bool sampled = p.tok && rec_samples(p.ctl->samp[p.rows[m].slot], p.hs);
  const bool want_lp = p.lp && p.ctl->lp[p.rows[m].slot];
  if (want_lp && tid == 64) {   // wave 1 adds k_logprob's partials in block order while wave 0 reduces the maxima
    float part[kLpBlocks];
#pragma unroll
    for (int b = 0; b < kLpBlocks; ++b) part[b] = p.lp_part[(size_t)m * kLpBlocks + b];
    float s = 0.f;
#pragma unroll
    for (int b = 0; b < kLpBlocks; ++b) s += part[b];
    lp_sum = s;
  }
  if (!sampled) {   // greedy: the arg-max of the lm_head blocks' maxima, the same bits with or without the sampler in the step
    constexpr int NP = 16;   // all partial loads in flight together (one memory round trip)
    float pv[NP];
    int pi[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = tid + 256 * j;
      const bool in = i < p.nblk;
      pv[j] = in ? p.pval[(size_t)m * p.nblk + i] : -INFINITY;
      pi[j] = in ? p.pidx[(size_t)m * p.nblk + i] : 0x7fffffff;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (pv[j] > bv || (pv[j] == bv && pi[j] < bi)) { bv = pv[j]; bi = pi[j]; }
    for (int i = tid + 256 * NP; i < p.nblk; i += 256) {
      const float v = p.pval[(size_t)m * p.nblk + i];
      const int ix = p.pidx[(size_t)m * p.nblk + i];
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    if (sampled) bi = p.tok[m];
    if ((unsigned)bi >= (unsigned)p.V) bi = 0;   // no finite logit (NaN weights / inputs): a defined token instead of an out-of-range embedding row
    tok_s = bi;
    RowDesc rd = p.rows[m];
    const int step = rd.flags;                 // tokens this row has emitted so far
    const int sl = rd.slot;                    // history / counters live per KV slot (== m outside sessions)
    if (step < p.max_steps) p.hist[(size_t)step * kMaxRows + sl] = bi;
    if (want_lp && step < p.max_steps) {
      const float2 rc = p.lp_rowc[m];
      p.lp[(size_t)step * kMaxRows + sl] = (p.logits[(size_t)m * p.V + bi] - rc.x) * rc.y - logf(lp_sum);
    }
    if (p.phist && p.ctl->pen[sl].on) {   // one writer per slot: no atomics
      uint16_t& e = p.phist[(size_t)sl * p.V + bi];
      if ((e & 0x7fffu) != 0x7fffu) e = (uint16_t)(e + 1);
    }
    if (!p.finished[sl]) {
      p.count[sl] = step + 1;
      bool stop = false;   // HF generate(): any id of generation_config.eos_token_id ends the sequence
#pragma unroll
      for (int e = 0; e < SMI_MAX_EOS; ++e) stop |= e < p.ctl->n_eos && (long long)bi == p.ctl->eos[e];
      if (p.seq && p.seq[sl].n_stop > 0) stop |= seq_stop(p.seq[sl], p.hist, sl, step, bi, p.ctl->pen[sl].min_new, p.max_steps);
      if (stop) p.finished[sl] = 1;
    }
    rd.token = bi;
    rd.pos += 1;
    rd.flags = step + 1;
    p.rows[m] = rd;
    if (m == 0) *p.step = step + 1;
  }
  __syncthreads();
  if (wave == 0) {
    if (p.exact) embed_row_x((const float*)p.Wlm, p.KT, tok_s, m, p.M, p.gamma0, p.h, p.xs, p.sspart, p.npart, lane);
    else embed_row(p.Wlm, p.KT, tok_s, m, p.M, p.gamma0, p.h, p.xs, p.sspart, p.npart, lane);
  }
}

}  // namespace
#ifdef SMI_DIAG   // the one-row decode engine (built, bit-exact, slower than the launch path: DESIGN 3.7) lives in the diagnostics build only
#include "smi_eng.h"        // all layers of a step in one persistent launch
#include "smi_eng_host.h"
#endif
namespace {

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Layout {
  size_t off[SMI_LLM_NUM_SECTIONS];   // per-layer sections: offset inside a layer block
  size_t bytes[SMI_LLM_NUM_SECTIONS];
  size_t layer_stride, layers_base, total;
  int vpad;
};

bool cfg_ok(const smi_llm_cfg* c) {
  if (!c) return false;
  if (c->head_dim != kHeadDim || c->hidden_size <= 0 || c->hidden_size % 32) return false;
  if (c->intermediate_size <= 0 || c->intermediate_size % 32) return false;
  if (c->num_heads <= 0 || c->num_kv_heads <= 0 || c->num_heads % c->num_kv_heads) return false;
  if (c->num_layers <= 0 || c->vocab_size <= 0) return false;
  if (c->max_slots < 1 || c->max_slots > kMaxRows || c->max_positions < 2) return false;
  if ((c->num_heads * c->head_dim) % 32) return false;
  if (c->kv_dtype != 0 && c->kv_dtype != 1) return false;
  if (c->wd_plain != 0 && c->wd_plain != 1) return false;
  if (c->weights_exact != 0 && c->weights_exact != 1) return false;
  if (c->kv_page_tokens != 0) {   // paged KV: a power of two in 16..1024 that divides max_positions, and a pool of at least one page
    const int t = c->kv_page_tokens;
    if (t < 16 || t > 1024 || (t & (t - 1)) || c->max_positions % t || c->kv_pages < 1) return false;
  }
  return true;
}

Layout make_layout(const smi_llm_cfg* c) {
  Layout L;
  memset(&L, 0, sizeof(L));
  const size_t H = c->hidden_size, Q = (size_t)c->num_heads * c->head_dim, KV = (size_t)c->num_kv_heads * c->head_dim;
  const size_t I = c->intermediate_size;
  L.vpad = (c->vocab_size + 15) / 16 * 16;
  L.bytes[SMI_LLM_LN1] = H * 4;
  const size_t wb = c->weights_exact ? 4 : 2;   // exact-weights mode: fp32 [N][K] row-major instead of bf16 tiles
  L.bytes[SMI_LLM_WQKV] = (Q + 2 * KV) * H * wb;
  L.bytes[SMI_LLM_BQKV] = (Q + 2 * KV) * 4;
  L.bytes[SMI_LLM_WO] = H * Q * wb;
  L.bytes[SMI_LLM_LN2] = H * 4;
  L.bytes[SMI_LLM_WGU] = 2 * I * H * wb;
  L.bytes[SMI_LLM_WD] = H * I * wb;
  L.bytes[SMI_LLM_FINAL_NORM] = H * 4;
  L.bytes[SMI_LLM_LM_HEAD] = (size_t)L.vpad * H * wb;
  L.bytes[SMI_LLM_ROPE] = (size_t)c->max_positions * (kHeadDim / 2) * 8;
  L.bytes[SMI_LLM_TAG] = sizeof(smi_llm_arena_tag);
  size_t o = 0;
  for (int s = SMI_LLM_LN1; s <= SMI_LLM_WD; ++s) { L.off[s] = o; o += smi_align_up(L.bytes[s], 256); }
  L.layer_stride = o;
  size_t g = 0;
  for (int s = SMI_LLM_FINAL_NORM; s <= SMI_LLM_TAG; ++s) { L.off[s] = g; g += smi_align_up(L.bytes[s], 256); }
  L.layers_base = g;
  L.total = g + L.layer_stride * c->num_layers;
  return L;
}

// The activation buffers of one pass over the layers, for some number of rows (gemm_operands / attn_operands name them to the
// kernels).
struct Work {
  DevBuf<float> h, q;                             // residual rows [rows][H]; QKV's query output [rows][Q]
  DevBuf<unsigned char> xs_h, xs_attn, xs_act;    // GEMM operands as exact bf16 triples ([K/32][3][4][M][16 B])
  DevBuf<float> ss;                               // [rows][NTh * 4] partial sums of squares of h (RMSNorm), one per 4 columns
};

// The diagnostics switches of the launch path, read once per handle by read_switches; the product build reads no
// environment and gets the defaults.
struct Switches {
  int prefetch_mask, prefetch_rows;   // same-XCD L2 prefetch by helper blocks: one bit per producer kernel, up to this many live rows
  int pf_qkv_eighths;   // how much of gate_up QKV's helpers prefetch, in eighths
  int pf_inline;        // gate_up's work blocks touch the next layer's QKV weights
  int tune2;            // bit mask (the kTune2* bits)
  int fuse2_rows;       // rows up to which 2+ live rows take the fused attention + o_proj with the last-arriver head sum
  int pg_split_rows;    // passes of up to this many rows take the few-row prefill GEMM shapes / split-K
  int pg_min[4];        // prompt rows from which the prefill GEMM replaces the row-grouped decode GEMM, per kernel (QKV, o_proj, gate_up, down)
  int pg_forced;        // a SPARKMI_PGEMM_MIN_* is set: kernels picked per launch by the pass's row count, as in round 3
  int attn_pf2;         // bf16 KV: prefill attention on the matrix pipes
  int no_fuse_o;        // one-row decode with the separate o_proj kernel
  int lm_screen;        // the one-row greedy lm_head's int8 screen: -1 by the size of the lm_head section, 0 / 1 forced (SPARKMI_LM_SCREEN)
};

}  // namespace

struct smi_llm {
  smi_llm_cfg cfg;
  Layout lay;
  const unsigned char* arena;
  int H, Q, KV, I, KTh, KTq, KTi, NTqkv, NTh, NTgu, NTlm;
  // device scratch
  Work dec;            // the decode rows' workspace (kMaxRows rows)
  Work big; int big_rows;   // prefill workspace for up to big_rows rows at once (allocated at the first multi-chunk prefill)
  DevBuf<float4> pslab;     // k_pgemm split-K partial sums (prompt rows passes of up to kPgSplitRows rows)
  Switches sw;          // the diagnostics switches (read_switches)
  DevBuf<float> part_o, h2;   // fused o_proj (one row): per-head partials [heads][H]; h + o_proj [H]
  DevBuf<float4> dpart;       // chain-split down_proj (k_downC): [16 chains][NTh][4 m-tiles][64] chain sums
  int fuse_o;          // config allows the fused o_proj (and Switches::no_fuse_o is clear)
  DevBuf<unsigned int> fuse_cnt;   // [kFuse2Max][kFuseQB] arrival counters of that kernel (zero between launches)
  DevBuf<RowDesc> rows;       // live decode rows [kMaxRows]
  DevBuf<RowDesc> plan;       // prefill plan (grows on demand: ensure_plan)
  DevBuf<PfTile> pf_tiles;    // prefill attention tiles of the row group in flight (k_attn_pf2; grows on demand)
  int pf_ntiles;
  std::vector<PfTile> host_tiles;
  int dbg_pf_rows;      // diagnostics: rows the last smi_llm_debug_prefill_layer left in the big workspace (smi_llm_debug_read 16 .. 20)
  DevBuf<float> pval; DevBuf<int> pidx; int lm_blocks, lm_cap;
  DevBuf<int64_t> hist; DevBuf<int32_t> count, finished, step;
  DevBuf<void> kcache, vcache; size_t kv_layer_elems;
  int B; int started;
  // paged KV cache (cfg.kv_page_tokens > 0): page table [max_slots][ppslot] on the device, mirrored on the host
  int paged, pshift, ppslot;
  DevBuf<int32_t> ptab;
  std::vector<int32_t> hptab;
  std::vector<int32_t> free_pages;
  std::vector<int32_t> page_ref;   // [kv_pages] slots whose table rows hold the page (> 1: shared by forked takes)
  int slot_pages[kMaxRows];     // pages a slot holds
  Ctl hctl; DevBuf<Ctl> ctl;   // host copy / device block of the generation controls
  int admit_seq;        // sequences admitted so far in this generation / session (sampler stream ids)
  // One bookkeeping for plain generation and sessions: a sequence sits in a KV slot (slot_busy / slot_len) and the live rows map
  // to slots through live_order.  smi_llm_prefill is slots 0 .. B-1 in order; in a session (continuous batching) admissions and
  // retirements change the set, so rows map to arbitrary slots.  `session` only gates admit / retire.
  int session, identity_slots = 1;
  std::vector<int> live_order;   // the KV slot of every live row, in row order (what the device row list holds)
  int attn_seg = 1;                    // context segments per (head, row) of the attention launches being issued (1 = unsplit)
  DevBuf<float> apart;                 // segment partials [rows][heads][attn_seg][66] (grows on demand: ensure_apart)
  int slot_busy[kMaxRows], slot_len[kMaxRows];      // host: slot in use; prompt length + tokens emitted (cache positions used)
  int slot_plen[kMaxRows];      // host: the prompt length of the sequence in the slot (slot_len - slot_plen = its token index)
  uint64_t handle_id, session_gen;   // blob stamps: this handle among the process's, and its generations / sessions so far (gen_reset)
  std::vector<unsigned char> host_blob;   // host staging of the blob headers a save uploads
  // sampling state (smi_llm_set_sampling)
  int do_sample, top_k = 50; float temperature = 0.8f, top_p = 0.95f; unsigned long long seed;
  // host: what the record set of the sequence in each slot (live or being admitted) asks of a step, F_* bits: its sampling record
  // is SMI_SAMPLING_SAMPLE, it has a penalty record (PenRec::on), returns log-probabilities (Ctl::lp), is constrained
  // (Ctl::allow, n > 0), has bias entries (SeqRec::n_bias > 0), has stop sequences (SeqRec::n_stop > 0), bans repeated
  // n-grams (Ctl::ngram > 0)
  uint8_t slot_feat[kMaxRows];
  int lm_restrict;              // host: every row of the steps being issued is constrained (the restricted lm_head may run)
  int seq_dirty[kMaxRows];      // host: the slot's device record is not all zero (an admission without a record clears it)
  DevBuf<SeqRec> seq;           // device: per-slot bias / stop records [kMaxRows] (smi_llm_admit_biased)
  std::vector<SeqRec> hseq;     // host: what the device records hold
  DevBuf<int32_t> pctx;         // device: prompt ids [max_slots][max_positions], the n-gram ban's context store (smi_llm_admit_ngram)
  std::vector<int32_t> host_pctx;   // host staging of the rows an admission writes
  DevBuf<int> tlist;            // device: {count, vocabulary tiles ascending} -- the union of the constrained slots' tiles
  std::vector<int32_t> host_tlist;
  // The one-row greedy lm_head's int8 screen: the copy of the lm_head section (tiles, s_v, s_v Q_v; built once by
  // lm_screen_build), the per-tile upper / per-block lower bounds of a step, the candidate list {count, tiles} and, diagnostics,
  // the counts of the last selections.  scr_on: steps that qualify take it (lm_screened); scr_force: smi_llm_debug_head asked.
  DevBuf<unsigned char> scr_q8; DevBuf<float> scr_s8, scr_sq8, scr_ub, scr_lb; DevBuf<int> scr_list, scr_log;
  int scr_ready, scr_on, scr_force, scr_blocks;
  DevBuf<float> lp;             // log-probabilities [max_steps][kMaxRows], beside hist (k_finalize)
  DevBuf<float> lp_part; DevBuf<float2> lp_rowc;   // k_logprob -> k_finalize: [kMaxRows][kLpBlocks] partial sums, [kMaxRows] (max, 1/T)
  DevBuf<uint16_t> phist;       // penalty histories [max_slots][vocab] (k_penalize, k_finalize)
  DevBuf<int64_t> poll_dev; DevBuf<int64_t, true> poll_host;   // smi_llm_poll: device staging / pinned host copy, [kMaxRows][1 + max_steps] words
  DevBuf<int32_t> pen_idx;      // admission: slot * vocab + id of the prompt tokens whose bit k_pen_prompt sets (grows on demand)
  std::vector<int32_t> host_pen_idx;
  DevBuf<float> logits; DevBuf<int> tok;
  DevBuf<float> cand_v; DevBuf<int> cand_i; DevBuf<unsigned int> cand_n;   // sampler candidate lists
  DevBuf<unsigned long long> stamps; int stamps_on;
  int max_steps;
  int wd_parts;         // W_down tiles are stored row-part-major (smi_llm_cfg.wd_plain == 0; include/sparkmi.h)
  int exact;            // smi_llm_cfg.weights_exact: fp32 matrices, every GEMM on k_gemm_x (verification mode)
  hipGraphExec_t graph; uint64_t graph_id;   // the one-step graph in use (owned by graph_cache) and its graph_key
  // every exec remembers the stream it last ran on: a caller may alternate streams, and an exec is destroyed only after THAT
  // stream has drained (graphs_flush)
  std::map<hipGraphExec_t, hipStream_t> graph_last;
  // One captured decode step per graph_key (row count, context segments, slots-are-rows, the step's feature mask, restricted
  // lm_head, steps per replay): in-flight batching changes the row count at every admission / retirement, and re-capturing the
  // ~100-node step each time cost more than the steps saved.
  // Everything else a step reads is device data (row descriptors, stop ids, seed, the per-slot sampling records) or fixed at
  // create; the handle's sampler settings and the attention-partials buffer are kernel arguments, so a change of either empties
  // the cache (graphs_flush).  The sample bit decides only whether lm_head writes the logits rows and the sampler kernels run:
  // a step in which no row samples is the greedy step exactly.  Likewise the penalty bit only adds the logits rows and
  // k_penalize: a step in which no row is penalised is the step without penalties exactly; and the log-probability bit only
  // adds the logits rows and k_logprob.  The constraint bits: some row constrained (the full lm_head writes the logits rows and
  // k_penalize applies stage 0), and every row constrained (the restricted lm_head, whose tile list is device data).  The
  // sequence bits: some row has a bias entry (the logits rows, and k_penalize gets the records: stage 0b), some row has a stop
  // sequence (k_finalize gets the records); with both clear neither kernel is handed the record array.  The n-gram bit: some
  // row has no_repeat_ngram_size > 0 (the logits rows, k_ngram_ban before k_penalize); with it clear the step is the step without.
  std::map<uint64_t, hipGraphExec_t> graph_cache;
  hipEvent_t ev0, ev1;
  // host staging
  std::vector<RowDesc> host_rows;
#ifdef SMI_DIAG
  EngState eng;         // one-row decode engine (smi_eng.h); eng.enabled = 0: the launch path everywhere
  int eng_on;           // runtime switch (smi_llm_set_engine; SPARKMI_ENGINE=0 at create)
  // the lm_head launches since smi_llm_debug_head last cleared the note: the form's name, its grid and block, the launches
  mutable char lm_note_form[32]; mutable int lm_note_grid[2], lm_note_block, lm_note_n;
#endif
};
#ifdef SMI_DIAG   // (diagnostics) every lm_head launch site names the kernel form it starts: smi_llm_debug_head reports it
#define SMI_LM_NOTE(L_, form_, gx_, gy_, blk_) do { const smi_llm* ln_ = (L_); \
    snprintf(ln_->lm_note_form, sizeof(ln_->lm_note_form), "%s", form_); ln_->lm_note_grid[0] = (int)(gx_); ln_->lm_note_grid[1] = (int)(gy_); \
    ln_->lm_note_block = (int)(blk_); ++ln_->lm_note_n; } while (0)
#else
#define SMI_LM_NOTE(L_, form_, gx_, gy_, blk_) do { } while (0)
#endif

namespace {

// Kernels a launch site may start with more dynamic LDS than the default 64 KiB window.  Such a site names its kernel in
// LdsBig<kernel>::reg; the initialiser of that static member runs when the library is loaded and enters the kernel here, and
// smi_llm_create opts every entry in to the large window on its device.  So the opt-in never happens inside a stream capture
// (a step's first launch of k_downC<10, 4> -- 33+ rows -- may be the one in the captured decode step), and a launch does not
// depend on what ran before it in the process.
std::vector<const void*>& lds_big_kernels() {
  static std::vector<const void*> v;
  return v;
}
bool lds_big_register(const void* f) {
  lds_big_kernels().push_back(f);
  return true;
}
template <auto F>
struct LdsBig {
  static inline const bool reg = lds_big_register((const void*)F);
};
constexpr int kLdsBigBytes = 160 * 1024;   // the window every LdsBig kernel is opted in to
int lds_big_opt_in() {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    smi_set_error("smi_llm_create: no current device");
    return SMI_EHIP;
  }
  for (size_t i = 0; i < lds_big_kernels().size() && !done[dev]; ++i)
    if (hipFuncSetAttribute(lds_big_kernels()[i], hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBigBytes) != hipSuccess) {
      smi_set_error("smi_llm_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(hipGetLastError()));
      return SMI_EHIP;
    }
  done[dev] = true;
  return SMI_OK;
}

// The KV cache's element type as a template argument of a GEMM launch: f(kv) with kv() = 1 for an f32 cache where the epilogue
// appends to the cache (EPI_QKV), and the constant 0 for every other epilogue -- those kernels never read it, so they exist once.
template <int EPI, class F>
auto with_kvf32(const smi_llm* L, F&& f) {
  if constexpr (EPI == EPI_QKV)
    if (L->cfg.kv_dtype) return f(std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 0>{});
}

// ---- paged KV cache: host-side page allocator.  A slot's row of the table lists the pages of its positions in order.  A page
// may sit in several rows (the leading pages of a forked admission's takes, pages_share); page_ref counts them, and a page goes
// back to the pool when its last holder lets go of it.
void pages_release(smi_llm* L, int slot) {
  for (int i = 0; i < L->slot_pages[slot]; ++i) {
    const int32_t pg = L->hptab[(size_t)slot * L->ppslot + i];
    if (--L->page_ref[pg] == 0) L->free_pages.push_back(pg);
  }
  L->slot_pages[slot] = 0;
}
// The empty slot `dst` takes the first `n` pages of slot `src` as its own first n pages, shared (read-only by contract: they
// hold positions no later step writes).  Host table only; the next pages_ensure uploads it.
void pages_share(smi_llm* L, int src, int dst, int n) {
  for (int i = 0; i < n; ++i) {
    const int32_t pg = L->hptab[(size_t)src * L->ppslot + i];
    L->hptab[(size_t)dst * L->ppslot + i] = pg;
    ++L->page_ref[pg];
  }
  L->slot_pages[dst] = n;
}
// Makes every listed slot hold pages for `tokens[i]` positions; all or nothing (SMI_ENOMEM when the pool is short).
int pages_ensure(smi_llm* L, const int* slots, const int* tokens, int n, hipStream_t st) {
  if (!L->paged) return SMI_OK;
  int extra = 0;
  for (int i = 0; i < n; ++i) {
    const int need = (tokens[i] + (1 << L->pshift) - 1) >> L->pshift;
    if (need > L->ppslot) { smi_set_error("KV pages: %d tokens exceed max_positions", tokens[i]); return SMI_EINVAL; }
    extra += need > L->slot_pages[slots[i]] ? need - L->slot_pages[slots[i]] : 0;
  }
  if (extra == 0) return SMI_OK;
  if (extra > (int)L->free_pages.size()) {
    smi_set_error("KV page pool exhausted: %d more pages of %d tokens needed, %zu of %d free (retire a sequence or enlarge kv_pages)",
                  extra, 1 << L->pshift, L->free_pages.size(), L->cfg.kv_pages);
    return SMI_ENOMEM;
  }
  for (int i = 0; i < n; ++i) {
    const int sl = slots[i], need = (tokens[i] + (1 << L->pshift) - 1) >> L->pshift;
    while (L->slot_pages[sl] < need) {
      L->hptab[(size_t)sl * L->ppslot + L->slot_pages[sl]++] = L->free_pages.back();
      L->page_ref[L->free_pages.back()] = 1;
      L->free_pages.pop_back();
    }
  }
  SMI_HIP(hipMemcpyAsync(L->ptab, L->hptab.data(), L->hptab.size() * 4, hipMemcpyHostToDevice, st));
  return SMI_OK;
}
KvMap kv_map(const smi_llm* L) { return KvMap{L->paged ? L->ptab : nullptr, L->pshift, L->ppslot}; }
// What a sequence's record set asks of a step (smi_llm::slot_feat).
enum : uint8_t { F_SAMPLE = 1, F_PEN = 2, F_LP = 4, F_ALLOW = 8, F_BIAS = 16, F_STOP = 32, F_NGRAM = 64 };
constexpr int kFeatBits = 7;   // bits of the feature mask in graph_key
// The features of the steps being issued: the OR over EVERY slot, live or being admitted -- not only the step's rows -- plus
// F_SAMPLE when the handle samples.  An over-estimate is harmless: a row without a feature leaves that feature's kernels at
// once (the sampler kernels, k_penalize, k_logprob) and k_finalize takes its arg-max, so its bits are those of the step without.
// What each bit adds to a step: the comment at smi_llm::graph_cache.
unsigned step_feat(const smi_llm* L) {
  unsigned f = L->do_sample ? F_SAMPLE : 0;
  for (int sl = 0; sl < kMaxRows; ++sl) f |= L->slot_feat[sl];
  return f;
}
// The sequence in `slot` has left (or was not admitted after all): its features no longer count.  Its records stay -- the
// slot's log-probabilities stay readable until it is reused (Ctl::lp), and seq_dirty says what the device record holds.
void slot_clear(smi_llm* L, int slot) { L->slot_feat[slot] = 0; }
// A new generation / session: every sequence inherits the handle's settings, has no penalties, keeps no log-probabilities, is
// not constrained, has no bias entries or stop sequences (seq_dirty stays: the device records are as they were) and bans no
// n-grams.
void slots_clear(smi_llm* L) {
  memset(L->hctl.samp, 0, sizeof(L->hctl.samp));
  memset(L->hctl.pen, 0, sizeof(L->hctl.pen));
  memset(L->hctl.lp, 0, sizeof(L->hctl.lp));
  memset(L->hctl.allow, 0, sizeof(L->hctl.allow));
  memset(L->hctl.ngram, 0, sizeof(L->hctl.ngram));
  memset(L->hctl.ngplen, 0, sizeof(L->hctl.ngplen));
  memset(L->slot_feat, 0, sizeof(L->slot_feat));
  L->lm_restrict = 0;
}
// The step's lm_head reads only the tiles of the union (k_lm / k_lm32 with RT = 1): every row of the step is constrained, and the
// persistent kernels run (K <= 32 tiles, bf16 weights; the generic EPI_LM GEMM and the exact-weights mode take the full path).
bool lm_restricted(const smi_llm* L, unsigned feat) {
  return L->lm_restrict && L->KTh <= 32 && !L->exact && (feat & F_ALLOW);
}
// Some row of the step reads the logits rows: a sampling, penalised, biased, n-gram or log-probability row, or a constrained row whose stage 0
// runs in k_penalize (every constrained row of a full-lm_head step; on the restricted path k_penalize then also runs, so the
// rows it hands on are dense).
bool logits_needed(const smi_llm* L, unsigned feat) {
  return (feat & (F_SAMPLE | F_PEN | F_LP | F_BIAS | F_NGRAM)) || ((feat & F_ALLOW) && !lm_restricted(L, feat));
}
// One live row whose logits no kernel reads (no sampling, penalty, log-probability, constraint, bias or n-gram row anywhere), bf16
// weights, the persistent kernel's K range, and the copy built: the step's lm_head is screen + select + listed tiles.
bool lm_screened(const smi_llm* L, unsigned feat) {
  return (L->scr_on || L->scr_force) && L->scr_ready && L->B == 1 && L->KTh <= 32 && !L->exact &&
         !(feat & (F_SAMPLE | F_PEN | F_LP | F_ALLOW | F_BIAS | F_NGRAM));
}
// the step-graph cache key: rows | segments << 8 | slots-are-rows << 24 | feature mask << 25 (kFeatBits = 7 bits: 25..31) |
// restricted lm_head << 32 | screened lm_head << 33 | steps per replay << 34
uint64_t graph_key(const smi_llm* L, unsigned feat, int K) {
  return (uint64_t)L->B | ((uint64_t)L->attn_seg << 8) | ((uint64_t)(L->identity_slots ? 1 : 0) << 24) | ((uint64_t)feat << 25) |
         ((uint64_t)(lm_restricted(L, feat) ? 1 : 0) << (25 + kFeatBits)) | ((uint64_t)(lm_screened(L, feat) ? 1 : 0) << (26 + kFeatBits)) |
         ((uint64_t)K << (27 + kFeatBits));
}
void graphs_flush(smi_llm* L) {
  // an exec is never destroyed while a launch of it may still be running: the stream each exec last ran on drains first
  // (one synchronise per distinct stream)
  std::vector<hipStream_t> drained;
  for (auto& gl : L->graph_last) {
    bool seen = false;
    for (hipStream_t d : drained) seen |= d == gl.second;
    if (!seen) { (void)hipStreamSynchronize(gl.second); drained.push_back(gl.second); }
  }
  L->graph_last.clear();
  for (auto& kv : L->graph_cache) if (kv.second) (void)hipGraphExecDestroy(kv.second);
  L->graph_cache.clear();
  L->graph = nullptr;
}

// SPARKMI_TUNE2 bits (diagnostics), each the older form of a kernel kept for the parity tests: 8192 k_lm<2> in place of
// k_lm32, 16384 the register-staged k_pgemm in place of the ring forms, 1048576 / 2097152 k_gemm<.., H = 4> in place of k_down1 / k_downS
constexpr int kTune2Lm2 = 8192, kTune2PgemmRegs = 16384, kTune2GemmDown1 = 1048576, kTune2GemmDownS = 2097152;
// Fixed choices of the launch path
// A sequence's prompt rows take the kernel family ITS OWN length selects (never the call's total): up to kMaxRows rows the
// decode kernels in chunks, from kPfLong rows the prefill-GEMM family (k_pgemm + k_attn_pf2), in between (empty: kPfLong =
// kMaxRows + 1) the row-grouped decode GEMMs -- so its K/V rows, and with a bf16 cache its tokens, do not depend on what else is in the call.
constexpr int kPfLong = kMaxRows + 1;    // prompt rows (len - 1) from which a sequence's prompt runs through the prefill-GEMM family
// Decode steps captured per graph replay: a step needs nothing from the host, so K of them are captured back to back into one
// graph.  One replay boundary costs ~5 us that a kernel boundary inside a graph does not: graph step at one row 548.6 -> 544.5 us
// (K = 4 .. 25 alike; profiles/r03_graph_steps.txt).
constexpr int kGraphSteps = 8;
constexpr int kPgSegO = 2, kPgSegD = 8;  // K segments of the prefill o_proj / down_proj sums (fixed: part of the association)
enum { PF_GROUPED = 1, PF_PGEMM = 2 };   // kernel family of a pass over prompt rows (launch_layers_big)

// ------------------------------------------------------------------------------------------
// Kernel forms of the layer GEMMs (QKV, o_proj, gate_up, down_proj) and lm_head.
// A form names ONE launch: one kernel instantiation -- or k_downC / the split-K k_pgemm together with its k_resid_comb.  The
// tables below are the only place a template tuple is written: a row gives the form its id (GF_<id>), its launcher (launch_form)
// and its name (gemm_form_name).  Which form runs is decided once per kernel by a pick (pick_qkv, pick_o, pick_gu, pick_d,
// pick_lm): a host function of plain values -- the operand's shape, the row count and the switches (PickEnv) -- that returns the
// form with its grid, block, dynamic LDS and the fields the kernel splits its work by (GemmPick).  The launch sites (launch_one,
// launch_layer_big) read "operands, pick, launch"; smi_llm_gemm_forms (sparkmi_debug.h) reports the picks without a GPU, and
// DESIGN.md 3.4 has the table kernel x rows -> form.
// ------------------------------------------------------------------------------------------
// k_gemm / k_gemm_hot:  id | MT, NTB, NW, U, WB, PRO, EPI, H, OCC, LEAN, NOH, hot entry.  KVF32 is no column: the cache's type where
// the epilogue appends to the cache (EPI_QKV), else 0.  LEAN 1: the operand staged through wave-private LDS (2 .. 5 rows),
// LEAN 2: that at one row.  NW (the k-tile -> wave map) is fixed per kernel for every row count, so every form of a kernel sums
// in the same order; only the batch depth U shrinks for two m-tiles (register budget).
// o_proj: NW = number of heads, so that wave w sums head w's two (head-interleaved) k tiles -- the per-head partial the fused
// path produces -- and the block's in-order sum over the waves is the fused consumer's in-order sum over the heads; other head
// counts: no fused path (smi_llm_create leaves fuse_o off), eight waves.
#define SMI_O_FORMS(X, NW, U) \
  X(O##NW##_H4_L0, 1, 1, NW, U, 1, PRO_PLAIN, EPI_RESID, 4, 1, 0, kMaxOHeads, 0) \
  X(O##NW##_H4_L1, 1, 1, NW, U, 1, PRO_PLAIN, EPI_RESID, 4, 1, 1, kMaxOHeads, 0) \
  X(O##NW##_H4_L2, 1, 1, NW, U, 1, PRO_PLAIN, EPI_RESID, 4, 1, 2, kMaxOHeads, 0) \
  X(O##NW##_H1, 1, 1, NW, U, 1, PRO_PLAIN, EPI_RESID, 1, 1, 0, kMaxOHeads, 0)
#define SMI_KGEMM_FORMS(X) \
  X(QKV_L0, 1, 1, 16, 2, 1, PRO_NORM, EPI_QKV, 1, 1, 0, kMaxOHeads, 0)   /* measured best (profiles/README.md) */ \
  X(QKV_L1, 1, 1, 16, 2, 1, PRO_NORM, EPI_QKV, 1, 1, 1, kMaxOHeads, 0) \
  X(QKV_HOT, 1, 1, 16, 2, 1, PRO_NORM, EPI_QKV, 1, 1, 2, kMaxOHeads, 1) \
  X(QKV_2M, 2, 1, 16, 2, 1, PRO_NORM, EPI_QKV, 1, 1, 0, kMaxOHeads, 0)   /* a prompt pass's row group above 16 rows */ \
  SMI_O_FORMS(X, 14, 2) SMI_O_FORMS(X, 4, 2) SMI_O_FORMS(X, 8, 4) \
  /* gate_up up to 3 rows: 69 VGPRs (>= 6 waves per SIMD), all 608 blocks resident at once, no second round (step 745 -> 705 us) */ \
  X(GU_L0, 1, 1, 8, 2, 2, PRO_NORM, EPI_SWIGLU, 1, 6, 0, kMaxOHeads, 0) \
  X(GU_L1, 1, 1, 8, 2, 2, PRO_NORM, EPI_SWIGLU, 1, 6, 1, kMaxOHeads, 0) \
  X(GU_L2, 1, 1, 8, 2, 2, PRO_NORM, EPI_SWIGLU, 1, 6, 2, kMaxOHeads, 0) \
  /* one row behind the fused o_proj: the operand is built in the kernel from the per-head partials (14 / 4 heads) */ \
  X(GU_FO14, 1, 1, 8, 2, 2, PRO_FUSEDO, EPI_SWIGLU, 1, 6, 2, 14, 1) \
  X(GU_FO4, 1, 1, 8, 2, 2, PRO_FUSEDO, EPI_SWIGLU, 1, 6, 2, 4, 1) \
  X(GU3_L0, 1, 3, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 0, kMaxOHeads, 0) \
  X(GU3_L1, 1, 3, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 1, kMaxOHeads, 0) \
  X(GU_2M3, 2, 3, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 0, kMaxOHeads, 0) \
  X(GU_2M2, 2, 2, 8, 2, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 0, kMaxOHeads, 0) \
  /* a prompt pass's row group below kGu1Lo rows (the remainder group of a long pass) */ \
  X(GUP_L0, 1, 1, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 0, kMaxOHeads, 0) \
  X(GUP_L1, 1, 1, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 1, kMaxOHeads, 0) \
  X(GUP_L2, 1, 1, 8, 4, 1, PRO_NORM, EPI_SWIGLU, 1, 1, 2, kMaxOHeads, 0) \
  /* down_proj on k_gemm (stamps on, KT > 160, NT % 4 != 0, SPARKMI_TUNE2): H row parts per weight tile */ \
  X(D_H4_L0, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 4, 1, 0, kMaxOHeads, 0) \
  X(D_H4_L1, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 4, 1, 1, kMaxOHeads, 0) \
  X(D_H4_L2, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 4, 1, 2, kMaxOHeads, 0) \
  X(D_H2, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 2, 1, 0, kMaxOHeads, 0) \
  X(D_H1_L0, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 1, 1, 0, kMaxOHeads, 0) \
  X(D_H1_L1, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 1, 1, 1, kMaxOHeads, 0)   /* (L1, L2: a prompt pass's row group of 1 .. 5 rows) */ \
  X(D_H1_L2, 1, 1, 16, 2, 5, PRO_PLAIN, EPI_RESID, 1, 1, 2, kMaxOHeads, 0) \
  X(D_2M, 2, 1, 16, 2, 1, PRO_PLAIN, EPI_RESID, 1, 1, 0, kMaxOHeads, 0)   /* a prompt pass's row group above 16 rows */ \
  X(LM_1M, 1, 4, 4, 2, 1, PRO_NORM, EPI_LM, 1, 1, 0, kMaxOHeads, 0)        /* lm_head with more than 32 k tiles */ \
  X(LM_2M, 2, 4, 4, 2, 1, PRO_NORM, EPI_LM, 1, 1, 0, kMaxOHeads, 0)
// down_proj's own kernels:  id | kernel, TPC (k tiles per chain: KT <= 16 * TPC), MG (k_downS: row groups of four) or MTN (k_downC: m-tiles)
enum { DN_DOWN1 = 1, DN_DOWNS, DN_DOWNC };
#define SMI_DOWN_FORMS_T(X, T) \
  X(D1_##T, DN_DOWN1, T, 0) X(DS_##T##_1, DN_DOWNS, T, 1) X(DS_##T##_2, DN_DOWNS, T, 2) \
  X(DC_##T##_1, DN_DOWNC, T, 1) X(DC_##T##_2, DN_DOWNC, T, 2) X(DC_##T##_4, DN_DOWNC, T, 4)
#define SMI_DOWN_FORMS(X) SMI_DOWN_FORMS_T(X, 2) SMI_DOWN_FORMS_T(X, 6) SMI_DOWN_FORMS_T(X, 10)
// k_pgemm (a prompt pass's row group):  id | PRO, EPI, NTW, WR, RING, XMAP, TWO, MTB.  REGS: the register-staged form
// (SPARKMI_TUNE2 bit kTune2PgemmRegs); FEW: up to pg_split_rows rows, 64-column tiles (more blocks) and a deeper ring -- RES_FEW
// with one block per K segment + the in-order combine (split-K); MANY: beyond.
#define SMI_PGEMM_FORMS(X) \
  X(PG_QKV_REGS, PRO_NORM, EPI_QKV, 2, 1, 0, 0, 0, 8) \
  X(PG_QKV_FEW, PRO_NORM, EPI_QKV, 2, 2, 6, 1, 0, 4) \
  X(PG_QKV_MANY, PRO_NORM, EPI_QKV, 6, 2, 3, 1, 0, 8) \
  X(PG_RES_REGS, PRO_PLAIN, EPI_RESID, 2, 1, 0, 0, 0, 8) \
  X(PG_RES_FEW, PRO_PLAIN, EPI_RESID, 2, 2, 6, 1, 0, 4) \
  X(PG_RES_MANY, PRO_PLAIN, EPI_RESID, 4, 2, 4, 1, 0, 8) \
  X(PG_GU_REGS, PRO_NORM, EPI_SWIGLU, 4, 1, 0, 0, 0, 8) \
  /* 64 KiB ring: two blocks per CU, the 304 blocks of a 127-row prompt in one round (ring of 6: 1.2 rounds, 30 us) */ \
  X(PG_GU_FEW, PRO_NORM, EPI_SWIGLU, 2, 2, 4, 0, 0, 4) \
  X(PG_GU_MANY, PRO_NORM, EPI_SWIGLU, 8, 2, 2, 0, 1, 8)
// the persistent lm_head (KT <= 32):  id | k_lm32?, HV (k_lm) or UW (k_lm32), RT (the restricted form), the name smi_llm_debug_head reports
#define SMI_LM_FORMS(X) \
  X(LM1, 0, 1, 0, "k_lm<1>") X(LM1_RT, 0, 1, 1, "k_lm<1,RT>") X(LM2, 0, 2, 0, "k_lm<2>") X(LM2_RT, 0, 2, 1, "k_lm<2,RT>") \
  X(LM32_7, 1, 7, 0, "k_lm32<7>") X(LM32_7_RT, 1, 7, 1, "k_lm32<7,RT>") X(LM32_8, 1, 8, 0, "k_lm32<8>") X(LM32_8_RT, 1, 8, 1, "k_lm32<8,RT>") \
  /* RT = 2: one greedy row behind the int8 screen -- k_lm_screen, k_lm_select, then k_lm<1, RT, NM> on the screen's list */ \
  X(LM1_SCR, 0, 1, 2, "k_lm_screen+k_lm<1,RT,NM>")
// exact-weights mode (k_gemm_x: fp32 matrices, one exact fp32 FMA chain per output):  id | PRO, EPI
#define SMI_X_FORMS(X) \
  X(X_QKV, PRO_NORM, EPI_QKV) X(X_RESID, PRO_PLAIN, EPI_RESID) X(X_GU, PRO_NORM, EPI_SWIGLU) X(X_LM, PRO_NORM, EPI_LM)

enum GemmForm : int {
  GF_BAD = -1,    // no form for these values: the launch is refused
  GF_NONE = 0,    // nothing to launch (o_proj done by the attention kernel)
#define X(id, ...) GF_##id,
  SMI_KGEMM_FORMS(X) GF_KG_END, SMI_DOWN_FORMS(X) GF_DN_END, SMI_PGEMM_FORMS(X) GF_PG_END, SMI_LM_FORMS(X) GF_LM_END, SMI_X_FORMS(X) GF_X_END
#undef X
};
struct KgShape { int MT, NTB, NW, U, WB, PRO, EPI, H, OCC, LEAN, NOH, hot; };
struct DnShape { int kernel, TPC, N; };
struct PgShape { int PRO, EPI, NTW, WR, RING, XMAP, TWO, MTB; };
struct LmShape { int k32, A, RT; const char* note; };
struct XShape { int PRO, EPI; };
#define X(id, ...) {__VA_ARGS__},
constexpr KgShape kKgShape[] = {SMI_KGEMM_FORMS(X)};
constexpr DnShape kDnShape[] = {SMI_DOWN_FORMS(X)};
constexpr PgShape kPgShape[] = {SMI_PGEMM_FORMS(X)};
constexpr LmShape kLmShape[] = {SMI_LM_FORMS(X)};
constexpr XShape kXShape[] = {SMI_X_FORMS(X)};
#undef X
constexpr const KgShape& kg_shape(int form) { return kKgShape[form - GF_NONE - 1]; }
constexpr const DnShape& dn_shape(int form) { return kDnShape[form - GF_KG_END - 1]; }
constexpr const PgShape& pg_shape(int form) { return kPgShape[form - GF_DN_END - 1]; }
constexpr const LmShape& lm_shape(int form) { return kLmShape[form - GF_PG_END - 1]; }
constexpr const XShape& x_shape(int form) { return kXShape[form - GF_LM_END - 1]; }
// k_pgemm's dynamic LDS: the operand (and, ring forms, weight) stages + the rows' norm factors
constexpr size_t pgemm_lds(int NTW, int WR, int RING, int TWO, int MTB) {
  const int cols = (4 / WR) * NTW, rows = MTB * 16;
  return (RING ? (size_t)RING * (12 * rows + cols * 64) : (size_t)2 * 12 * rows) * 16 + (TWO ? 0 : rows * 4);
}

// The switches a pick reads, as plain values (pick_env: as a handle holds them).
struct PickEnv {
  int pass;            // 0: decode rows; PF_GROUPED / PF_PGEMM: a prompt pass's row group and this kernel's family
  int fused;           // decode: 1 = one row with the fused o_proj in effect, 2 = 2 .. fuse2_rows rows with it (SPARKMI_FUSE2_ROWS)
  int stamps, exact, tune2;
  int pf_mask, pf_rows, has_pf;   // helper-block prefetch: the producers' mask, the row bound, and whether this launch has a target
  int kv_f32;
  int pg_split_rows;
  int lm_restricted;   // the step's lm_head reads only the constrained rows' tiles
  int lm_blocks;       // blocks of the persistent lm_head
  int lm_screen;       // one greedy row whose logits nobody reads: the int8 screen in front of the listed-tile lm_head
};
// One launch as a pick decided it.
struct GemmPick {
  int form = GF_BAD, kv_f32 = 0;
  int launches = 0;                          // kernels started: 2 with a combine, one per 32 rows for the persistent lm_head above 16
  int gx = 0, gy = 1, block = 0; size_t lds = 0;
  int gx2 = 0;                               // blocks (of 64) of the k_resid_comb that follows
  int work_blocks = 0, ldsb = 0, lt_shift = 0, kseg = 0;   // GemmP's fields of the same names
  int nsplit = 1, mtiles = 0;                // split-K: K segments (= grid y) and 16-row tiles of the slab
  int lm_groups = 0;                         // the persistent lm_head's ngroups argument
};

// idle CUs warm the L2 of their own XCD for a later kernel (decode with few rows only): (256 - work) / 8 * 8 extra blocks where
// the producer's mask bit, a target and the row bound allow and the work leaves room
int helper_blocks(const PickEnv& e, int bit, int M, int work) {
  return (e.pf_mask & bit) && e.has_pf && M <= e.pf_rows && work < 232 ? (256 - work) / 8 * 8 : 0;
}

// The k_gemm block shape of form f0 (its LEAN 0 form) over M rows; f1 / f2: the shape's LEAN 1 / one-row forms where the shape
// runs at such row counts.  One m-tile, up to 5 rows: the operand is staged through wave-private LDS while it fits the cap -- then
// one row takes LEAN 2, 2 .. 5 rows LEAN 1; 6 rows and more, or stamps on, take LEAN 0.
GemmPick pick_kgemm(int f0, int f1, int f2, int KT, int NT, int M, const PickEnv& e) {
  const KgShape& s = kg_shape(f0);
  GemmPick k;
  k.kv_f32 = s.EPI == EPI_QKV ? e.kv_f32 : 0;
  k.work_blocks = (NT + s.NTB - 1) / s.NTB * s.H;
  k.lds = (size_t)s.NW * s.NTB * s.MT * 1024 + 32 * 4 + s.NTB * 32 * 8;
  if (s.MT == 1 && M <= 5) {
    const int tw = (KT + s.NW - 1) / s.NW;               // k tiles per wave
    const size_t per_wave = (size_t)tw * 12 * M * 16;
    // (blocks of 14+ waves are alone on their CU anyway: down_proj's ten k tiles per wave then fit up to 3 rows -- 2 rows: down_proj
    // 8.7 -> 7.3 us, graph step 718 -> 690 us; at 4 rows (123 KB) a tie, so the cap stays below it)
    if (per_wave * s.NW <= (size_t)(s.NW >= 14 ? 96 : 40) * 1024) {
      k.ldsb = (int)per_wave;
      int sh = 4;                                         // 16 lanes fetch 12 pieces (M = 1)
      while ((1 << sh) < 12 * M) ++sh;
      k.lt_shift = sh;
      k.lds += per_wave * s.NW;
    }
  }
  const int lean = s.MT == 1 && s.EPI != EPI_LM && k.ldsb > 0 && !e.stamps ? (M == 1 ? 2 : 1) : 0;
  k.form = lean == 2 ? f2 : lean == 1 ? f1 : f0;
  k.gx = k.work_blocks + helper_blocks(e, s.EPI == EPI_QKV ? 1 : 4, M, k.work_blocks);
  k.gy = (M + s.MT * 16 - 1) / (s.MT * 16);   // one block row per MT * 16 rows
  k.block = s.NW * 64;
  k.launches = 1;
  return k;
}
GemmPick pick_x(int form, int NT, int M, const PickEnv& e) {
  GemmPick k;
  k.form = form; k.kv_f32 = x_shape(form).EPI == EPI_QKV ? e.kv_f32 : 0;
  k.gx = (NT + 3) / 4; k.gy = (M + 15) / 16; k.block = 256; k.launches = 1;
  return k;
}
// nsplit > 1 (PG_RES_FEW): one block per (tile, K segment) writes its segment's sums to the slab and k_resid_comb adds the
// segments in order and runs the epilogue -- the few-row form of the segmented sum (GemmP::kseg), same bits as the in-block form
GemmPick pick_pgemm(int form, int NT, int M, int kseg, int nsplit, const PickEnv& e) {
  const PgShape& s = pg_shape(form);
  const int cols = (4 / s.WR) * s.NTW, rows = s.MTB * 16;   // weight tiles / rows per block
  const int bx = (NT + cols - 1) / cols, by = (M + rows - 1) / rows;
  GemmPick k;
  k.form = form; k.kv_f32 = s.EPI == EPI_QKV ? e.kv_f32 : 0;
  k.gx = s.XMAP || nsplit > 1 ? bx * by : bx; k.gy = nsplit > 1 ? nsplit : s.XMAP ? 1 : by;
  k.block = 256; k.lds = pgemm_lds(s.NTW, s.WR, s.RING, s.TWO, s.MTB);
  k.kseg = kseg; k.nsplit = nsplit; k.mtiles = (M + 15) / 16;
  k.launches = nsplit > 1 ? 2 : 1;
  if (nsplit > 1) k.gx2 = NT * k.mtiles;
  return k;
}
// a prompt pass's row group on k_pgemm: regs / few / many = the kernel's three forms; K in nseg segments (0: one sum)
constexpr int kPgSplitRows = 512;        // passes of up to this many rows run o_proj / down_proj in k_pgemm's split-K form
GemmPick pick_pgemm_rows(int regs, int few, int many, int KT, int NT, int M, int nseg, const PickEnv& e) {
  const int kseg = nseg ? (KT + nseg - 1) / nseg : 0;
  if (e.tune2 & kTune2PgemmRegs) return pick_pgemm(regs, NT, M, kseg, 1, e);
  if (M <= e.pg_split_rows) return pick_pgemm(few, NT, M, kseg, kseg ? (KT + kseg - 1) / kseg : 1, e);
  return pick_pgemm(many, NT, M, kseg, 1, e);
}

GemmPick pick_qkv(int KT, int NT, int M, const PickEnv& e) {
  if (e.exact) return pick_x(GF_X_QKV, NT, M, e);
  if (e.pass == PF_PGEMM) return pick_pgemm_rows(GF_PG_QKV_REGS, GF_PG_QKV_FEW, GF_PG_QKV_MANY, KT, NT, M, 0, e);
  // decode rows stay one m-tile with a block row per 16 rows: few n tiles (N = 1152), so 16-row blocks put twice the CUs to
  // work and halve the operand bytes per CU (measured at M = 32); a prompt pass's row group takes two m-tiles above 16 rows
  if (e.pass == PF_GROUPED && M > 16) return pick_kgemm(GF_QKV_2M, GF_BAD, GF_BAD, KT, NT, M, e);
  return pick_kgemm(GF_QKV_L0, GF_QKV_L1, GF_QKV_HOT, KT, NT, M, e);
}
GemmPick pick_o(int KT, int NT, int heads, int M, const PickEnv& e) {
  if (e.exact) return pick_x(GF_X_RESID, NT, M, e);
  GemmPick k;
  if (e.pass == PF_PGEMM) return pick_pgemm_rows(GF_PG_RES_REGS, GF_PG_RES_FEW, GF_PG_RES_MANY, KT, NT, M, kPgSegO, e);
  if (e.pass == 0 && e.fused) {   // done by the attention kernel (per-head partials) and gate_up's prologue / the last-arriver head sum
    k.form = GF_NONE;
    return k;
  }
  // no helpers here: warming down_proj's 8.7 MB from o_proj (or from attention / gate_up) stretches the
  // producer by more than the consumer gains (measured, profiles/README.md), so down_proj stays cold
  // four row parts up to 8 rows: 629.8 -> 626.0 us per step once the prologues were down to one round trip; beyond, one part
  // and a block row per 16 rows (few n tiles, as QKV)
  const int h4 = heads == 14 ? GF_O14_H4_L0 : heads == 4 ? GF_O4_H4_L0 : GF_O8_H4_L0;
  k = M <= 8 ? pick_kgemm(h4, h4 + 1, h4 + 2, KT, NT, M, e) : pick_kgemm(h4 + 3, GF_BAD, GF_BAD, KT, NT, M, e);
  if (e.pass) k.kseg = (KT + kPgSegO - 1) / kPgSegO;   // (a pass's o_proj operands carry it in every family)
  return k;
}
constexpr int kGu1Lo = 4;                // rows from which (up to 16) gate_up runs the one-batch, three-tile shape with one m-tile
constexpr int kGu1Rows = 32;             // rows up to which gate_up runs its one-batch, three-tile shape
GemmPick pick_gu(int KT, int NT, int heads, int M, const PickEnv& e) {
  if (e.exact) return pick_x(GF_X_GU, NT, M, e);
  if (e.pass == PF_PGEMM) return pick_pgemm_rows(GF_PG_GU_REGS, GF_PG_GU_FEW, GF_PG_GU_MANY, KT, NT, M, 0, e);
  // two m-tiles: the operand triples (12 * M pieces per k tile) outweigh the weight tile 6:1, so where there are
  // n tiles to spare (gate_up: 608) a block takes several of them per operand fetch.  Any NTB gives the same bits:
  // a tile's k -> wave map does not change.  (Measured at M = 32: gate_up 19.4 -> 13.7 us with two, 14.4 with 4;
  // QKV / o_proj / down / lm_head lose with fewer blocks.)
  // 17..32 rows: three n tiles per block and ALL of a wave's k tiles in one batch -- every load of the block leaves at
  // entry (one memory round trip instead of two dependent ones; 233 VGPRs, one 8-wave block per CU, 203 blocks):
  // gate_up 12.8 -> 10.5 us, batch-32 step 1047 -> 998 us.  Beyond 32 rows (two block rows = 406 blocks, two rounds
  // at one block per CU) the two-tile, two-batch shape stays: two k tiles in flight, 13.9 -> 13.6 us at 32 rows, 18.5 -> 17.5 at 64.
  // (five n tiles per block in two batches -- 244 blocks, one round: 13.3 us against 10.3, step 947 -> 1017: not a rounds problem)
  if (M > kGu1Rows) return pick_kgemm(GF_GU_2M2, GF_BAD, GF_BAD, KT, NT, M, e);
  if (M > 16) return pick_kgemm(GF_GU_2M3, GF_BAD, GF_BAD, KT, NT, M, e);
  // kGu1Lo..16 rows: three n tiles per block and all of a wave's k tiles in one batch, as at 17..32 rows -- every load
  // of the block leaves at entry (one memory round trip).  8 rows 8.0 -> 6.9 us (graph step 801 -> 773 us), 16 rows 9.5 -> 7.9
  // (855 -> 817), 5 rows 763 -> 751, 4 rows 749 -> 742, 2 rows a tie (below 4 rows the operands staged through wave-private LDS
  // stay); same bits (the k tile -> wave map does not change).
  if (M >= kGu1Lo) return pick_kgemm(GF_GU3_L0, GF_GU3_L1, GF_BAD, KT, NT, M, e);
  if (e.pass) return pick_kgemm(GF_GUP_L0, GF_GUP_L1, GF_GUP_L2, KT, NT, M, e);
  GemmPick k = pick_kgemm(GF_GU_L0, GF_GU_L1, GF_GU_L2, KT, NT, M, e);
  if (e.fused == 1 && k.form == GF_GU_L2) {   // the hot entry of the two fused head counts; + the heads' norm partials in LDS
    k.form = heads == 14 ? GF_GU_FO14 : heads == 4 ? GF_GU_FO4 : GF_BAD;
    k.lds += 1024;
  }
  return k;
}
// rows from which down_proj runs chain-split (k_downC): graph step at 0.5B, same box (profiles/r04_batch_ab.txt): 4 rows 641 (k_downS) vs
// 692 us (chains), 8 rows 728 vs 713, 16 rows 790 (k_gemm<.., H = 4>) vs 744, 32 rows 892 vs 859
// (5 / 6 rows: 731 / 728 us with the chains, the same as k_downS within noise -- the chains take over from 7)
constexpr int kDcMin = 7;
GemmPick pick_d(int KT, int NT, int M, const PickEnv& e) {
  if (e.exact) return pick_x(GF_X_RESID, NT, M, e);
  if (e.pass == PF_PGEMM) return pick_pgemm_rows(GF_PG_RES_REGS, GF_PG_RES_FEW, GF_PG_RES_MANY, KT, NT, M, kPgSegD, e);
  GemmPick k;
  if (e.pass) {   // a prompt pass's row group on k_gemm
    k = M > 16 ? pick_kgemm(GF_D_2M, GF_BAD, GF_BAD, KT, NT, M, e) : pick_kgemm(GF_D_H1_L0, GF_D_H1_L1, GF_D_H1_L2, KT, NT, M, e);
    k.kseg = (KT + kPgSegD - 1) / kPgSegD;   // (a pass's down_proj operands carry it in every family)
    return k;
  }
  const bool own = !e.stamps && KT <= 160;   // down_proj's own kernels: a chain's k tiles in registers (TPC <= 10), no stamps
  const int t = GF_D1_2 + (KT <= 32 ? 0 : KT <= 96 ? 1 : 2) * (GF_D1_6 - GF_D1_2);   // the TPC = 2 / 6 / 10 forms
  if (own && M >= kDcMin && M <= kMaxRows && NT % 4 == 0) {
    // kDcMin .. 64 rows: the 16 chains on 16 different blocks + an in-order combine (k_downC, k_resid_comb); 1 / 2 / 4 m-tiles
    const int mtn = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    k.form = t + (GF_DC_2_1 - GF_D1_2) + (mtn == 1 ? 0 : mtn == 2 ? 1 : 2);
    k.gx = NT / 4 * 16; k.block = 256; k.gx2 = NT * mtn; k.launches = 2;
    k.lds = (size_t)dn_shape(k.form).TPC * 12 * (M < mtn * 16 ? M : mtn * 16) * 16;   // > 64 KiB from 35 rows at TPC = 10
    return k;
  }
  k.work_blocks = NT * 4;   // four row parts per weight tile
  // one row: four chains per wave, full load instructions (k_down1_hot; same bits).  SPARKMI_TUNE2 bit kTune2GemmDown1 keeps k_gemm (A/B)
  if (own && M == 1 && !(e.tune2 & kTune2GemmDown1)) {
    k.form = t; k.gx = k.work_blocks + helper_blocks(e, 4, M, k.work_blocks); k.block = 256; k.launches = 1;
    return k;
  }
  // 2 .. 8 rows in groups of four (k_downS).  SPARKMI_TUNE2 bit kTune2GemmDownS keeps k_gemm (A/B)
  if (own && M >= 2 && M <= 8 && !(e.tune2 & kTune2GemmDownS)) {
    k.form = t + (M <= 4 ? GF_DS_2_1 : GF_DS_2_2) - GF_D1_2; k.gx = k.work_blocks; k.block = 256; k.launches = 1;
    return k;
  }
  // k_gemm: 4-row parts at few rows (224 blocks, -0.7 us); same bits either way, the zero-fed MFMAs cost at M > 8
  // row parts (H blocks per weight tile) while the operand re-reads they cost stay small: measured step at
  // 16 / 32 / 64 rows with H = 1 | 2 | 4: 930 | 915 | 900, 1064 | 1055 | 1161, 1318 | 1443 | 1671 us
  // (one m-tile and a block row per 16 rows at every row count: WB batches of weight tiles requested at entry, so down_proj's
  // five batches wait for L2 operand round trips only, not for five dependent HBM round trips)
  if (M <= 16) return pick_kgemm(GF_D_H4_L0, GF_D_H4_L1, GF_D_H4_L2, KT, NT, M, e);
  if (M <= 32) return pick_kgemm(GF_D_H2, GF_BAD, GF_BAD, KT, NT, M, e);
  return pick_kgemm(GF_D_H1_L0, GF_BAD, GF_BAD, KT, NT, M, e);
}
// blocks of the persistent lm_head for M rows: lm_blocks, two resident per CU, up to 16 rows; one per CU beyond
int lm_pass_blocks(int lm_blocks, int M) { return M <= 16 ? lm_blocks : (lm_blocks < 256 ? lm_blocks : 256); }
GemmPick pick_lm(int KT, int NT, int M, const PickEnv& e) {
  if (e.exact) return pick_x(GF_X_LM, NT, M, e);
  if (KT > 32) return pick_kgemm(M > 16 ? GF_LM_2M : GF_LM_1M, GF_BAD, GF_BAD, KT, NT, M, e);
  // The persistent lm_head: 16 rows' operand resident in the registers of a 4-wave group.  Restricted: the same kernel for the same
  // row count, its groups from the tile list (ngroups = 0)
  GemmPick k;
  const int rt = e.lm_restricted ? 1 : 0;
  const size_t lds = (size_t)4 * 2 * 1024 + 32 * 4 + 2 * 32 * 8;
  k.gx = lm_pass_blocks(e.lm_blocks, M); k.lm_groups = rt ? 0 : (NT + 1) / 2;
  if (e.lm_screen && M == 1 && !rt) {   // the recompute keeps today's grid: k_finalize reads the same partial columns
    k.form = GF_LM1_SCR; k.block = 256; k.lds = lds; k.launches = 3; k.lm_groups = 0;
    return k;
  }
  if (M <= 16) {
    k.form = GF_LM1 + rt; k.block = 256; k.lds = lds; k.launches = 1;
    return k;
  }
  // 32 rows per pass: one 4-wave block per CU, the second m-tile's operands in LDS (k_lm32);
  // SPARKMI_TUNE2 bit kTune2Lm2: the two-group kernel (k_lm<2>) for A/B
  const size_t lds32 = (size_t)4 * 2 * 2 * 1024 + 32 * 4 + 2 * 32 * 8 + (size_t)KT * 12 * 16 * 16;
  k.launches = (M + 31) / 32;
  if (!(e.tune2 & kTune2Lm2) && lds32 <= 150 * 1024) {
    k.form = (KT <= 28 ? GF_LM32_7 : GF_LM32_8) + rt; k.block = 256; k.lds = lds32;
  } else {
    k.form = GF_LM2 + rt; k.block = 512; k.lds = 2 * lds;
  }
  return k;
}

// the form's kernel(s) by name, template arguments as numbers (as a kernel trace prints them, without blanks)
void gemm_form_name(const GemmPick& k, char* out, size_t n) {
  const int f = k.form;
  if (f <= GF_NONE) snprintf(out, n, "%s", "");
  else if (f < GF_KG_END) {
    const KgShape& s = kg_shape(f);
    snprintf(out, n, "%s<%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d>", s.hot ? "k_gemm_hot" : "k_gemm", s.MT, s.NTB, s.NW, s.U, s.WB, s.PRO, s.EPI,
             k.kv_f32, s.H, s.OCC, s.LEAN, s.NOH);
  } else if (f < GF_DN_END) {
    const DnShape& s = dn_shape(f);
    if (s.kernel == DN_DOWN1) snprintf(out, n, "k_down1_hot<%d>", s.TPC);
    else if (s.kernel == DN_DOWNS) snprintf(out, n, "k_downS<%d,%d>", s.TPC, s.N);
    else snprintf(out, n, "k_downC<%d,%d>+k_resid_comb<0,0>", s.TPC, s.N);
  } else if (f < GF_PG_END) {
    const PgShape& s = pg_shape(f);
    snprintf(out, n, "k_pgemm<%d,%d,%d,%d,%d,%d,%d,%d,%d>%s", s.PRO, s.EPI, k.kv_f32, s.NTW, s.WR, s.RING, s.XMAP, s.TWO, s.MTB,
             k.nsplit > 1 ? "+k_resid_comb<1,1>" : "");
  } else if (f < GF_LM_END) {
    const LmShape& s = lm_shape(f);
    if (s.RT == 2) snprintf(out, n, "k_lm_screen+k_lm_select+k_lm<%d,1,1>", s.A);
    else snprintf(out, n, "%s<%d,%d>", s.k32 ? "k_lm32" : "k_lm", s.A, s.RT);
  } else {
    const XShape& s = x_shape(f);
    snprintf(out, n, "k_gemm_x<%d,%d,%d>", s.PRO, s.EPI, k.kv_f32);
  }
}
// the name of an lm_head form as smi_llm_debug_head reports it (null: not an lm_head form)
const char* lm_form_note(int form) {
  if (form > GF_PG_END && form < GF_LM_END) return lm_shape(form).note;
  return form == GF_LM_1M ? "k_gemm<1,EPI_LM>" : form == GF_LM_2M ? "k_gemm<2,EPI_LM>" : form == GF_X_LM ? "k_gemm_x<EPI_LM>" : nullptr;
}

const unsigned char* sec(const smi_llm* L, int s, int layer) {
  if (s >= SMI_LLM_FINAL_NORM) return L->arena + L->lay.off[s];
  return L->arena + L->lay.layers_base + (size_t)layer * L->lay.layer_stride + L->lay.off[s];
}

void* kv_layer(const smi_llm* L, void* base, int layer) {
  const size_t esz = L->cfg.kv_dtype ? 4 : 2;
  return (unsigned char*)base + (size_t)layer * L->kv_layer_elems * esz;
}

#ifndef SMI_DIAG   // product build: no engine (the launch path everywhere)
inline bool eng_usable(const smi_llm*, const RowDesc*, int) { return false; }
inline int eng_launch(smi_llm*, hipStream_t) { return SMI_OK; }
inline int eng_check(smi_llm*) { return SMI_OK; }
#else
// ---- one-row decode engine (smi_eng.h): build at create, launch in place of the 4 x layers launches of a one-row step
void eng_destroy(smi_llm* L) {
  EngState& E = L->eng;
  E.plan.reset(); E.stream.reset(); E.gran.reset(); E.words.reset(); E.stamps.reset();
  E.enabled = 0;
}

// Not an error when the engine does not apply (other KV type, paged cache, odd shapes, small device): `why` says so and the
// launch path is used.  An allocation failure IS reported.  (eng_create releases what a build that did not finish left.)
int eng_build(smi_llm* L) {
  EngState& E = L->eng;
  const smi_llm_cfg& c = L->cfg;
  E.enabled = 0;
  auto skip = [&](const char* m) { snprintf(E.why, sizeof(E.why), "%s", m); return SMI_OK; };
  { const char* e = smi_env("SPARKMI_ENGINE"); if (e && e[0] == '0') return skip("SPARKMI_ENGINE=0"); }
  if (c.kv_dtype != 0) return skip("f32 KV cache");
  if (L->exact) return skip("exact-weights mode");
  if (L->paged) return skip("paged KV cache");
  int dev = 0, ncu = 0;
  SMI_HIP(hipGetDevice(&dev));
  SMI_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  { const char* e = smi_env("SPARKMI_ENGINE_CUS"); if (e && atoi(e) > 0 && atoi(e) <= ncu) ncu = atoi(e); }
  EngPlanHost P;
  char why[128];
  if (!eng_build_plan(L->H, L->Q, L->KV, L->I, c.num_heads, ncu, P, why, sizeof(why))) return skip(why);
  const EngLds lds = eng_lds(L->H, P.g.KT[EPH_DOWN], P.g.KT[EPH_QKV] > P.g.KT[EPH_O] ? P.g.KT[EPH_QKV] : P.g.KT[EPH_O]);
  if (lds.total > 160 * 1024 - 512) return skip("LDS image too large");
  E.ncu = ncu; E.maxlen = P.maxlen; E.lds = lds.total;
  E.gran_per_buf = 2 * L->H + (L->Q + 2 * L->KV) + L->Q + L->I;
  { const char* e = smi_env("SPARKMI_ENGINE_BURST"); E.ld_burst = e && atoi(e) > 0 ? atoi(e) : 16; }
  { const char* e = smi_env("SPARKMI_ENGINE_POLL"); E.poll_quiet = e ? atoi(e) : 1; }
  { const char* e = smi_env("SPARKMI_ENGINE_DELAYS"); for (int i = 0; i < 5; ++i) E.edge_delay[i] = 16; if (e) sscanf(e, "%d,%d,%d,%d,%d", &E.edge_delay[0], &E.edge_delay[1], &E.edge_delay[2], &E.edge_delay[3], &E.edge_delay[4]); }
  { const char* e = smi_env("SPARKMI_ENGINE_SLEEP"); E.ld_sleep = e && atoi(e) >= 0 ? atoi(e) : 0; }
  { const char* e = smi_env("SPARKMI_ENGINE_TIMEOUT_MS"); const double ms = e ? atof(e) : 500.0; E.timeout_ticks = (unsigned)((ms > 1.0 ? ms : 1.0) * 1e5); }
  const size_t ncw = (size_t)ncu;   // one stream per CU
  const size_t stream_bytes = (size_t)c.num_layers * ncw * P.maxlen * 1024;
  DevBuf<uint32_t> desc_dev;   // the two temporaries of the packing launch
  DevBuf<uint16_t> lens_dev;
  int rc;
  if ((rc = E.plan.alloc(P.cu.size() * sizeof(EngCuPlan), "engine plan")) || (rc = E.stream.alloc(stream_bytes, "engine weight stream")) ||
      (rc = E.gran.alloc_zero((size_t)2 * E.gran_per_buf * 8, "engine granules")) || (rc = E.words.alloc_zero(256, "engine words")) ||
      (rc = E.stamps.alloc_zero((size_t)3 * c.num_layers * 16 * 8, "engine stamps")) ||
      (rc = desc_dev.alloc(P.desc.size() * 4, "engine descriptors")) || (rc = lens_dev.alloc(P.lens.size() * 2, "engine lengths"))) return rc;
  SMI_HIP(hipMemcpy(E.plan, P.cu.data(), P.cu.size() * sizeof(EngCuPlan), hipMemcpyHostToDevice));
  SMI_HIP(hipMemcpy(desc_dev, P.desc.data(), P.desc.size() * 4, hipMemcpyHostToDevice));
  SMI_HIP(hipMemcpy(lens_dev, P.lens.data(), P.lens.size() * 2, hipMemcpyHostToDevice));
  EngPackP pk;
  memset(&pk, 0, sizeof(pk));
  pk.desc = desc_dev; pk.lens = lens_dev; pk.maxlen = P.maxlen; pk.ncw = (int)ncw;
  pk.arena = L->arena; pk.layers_base = L->lay.layers_base; pk.layer_stride = L->lay.layer_stride;
  const int secs[4] = {SMI_LLM_WQKV, SMI_LLM_WO, SMI_LLM_WGU, SMI_LLM_WD};
  for (int ph = 0; ph < 4; ++ph) { pk.woff[ph] = L->lay.off[secs[ph]]; pk.KT[ph] = P.g.KT[ph]; pk.NW[ph] = P.g.NW[ph]; pk.wperm[ph] = 0; }
  pk.wperm[EPH_DOWN] = L->wd_parts;
  pk.out = (uint4*)E.stream.get();
  const size_t imgs = ncw * P.maxlen;
  hipLaunchKernelGGL(k_eng_pack, dim3((unsigned)((imgs + 3) / 4), (unsigned)c.num_layers), dim3(256), 0, 0, pk);
  SMI_HIP(hipGetLastError());
  SMI_HIP(hipDeviceSynchronize());   // (the packing launch is done before its two temporaries go)
  if (hipFuncSetAttribute((const void*)k_engine, hipFuncAttributeMaxDynamicSharedMemorySize, E.lds) != hipSuccess) {
    (void)hipGetLastError();
    return skip("hipFuncSetAttribute(LDS) refused");
  }
  snprintf(E.why, sizeof(E.why), "on: %d CUs, %d images per wave and layer at most, %d B of LDS", ncu, P.maxlen, E.lds);
  E.enabled = 1;
  return SMI_OK;
}

int eng_create(smi_llm* L) {
  const int rc = eng_build(L);
  if (rc || !L->eng.enabled) eng_destroy(L);
  return rc;
}

// the one-row step the engine stands for: one live sequence in slot 0, contiguous bf16 cache, one context segment (its layers
// only: lm_head, the sampler and k_finalize stay launches, so a sampling record applies to the engine's row as to any other)
bool eng_usable(const smi_llm* L, const RowDesc* rows, int M) {
  return L->eng.enabled && L->eng_on && M == 1 && rows == L->rows && L->identity_slots && !L->paged && L->attn_seg <= 1 && !L->stamps_on &&
         !(step_feat(L) & (F_LP | F_BIAS | F_STOP | F_NGRAM));   // (a step with a log-probability, biased, stop-sequence or n-gram row keeps to the launch path)
}

int eng_launch(smi_llm* L, hipStream_t st) {
  const EngState& E = L->eng;
  const smi_llm_cfg& c = L->cfg;
  EngP p;
  memset(&p, 0, sizeof(p));
  p.H = L->H; p.Q = L->Q; p.KV = L->KV; p.I = L->I; p.n_heads = c.num_heads; p.n_kv = c.num_kv_heads; p.layers = c.num_layers;
  p.max_pos = c.max_positions; p.eps = c.rms_eps;
  const EngGeom g = eng_geom(L->H, L->Q, L->KV, L->I, c.num_heads);
  for (int ph = 0; ph < 4; ++ph) { p.KT[ph] = g.KT[ph]; p.NW[ph] = g.NW[ph]; }
  p.plan = E.plan; p.stream = E.stream; p.maxlen = E.maxlen; p.ncu = E.ncu;
  p.arena = L->arena; p.layers_base = L->lay.layers_base; p.layer_stride = L->lay.layer_stride;
  p.off_ln1 = L->lay.off[SMI_LLM_LN1]; p.off_bqkv = L->lay.off[SMI_LLM_BQKV]; p.off_ln2 = L->lay.off[SMI_LLM_LN2];
  p.final_norm = (const float*)(L->arena + L->lay.off[SMI_LLM_FINAL_NORM]);
  p.rope = (const float2*)(L->arena + L->lay.off[SMI_LLM_ROPE]);
  p.rows = L->rows; p.h = L->dec.h; p.ss_in = L->dec.ss; p.xs_out = L->dec.xs_h; p.ss_out = L->dec.ss;
  p.kcache = (uint16_t*)L->kcache.get(); p.vcache = (uint16_t*)L->vcache.get(); p.kv_layer_elems = L->kv_layer_elems;
  p.gran = E.gran; p.serial = E.words; p.err = E.words + 4; p.arrive = E.words + 8;
  p.timeout_ticks = E.timeout_ticks;
  p.ld_burst = E.ld_burst; p.ld_sleep = E.ld_sleep; p.poll_quiet = E.poll_quiet;
  for (int i = 0; i < 5; ++i) p.edge_delay[i] = E.edge_delay[i];
  p.stamps = smi_env("SPARKMI_ENGINE_STAMPS") ? E.stamps : nullptr;
  hipLaunchKernelGGL(k_engine, dim3(E.ncu), dim3(kEngBlock), E.lds, st, p);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

// After a stream synchronisation: did an engine launch give up on a hand-off?  (bounded spins, smi_eng_comm.h)
int eng_check(smi_llm* L) {
  if (!L->eng.enabled) return SMI_OK;
  unsigned e[2] = {0, 0};
  SMI_HIP(hipMemcpy(e, L->eng.words + 4, 8, hipMemcpyDeviceToHost));
  if (e[0] == 0) return SMI_OK;
  SMI_HIP(hipMemset(L->eng.words + 4, 0, 8));
  L->started = 0;
  smi_set_error("decode engine: a hand-off timed out (layer %u, edge %u) -- are all %d CUs free for this stream?  SPARKMI_ENGINE=0 selects the launch path",
                (e[1] - 1) / 8, (e[1] - 1) % 8, L->eng.ncu);
  return SMI_EHIP;
}
#endif   // SMI_DIAG

enum { KQKV = 0, KATTN, KO, KGU, KD, KLM, KFIN };

int ensure_apart(smi_llm* L, size_t floats) {
  if (floats * 4 <= L->apart.bytes()) return SMI_OK;
  graphs_flush(L);   // captured steps hold the old buffer's address
  return L->apart.ensure(floats * 4, "attention partials");
}

// lm_head partial columns (= persistent blocks) finalize / the sampler read for M live rows
int lm_blocks_for(const smi_llm* L, int M) {
  if (L->KTh > 32 || L->exact) return L->lm_cap;
  return lm_pass_blocks(L->lm_blocks, M);
}

// ids per set of k_penalize's partition of a row into nblk sets: a multiple of 4 (aligned float4 sets)
int pen_set_ids(int V, int nblk) { return ((V + nblk - 1) / nblk + 3) & ~3; }

// k_logprob's arguments for a step of M rows (the lm_head's maxima, the handle's sampler settings)
LpP lp_params(const smi_llm* L, int M) {
  LpP lp;
  lp.logits = L->logits; lp.ctl = L->ctl; lp.rows = L->rows; lp.pval = L->pval; lp.nblk = lm_blocks_for(L, M);
  lp.V = L->cfg.vocab_size; lp.per = pen_set_ids(lp.V, kLpBlocks); lp.inv_temp = 1.0f / L->temperature; lp.hs = L->do_sample;
  lp.part = L->lp_part; lp.rowc = L->lp_rowc;
  return lp;
}

// k_penalize's arguments for a step of M rows; a caller whose rows have bias entries adds the sequence records (PenP::seq)
PenP pen_params(const smi_llm* L, int M) {
  PenP pp;
  pp.logits = L->logits; pp.hist = L->phist; pp.ctl = L->ctl; pp.rows = L->rows; pp.pval = L->pval; pp.pidx = L->pidx;
  pp.V = L->cfg.vocab_size; pp.nblk = lm_blocks_for(L, M); pp.per = pen_set_ids(pp.V, pp.nblk); pp.hs = L->do_sample;
  pp.seq = nullptr; pp.ghist = L->hist; pp.max_steps = L->max_steps;
  return pp;
}

// k_ngram_ban's arguments and dynamic LDS for a step: the tail, and the whole context when max_positions ids fit in 48 KiB
NgramP ngram_params(const smi_llm* L, size_t* lds) {
  NgramP np;
  np.logits = L->logits; np.ctl = L->ctl; np.rows = L->rows; np.pctx = L->pctx; np.ghist = L->hist;
  np.V = L->cfg.vocab_size; np.max_pos = L->cfg.max_positions; np.max_steps = L->max_steps;
  np.lds_ids = L->cfg.max_positions <= 12288 - SMI_MAX_NGRAM ? L->cfg.max_positions : 0;
  *lds = (size_t)(SMI_MAX_NGRAM + np.lds_ids) * 4;
  return np;
}

// the sampler kernels' arguments for a step of M rows (the handle's settings; the lm_head's maxima as the top-k bound)
SampleP sample_params(const smi_llm* L, int M) {
  SampleP sp;
  sp.logits = L->logits; sp.V = L->cfg.vocab_size; sp.top_k = L->top_k; sp.inv_temp = 1.0f / L->temperature;
  sp.top_p = L->top_p; sp.hs = L->do_sample; sp.ctl = L->ctl; sp.rows = L->rows; sp.tok = L->tok;
  sp.pval = L->pval; sp.nblk = lm_blocks_for(L, M);
  sp.cand_v = L->cand_v; sp.cand_i = L->cand_i; sp.cand_n = L->cand_n;
  return sp;
}

// k_finalize's arguments for a step of M rows in which no row samples, is penalised, returns log-probabilities or has a stop
// sequence: the caller adds what the kernels it ran before left (FinP::tok, phist, lp*) and the stop records (FinP::seq)
FinP fin_params(const smi_llm* L, int M) {
  FinP f;
  f.tok = nullptr; f.hs = L->do_sample; f.phist = nullptr;
  f.lp = nullptr; f.lp_part = nullptr; f.lp_rowc = nullptr; f.logits = L->logits;
  f.pval = L->pval; f.pidx = L->pidx; f.M = M; f.KT = L->KTh; f.V = L->cfg.vocab_size; f.nblk = lm_blocks_for(L, M);
  f.rows = L->rows; f.hist = L->hist; f.count = L->count; f.finished = L->finished; f.step = L->step;
  f.ctl = L->ctl; f.Wlm = (const uint16_t*)sec(L, SMI_LLM_LM_HEAD, 0); f.h = L->dec.h; f.max_steps = L->max_steps;
  f.gamma0 = (const float*)sec(L, SMI_LLM_LN1, 0); f.xs = L->dec.xs_h; f.sspart = L->dec.ss; f.npart = L->NTh * 4; f.exact = L->exact;
  f.seq = nullptr;
  return f;
}

#define SMI_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)   // a failed step ends the composition

// The token pick's kernels, one launcher each: the only place a kernel's grid, block and dynamic LDS are written.  A decode
// step (launch_one(KFIN)) and the kernel-alone diagnostics (smi_llm_debug_*) are compositions of these, over M rows of L->rows.
int launch_ngram_ban(const smi_llm* L, int M, hipStream_t st) {
  size_t lds;
  const NgramP np = ngram_params(L, &lds);
  hipLaunchKernelGGL(k_ngram_ban, dim3(1, M), dim3(256), lds, st, np);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// seq: the sequence records when some row has a bias entry (stage 0b), else null
int launch_penalize(const smi_llm* L, int M, const SeqRec* seq, hipStream_t st) {
  PenP pp = pen_params(L, M);
  pp.seq = seq;
  hipLaunchKernelGGL(k_penalize, dim3((pp.nblk + kPenWaves - 1) / kPenWaves, M), dim3(256), 0, st, pp);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// k_sample_scan + k_sample, never apart.  use_bound: the lm_head's maxima bound the top-k candidates (a step: always); false:
// the exact radix selection
int launch_sampler(const smi_llm* L, int M, bool use_bound, hipStream_t st) {
  SampleP sp = sample_params(L, M);
  if (!use_bound) sp.pval = nullptr;
  hipLaunchKernelGGL(k_sample_scan, dim3(kScanBlocks, M), dim3(256), 0, st, sp);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sample, dim3(M), dim3(1024), 0, st, sp);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
int launch_logprob(const smi_llm* L, int M, hipStream_t st) {
  const LpP lp = lp_params(L, M);
  hipLaunchKernelGGL(k_logprob, dim3(kLpBlocks, M), dim3(256), 0, st, lp);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// f: fin_params plus what the kernels launched before it left (tok, phist, lp*) and the stop records (seq)
int launch_finalize(const FinP& f, hipStream_t st) {
  hipLaunchKernelGGL(k_finalize, dim3(f.M), dim3(256), 0, st, f);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

int segs_for(int ctx_bound) { return ctx_bound <= kAttnSeg ? 1 : (ctx_bound + kAttnSeg - 1) / kAttnSeg; }

// attention (+ the segment merge when the context bound of the current call exceeds one segment)
template <int KVF32>
int launch_attn(smi_llm* L, AttnP a, hipStream_t st) {
  a.nseg = L->attn_seg < 1 ? 1 : L->attn_seg;
  a.work_blocks = a.n_heads * a.M * a.nseg;
  // (the one-row fused kernel addresses a token's K / V piece by a 32-bit byte offset inside the KV head's row: kFuseMaxPos)
  const bool fuse = a.M == 1 && a.nseg == 1 && a.slot_is_row && a.part_o && !a.cnt && a.max_pos <= kFuseMaxPos;
  const bool fuse2 = a.nseg == 1 && a.slot_is_row && a.part_o && a.cnt;   // (a.cnt is only set by fuse2_now)   // 2 .. 8 rows: fused o_proj + last-arriver head sum
  if (fuse || fuse2) a.work_blocks *= kFuseQB;
  if (a.nseg > 1) {
    int rc = ensure_apart(L, (size_t)a.M * a.n_heads * a.nseg * 66);
    if (rc) return rc;
    a.part = L->apart;
  }
  const int helpers = ((L->sw.prefetch_mask & 2) && a.M <= L->sw.prefetch_rows && a.work_blocks < 232) ? (256 - a.work_blocks) / 8 * 8 : 0;
  const bool pg = a.km.ptab != nullptr;   // paged cache: the slot == row kernels look the token's page up (PG)
#ifdef SMI_DIAG   // measured, not adopted: the product library does not carry these instantiations
  if (fuse2 && pg)
    hipLaunchKernelGGL((k_attn<KVF32, 2, 2, 1>), dim3(a.work_blocks), dim3(2 * kAttnWaves * 64), 0, st, a);
  else if (fuse2)
    hipLaunchKernelGGL((k_attn<KVF32, 2, 2>), dim3(a.work_blocks), dim3(2 * kAttnWaves * 64), 0, st, a);
  else
#endif
  if (fuse && pg)
    hipLaunchKernelGGL((k_attn<KVF32, 1, 1, 1>), dim3(a.work_blocks + helpers), dim3(2 * kAttnWaves * 64), 0, st, a);
  else if (fuse && a.n_heads < 65536 && a.group < 32768)   // the hot entry (beyond the bounds: the struct-only one)
    launch_attn_hot<KVF32>(a, a.work_blocks + helpers, st);
  else if (fuse)
    hipLaunchKernelGGL((k_attn<KVF32, 1, 1>), dim3(a.work_blocks + helpers), dim3(2 * kAttnWaves * 64), 0, st, a);
  else if (a.M == 1 && a.nseg == 1 && a.slot_is_row && pg)
    hipLaunchKernelGGL((k_attn<KVF32, 1, 0, 1>), dim3(a.work_blocks + helpers), dim3(kAttnWaves * 64), 0, st, a);
  else if (a.M == 1 && a.nseg == 1 && a.slot_is_row)
    hipLaunchKernelGGL((k_attn<KVF32, 1>), dim3(a.work_blocks + helpers), dim3(kAttnWaves * 64), 0, st, a);
  else if (a.nseg == 1 && a.slot_is_row && pg)
    hipLaunchKernelGGL((k_attn<KVF32, 2, 0, 1>), dim3(a.work_blocks + helpers), dim3(kAttnWaves * 64), 0, st, a);
  else if (a.nseg == 1 && a.slot_is_row)
    hipLaunchKernelGGL((k_attn<KVF32, 2>), dim3(a.work_blocks + helpers), dim3(kAttnWaves * 64), 0, st, a);
  else
    hipLaunchKernelGGL((k_attn<KVF32, 0>), dim3(a.work_blocks + helpers), dim3(kAttnWaves * 64), 0, st, a);
  SMI_LAUNCH_CHECK();
  if (a.nseg > 1) {
    hipLaunchKernelGGL(k_attn_merge, dim3(a.M), dim3(1024), 0, st, a);
    SMI_LAUNCH_CHECK();
  }
  return SMI_OK;
}

// One live row in its own slot, one context segment: the attention kernel also computes its head's share of the o_proj
// (k_attn<.., FUSE>), gate_up builds its operand from those partials (PRO_FUSEDO) and down_proj adds its residual from h2;
// the o_proj kernel is not launched.  The predicate is the one launch_attn picks the one-row kernel by.
// (the shapes that have the fused path: the two head counts with a gate_up form of their own, hidden tiles the attention blocks share out)
bool fuse_o_fits(int heads, int NTh, int KTh) {
  return (heads == 14 || heads == 4) && heads <= kMaxOHeads && NTh % kFuseQB == 0 && NTh / kFuseQB <= kAttnWaves * kFuseOT && KTh * 8 <= 256;
}
bool fuse_o_now(const smi_llm* L, const RowDesc* rows, int M) {
  return L->fuse_o && M == 1 && rows == L->rows && L->identity_slots && L->attn_seg <= 1;
}
// 2 .. fuse2_rows live rows, each in its own slot, one context segment: the attention kernel also computes the o_proj and the last
// block of a (row, quarter) to arrive finishes the rows (k_attn<.., FUSE = 2>); the o_proj kernel is not launched.
bool fuse2_now(const smi_llm* L, const RowDesc* rows, int M) {
  return L->fuse_o && M >= 2 && M <= L->sw.fuse2_rows && rows == L->rows && L->identity_slots && L->attn_seg <= 1;
}

// ---- The forms' launchers, one per table: the template arguments are a table row's, everything else is the pick's.  A launcher
// enters exactly the instantiations it starts in LdsBig (both cache types where the epilogue appends to the cache).
template <int MT, int NTB, int NW, int U, int WB, int PRO, int EPI, int H, int OCC, int LEAN, int NOH, int HOT>
int launch_kgemm_form(const smi_llm* L, const GemmP& p, const GemmPick& k, hipStream_t st) {
  SMI_REQUIRE(k.lds <= (size_t)kLdsBigBytes, "k_gemm: %zu bytes of LDS", k.lds);
  with_kvf32<EPI>(L, [&](auto kv) {
    if constexpr (HOT) {   // the hot values come from the struct that travels behind them (launch_gemm_hot)
      static_assert(LEAN == 2, "hot entries: the one-row kernels");
      static_cast<void>(LdsBig<k_gemm_hot<MT, NTB, NW, U, WB, PRO, EPI, kv(), H, OCC, LEAN, NOH>>::reg);
      launch_gemm_hot<MT, NTB, NW, U, WB, PRO, EPI, kv(), H, OCC, NOH>(p, dim3(k.gx, k.gy), k.lds, st);
    } else {
      static_cast<void>(LdsBig<k_gemm<MT, NTB, NW, U, WB, PRO, EPI, kv(), H, OCC, LEAN, NOH>>::reg);
      hipLaunchKernelGGL((k_gemm<MT, NTB, NW, U, WB, PRO, EPI, kv(), H, OCC, LEAN, NOH>), dim3(k.gx, k.gy), dim3(NW * 64), k.lds, st, p);
    }
  });
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// down_proj's own kernels; DN_DOWNC: the chains split over blocks (k_downC) and the in-order combine + RESID epilogue (k_resid_comb)
template <int KERNEL, int TPC, int N>
int launch_down_form(const smi_llm* L, const GemmP& p, const GemmPick& k, hipStream_t st) {
  if constexpr (KERNEL == DN_DOWN1) launch_down1_hot<TPC>(p, k.gx, st);
  else if constexpr (KERNEL == DN_DOWNS) hipLaunchKernelGGL((k_downS<TPC, N>), dim3(k.gx), dim3(256), 0, st, p);
  else {
    DownCP d;
    d.W = p.W; d.NT = p.NT; d.KT = p.KT; d.M = p.M; d.wperm = p.wperm; d.XS = p.XS; d.part = L->dpart;
    d.Y = p.Y; d.Yin = p.Yin; d.gamma_next = p.gamma_next; d.XSout = p.XSout; d.ssout = p.ssout;
    static_cast<void>(LdsBig<k_downC<TPC, N>>::reg);
    SMI_REQUIRE(k.lds <= (size_t)kLdsBigBytes, "k_downC: %zu bytes of LDS", k.lds);
    hipLaunchKernelGGL((k_downC<TPC, N>), dim3(k.gx), dim3(256), k.lds, st, d);
    SMI_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_resid_comb<0, 0>), dim3(k.gx2), dim3(64), 0, st, d, 16, N);
  }
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// One prefill GEMM over a row group with k_pgemm; k.nsplit > 1: split-K through L->pslab + k_resid_comb
template <int PRO, int EPI, int NTW, int WR, int RING, int XMAP, int TWO, int MTB>
int launch_pgemm_form(const smi_llm* L, GemmP p, const GemmPick& k, hipStream_t st) {
  if constexpr (pgemm_lds(NTW, WR, RING, TWO, MTB) > 64 * 1024) {
    static_assert(pgemm_lds(NTW, WR, RING, TWO, MTB) <= (size_t)kLdsBigBytes, "k_pgemm: LDS beyond the opted-in window");
    with_kvf32<EPI>(L, [&](auto kv) { static_cast<void>(LdsBig<k_pgemm<PRO, EPI, kv(), NTW, WR, RING, XMAP, TWO, MTB>>::reg); });
  }
  if (k.nsplit > 1) {
    SMI_REQUIRE(EPI == EPI_RESID && XMAP && RING >= 3 && p.kseg > 0 && k.nsplit <= 16, "launch_pgemm_form: split-K is the RESID ring form's");
    SMI_REQUIRE(L->pslab && (size_t)k.nsplit * p.NT * k.mtiles * 1024 <= L->pslab.bytes(), "launch_pgemm_form: partial slab too small");
    p.slab = L->pslab; p.slab_mt = k.mtiles;
  }
  with_kvf32<EPI>(L, [&](auto kv) {
    hipLaunchKernelGGL((k_pgemm<PRO, EPI, kv(), NTW, WR, RING, XMAP, TWO, MTB>), dim3(k.gx, k.gy), dim3(256), k.lds, st, p);
  });
  SMI_LAUNCH_CHECK();
  if (k.nsplit > 1) {
    DownCP d;
    d.W = nullptr; d.NT = p.NT; d.KT = p.KT; d.M = p.M; d.wperm = 0; d.XS = nullptr; d.part = L->pslab;
    d.Y = p.Y; d.Yin = p.Yin; d.gamma_next = p.gamma_next; d.XSout = p.XSout; d.ssout = p.ssout;
    hipLaunchKernelGGL((k_resid_comb<1, 1>), dim3(k.gx2), dim3(64), 0, st, d, k.nsplit, k.mtiles);
    SMI_LAUNCH_CHECK();
  }
  return SMI_OK;
}
// One greedy row behind the int8 screen: screen, select, the listed tiles -- one chain on the step's stream.  The
// recompute keeps the pick's grid (k_finalize reads the same partial columns); its groups come from the screen's list.
int launch_lm_screened(const smi_llm* L, const GemmP& p, const GemmPick& k, hipStream_t st) {
  SMI_REQUIRE(L->scr_ready && p.M == 1 && p.KT <= 2 * kScrKT && !p.Y, "launch_lm_screened: one greedy row whose logits nobody reads, K <= %d", 64 * kScrKT);
  ScreenP s;
  s.Q8 = (const uint4*)L->scr_q8.get(); s.s8 = L->scr_s8; s.sq8 = L->scr_sq8; s.XS = p.XS;
  s.M = p.M; s.NT = p.NT; s.KT = p.KT; s.KT64 = (p.KT + 1) / 2; s.V = p.V;
  s.ub = L->scr_ub; s.lb = L->scr_lb; s.nlb = L->scr_blocks; s.list = L->scr_list; s.log = L->scr_log;
  if (s.KT64 == 14) hipLaunchKernelGGL((k_lm_screen<14>), dim3(s.nlb), dim3(256), 0, st, s);   // K = 896: every load and MFMA unconditional
  else hipLaunchKernelGGL((k_lm_screen<kScrKT>), dim3(s.nlb), dim3(256), 0, st, s);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lm_select, dim3(1), dim3(1024), 0, st, s);
  SMI_LAUNCH_CHECK();
  GemmP q = p;
  q.tlist = L->scr_list;
  hipLaunchKernelGGL((k_lm<1, 1, 1>), dim3(k.gx), dim3(256), k.lds, st, q, 0, 0);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
// the persistent lm_head: one launch up to 16 rows, else one pass per 32 rows; RT = 2: the screened one-row form
template <int K32, int A, int RT>
int launch_lm_form(const smi_llm* L, const GemmP& p, const GemmPick& k, hipStream_t st) {
  if constexpr (RT == 2) {
    static_assert(!K32 && A == 1, "the screened lm_head is the one-row kernel's");
    return launch_lm_screened(L, p, k, st);
  } else {
    if constexpr (K32) static_cast<void>(LdsBig<k_lm32<A, RT>>::reg);   // 16 rows' operand triples in LDS: 86 KB at K = 896
    for (int i = 0; i < k.launches; ++i) {
      if constexpr (K32) hipLaunchKernelGGL((k_lm32<A, RT>), dim3(k.gx), dim3(256), k.lds, st, p, k.lm_groups, 32 * i);
      else hipLaunchKernelGGL((k_lm<A, RT>), dim3(k.gx), dim3(256 * A), k.lds, st, p, k.lm_groups, 32 * i);
      SMI_LAUNCH_CHECK();
    }
    return SMI_OK;
  }
}
// exact-weights mode: p prepared as for k_gemm, W = fp32 [N][K]
template <int PRO, int EPI>
int launch_x_form(const smi_llm* L, const GemmP& p, const GemmPick& k, hipStream_t st) {
  with_kvf32<EPI>(L, [&](auto kv) { hipLaunchKernelGGL((k_gemm_x<PRO, EPI, kv()>), dim3(k.gx, k.gy), dim3(256), 0, st, p, (const float*)p.W); });
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

// Starts the picked form on the operands p: the pick's derived fields go into p, the form's table row names the kernel.
int launch_form(const smi_llm* L, GemmP p, const GemmPick& k, hipStream_t st) {
  p.work_blocks = k.work_blocks; p.ldsb = k.ldsb; p.lt_shift = k.lt_shift; p.kseg = k.kseg;
  if (k.form < GF_KG_END || (k.form > GF_PG_END && k.form < GF_LM_END)) p.stamps = L->stamps_on ? L->stamps : nullptr;
  if (lm_form_note(k.form))   // (diagnostics) the lm_head's form, grid and block for smi_llm_debug_head
    for (int i = 0; i < k.launches; ++i) SMI_LM_NOTE(L, lm_form_note(k.form), k.gx, k.gy, k.block);
  switch (k.form) {
    case GF_NONE: return SMI_OK;
#define X(id, ...) case GF_##id: return launch_kgemm_form<__VA_ARGS__>(L, p, k, st);
    SMI_KGEMM_FORMS(X)
#undef X
#define X(id, ...) case GF_##id: return launch_down_form<__VA_ARGS__>(L, p, k, st);
    SMI_DOWN_FORMS(X)
#undef X
#define X(id, ...) case GF_##id: return launch_pgemm_form<__VA_ARGS__>(L, p, k, st);
    SMI_PGEMM_FORMS(X)
#undef X
#define X(id, k32, a, rt, note) case GF_##id: return launch_lm_form<k32, a, rt>(L, p, k, st);
    SMI_LM_FORMS(X)
#undef X
#define X(id, ...) case GF_##id: return launch_x_form<__VA_ARGS__>(L, p, k, st);
    SMI_X_FORMS(X)
#undef X
  }
  smi_set_error("launch_form: no kernel form for these rows and switches (form %d)", k.form);   // a missing kernel is an error
  return SMI_EINVAL;
}

// The operands of GEMM kernel `which` (KQKV, KO, KGU, KD, KLM) of `layer` for M rows in workspace w: what follows from the model
// and the workspace alone.  npart: RMSNorm partials per row as the producer of the kernel's operand left them in w.ss.  What
// belongs to one launch path is that caller's: prefetch descriptors, the fused o_proj's fields, Yin, wperm (the bf16 tile order
// of W_down: the exact-weights path reads fp32 [N][K]), kseg / slab, stamps, the restricted lm_head's lists and lm_head's Y.
GemmP gemm_operands(const smi_llm* L, int which, int layer, const Work& w, const RowDesc* rows, int M, int npart) {
  const smi_llm_cfg& c = L->cfg;
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.M = M; p.rows = rows; p.eps = c.rms_eps; p.sspart = w.ss; p.npart = npart;
  switch (which) {
    case KQKV:
      p.W = (const uint4*)sec(L, SMI_LLM_WQKV, layer); p.NT = L->NTqkv; p.KT = L->KTh; p.XS = w.xs_h;
      p.Y = w.q; p.bias = (const float*)sec(L, SMI_LLM_BQKV, layer); p.rope = (const float2*)sec(L, SMI_LLM_ROPE, 0);
      p.kcache = kv_layer(L, L->kcache, layer); p.vcache = kv_layer(L, L->vcache, layer);
      p.q_dim = L->Q; p.kv_dim = L->KV; p.n_kv = c.num_kv_heads; p.max_pos = c.max_positions; p.km = kv_map(L);
      break;
    case KO:   // h += Wo attn; emits the post-attention norm's operand
      p.W = (const uint4*)sec(L, SMI_LLM_WO, layer); p.NT = L->NTh; p.KT = L->KTq; p.XS = w.xs_attn; p.Y = w.h;
      p.XSout = w.xs_h; p.gamma_next = (const float*)sec(L, SMI_LLM_LN2, layer); p.ssout = w.ss;
      break;
    case KGU:
      p.W = (const uint4*)sec(L, SMI_LLM_WGU, layer); p.NT = L->NTgu; p.KT = L->KTh; p.XS = w.xs_h; p.XSout = w.xs_act;
      break;
    case KD:   // h += Wd act; emits the next layer's input-norm operand (or the final norm's)
      p.W = (const uint4*)sec(L, SMI_LLM_WD, layer); p.NT = L->NTh; p.KT = L->KTi; p.XS = w.xs_act; p.Y = w.h;
      p.XSout = w.xs_h; p.ssout = w.ss;
      p.gamma_next = layer + 1 < c.num_layers ? (const float*)sec(L, SMI_LLM_LN1, layer + 1) : (const float*)sec(L, SMI_LLM_FINAL_NORM, 0);
      break;
    case KLM:
      p.W = (const uint4*)sec(L, SMI_LLM_LM_HEAD, 0); p.NT = L->NTlm; p.KT = L->KTh; p.XS = w.xs_h;
      p.V = c.vocab_size; p.pval = L->pval; p.pidx = L->pidx;
      break;
  }
  return p;
}

// The model-derived part of the attention's arguments for M rows in workspace w (the fused o_proj's fields, slot_is_row and the
// prefetch descriptor are the decode caller's).
AttnP attn_operands(const smi_llm* L, int layer, const Work& w, const RowDesc* rows, int M) {
  const smi_llm_cfg& c = L->cfg;
  AttnP a;
  memset(&a, 0, sizeof(a));
  a.q = w.q; a.kcache = kv_layer(L, L->kcache, layer); a.vcache = kv_layer(L, L->vcache, layer);
  a.rows = rows; a.xs_out = w.xs_attn; a.M = M; a.q_dim = L->Q; a.n_kv = c.num_kv_heads;
  a.group = c.num_heads / c.num_kv_heads; a.max_pos = c.max_positions; a.n_heads = c.num_heads; a.km = kv_map(L);
  return a;
}

// The switches the picks read, as the handle holds them, for a kernel of a decode step (pass 0) or of a prompt pass's family.
PickEnv pick_env(const smi_llm* L, int pass) {
  PickEnv e{};
  e.pass = pass; e.stamps = L->stamps_on; e.exact = L->exact; e.tune2 = L->sw.tune2;
  e.pf_mask = L->sw.prefetch_mask; e.pf_rows = L->sw.prefetch_rows;
  e.kv_f32 = L->cfg.kv_dtype ? 1 : 0; e.pg_split_rows = L->sw.pg_split_rows; e.lm_blocks = L->lm_blocks;
  return e;
}
// The pick of GEMM kernel `which` (KQKV, KO, KGU, KD, KLM) over M rows at the handle's shape.
GemmPick pick_gemm(const smi_llm* L, int which, int M, const PickEnv& e) {
  switch (which) {
    case KQKV: return pick_qkv(L->KTh, L->NTqkv, M, e);
    case KO: return pick_o(L->KTq, L->NTh, L->cfg.num_heads, M, e);
    case KGU: return pick_gu(L->KTh, L->NTgu, L->cfg.num_heads, M, e);
    case KD: return pick_d(L->KTi, L->NTh, M, e);
    case KLM: return pick_lm(L->KTh, L->NTlm, M, e);
  }
  return GemmPick{};
}

// One kernel of a decode step over M rows: operands, pick, launch.
int launch_one(smi_llm* L, int which, int layer, const RowDesc* rows, int M, float* logits, hipStream_t st) {
  const smi_llm_cfg& c = L->cfg;
  const bool fused = fuse_o_now(L, rows, M);
  GemmP p = gemm_operands(L, which, layer, L->dec, rows, M, L->NTh * 4);
  if (which == KLM) p.Y = logits ? logits : (logits_needed(L, step_feat(L)) ? L->logits : nullptr);
  PickEnv e = pick_env(L, 0);
  e.fused = fused ? 1 : fuse2_now(L, rows, M) ? 2 : 0;
  if (L->exact && which != KATTN && which != KFIN) {
    // verification mode: same operands, scalars and epilogues, fp32 weights, one exact fp32 FMA chain per output (k_gemm_x)
    SMI_REQUIRE(which != KLM || (L->NTlm + 3) / 4 <= L->lm_cap, "lm_head partial buffer too small");
    return launch_form(L, p, pick_gemm(L, which, M, e), st);
  }
  switch (which) {
    case KQKV:
      // helpers: the first pf_qkv_eighths / 8 of this layer's gate_up slices (consumer block b reads weight tile row b).  Measured
      // at one row, graph step, one box (profiles/r03_prefetch.txt): 8/8 600 us, 6/8 569, 4/8 564, 2/8 559 (default), none 566-571
      p.pf = PfDesc{sec(L, SMI_LLM_WGU, layer), L->KTh * 1024, L->NTgu, 0, ((L->NTgu + 7) / 8 * L->sw.pf_qkv_eighths + 7) / 8};
      e.has_pf = p.pf.base != nullptr;
      return launch_form(L, p, pick_gemm(L, KQKV, M, e), st);
    case KATTN: {
      AttnP a = attn_operands(L, layer, L->dec, rows, M);
      a.slot_is_row = rows == L->rows && L->identity_slots;   // the live decode rows are (slot b, ...) in order (contiguous cache: slots contiguous; paged: through the page table)
      // helpers: second half of this layer's gate_up slices
      a.pf = PfDesc{sec(L, SMI_LLM_WGU, layer), L->KTh * 1024, L->NTgu, (L->NTgu / 8 + 1) / 2, (L->NTgu + 7) / 8};
      if (fused) { a.Wo = (const uint4*)sec(L, SMI_LLM_WO, layer); a.NTo = L->NTh; a.part_o = L->part_o; }
      if (fuse2_now(L, rows, M)) {
        a.Wo = (const uint4*)sec(L, SMI_LLM_WO, layer); a.NTo = L->NTh; a.part_o = L->part_o; a.cnt = L->fuse_cnt;
        a.h = L->dec.h; a.gamma_next = (const float*)sec(L, SMI_LLM_LN2, layer); a.xs_next = L->dec.xs_h; a.ssout = L->dec.ss;
      }
      return c.kv_dtype ? launch_attn<1>(L, a, st) : launch_attn<0>(L, a, st);
    }
    case KO:   // (fused: done by the attention kernel, nothing to launch -- pick_o)
      return launch_form(L, p, pick_gemm(L, KO, M, e), st);
    case KGU:
      if (fused) {
        p.part_o = L->part_o; p.n_oheads = c.num_heads; p.hres = L->dec.h; p.h2out = L->h2;
        if (L->sw.pf_inline && layer + 1 < c.num_layers && L->NTqkv % 8 == 0) {   // SPARKMI_PF_INLINE=0: off (A/B)
          p.pf2_base = sec(L, SMI_LLM_WQKV, layer + 1); p.pf2_slice = L->KTh * 1024; p.pf2_nslices = L->NTqkv;
        }
        p.gam = (const float*)sec(L, SMI_LLM_LN2, layer);
      }
      return launch_form(L, p, pick_gemm(L, KGU, M, e), st);
    case KD:
      p.wperm = L->wd_parts;
      if (fused) p.Yin = L->h2;   // h + o_proj, left there by gate_up's block 0
      // helpers: the next layer's QKV slices (its o_proj slices ride along: same slice size, contiguous-ish)
      if (layer + 1 < c.num_layers) p.pf = PfDesc{sec(L, SMI_LLM_WQKV, layer + 1), L->KTh * 1024, L->NTqkv, 0, (L->NTqkv + 7) / 8};
      e.has_pf = p.pf.base != nullptr;
      return launch_form(L, p, pick_gemm(L, KD, M, e), st);
    case KLM: {
      // every row constrained: only the union's tiles (the groups come from p.tlist, the rows' own ranges through p.ctl)
      e.lm_restricted = L->KTh <= 32 && !logits && rows == L->rows && lm_restricted(L, step_feat(L));
      if (e.lm_restricted) { p.tlist = L->tlist; p.ctl = L->ctl; }
      // one greedy row, nobody reads its logits: the int8 screen lists the tiles that can hold the maximum (same token, same maximum bits)
      e.lm_screen = M == 1 && !logits && !p.Y && rows == L->rows && lm_screened(L, step_feat(L));
      SMI_REQUIRE(L->KTh <= 32 || (L->NTlm + 3) / 4 <= L->lm_cap, "lm_head partial buffer too small");
      return launch_form(L, p, pick_gemm(L, KLM, M, e), st);
    }
    case KFIN: {
      const unsigned feat = step_feat(L);
      FinP f = fin_params(L, M);
      if (feat & F_NGRAM) {   // rows with n = 0 leave at once; the others get -inf at the ids that would repeat an n-gram
        SMI_TRY(launch_ngram_ban(L, M, st));
      }
      // rows neither penalised, biased, n-gram banned nor constrained leave k_penalize at once
      if ((feat & (F_PEN | F_BIAS | F_NGRAM)) || ((feat & F_ALLOW) && logits_needed(L, feat))) {
        SMI_TRY(launch_penalize(L, M, (feat & F_BIAS) ? L->seq : nullptr, st));
        f.phist = L->phist;
      }
      if (feat & F_SAMPLE) {   // rows that do not sample leave both sampler kernels at once
        SMI_TRY(launch_sampler(L, M, true, st));
        f.tok = L->tok;
      }
      if (feat & F_LP) {   // unflagged rows leave k_logprob at once
        SMI_TRY(launch_logprob(L, M, st));
        f.lp = L->lp; f.lp_part = L->lp_part; f.lp_rowc = L->lp_rowc;
      }
      if (feat & F_STOP) f.seq = L->seq;
      return launch_finalize(f, st);
    }
  }
  smi_set_error("launch_one: bad kernel id %d", which);
  return SMI_EINVAL;
}

// RMSNorm partials per row that a layer's QKV finds in the big workspace: [rows][NT * 4] as the row-grouped down_proj leaves them,
// [rows][NT] as the prefill GEMM and its split-K combine do.  The kernel that fills a pass's layer-0 input (k_embed) is told the same.
int pf_nparts_in(const smi_llm* L, int M, int family) {
  const bool gd = L->sw.pg_forced ? M < L->sw.pg_min[3] : family != PF_PGEMM;
  return gd ? L->NTh * 4 : L->NTh;
}

// Layer l of a pass over M (> 32) prompt rows living in the big workspace: its kernels KQKV .. last_kernel (KD: the whole layer;
// the last layer ends after its K/V append whatever last_kernel says -- no prompt row's hidden state feeds lm_head).
// Up to kPgemmMinRows rows the decode GEMM runs with one block row per 32 rows (same bits as 32-row
// chunks, one launch instead of M / 32); beyond, the LDS-shared prefill GEMM (k_pgemm) takes over.
int launch_layer_big(smi_llm* L, int l, const RowDesc* rows, int M, int family, int last_kernel, hipStream_t st) {
  const smi_llm_cfg& c = L->cfg;
  // Which GEMM family: decided by the CALLER from the sequences' own lengths (prefill_prompts), the same for all four kernels of
  // the pass.  Diagnostics (SPARKMI_PGEMM_MIN_* set): per kernel by the pass's row count, as in round 3 -- every mix is
  // parity-tested.  The RESID kernels leave the RMSNorm partials as [rows][NT * 4] (grouped) or [rows][NT] (prefill GEMM and
  // its split-K combine); their consumers are told which.
  const bool pg = family == PF_PGEMM;
  const bool gq = L->sw.pg_forced ? M < L->sw.pg_min[0] : !pg, go = L->sw.pg_forced ? M < L->sw.pg_min[1] : !pg,
             gg = L->sw.pg_forced ? M < L->sw.pg_min[2] : !pg, gd = L->sw.pg_forced ? M < L->sw.pg_min[3] : !pg;
  const int np_from_d = pf_nparts_in(L, M, family), np_from_o = go ? L->NTh * 4 : L->NTh;
  // each kernel: operands, pick (by its family and the row count; the k_pgemm forms and the split-K segments: pick_pgemm_rows), launch
  auto launch = [&](int which, bool grouped, const GemmP& p) {
    return launch_form(L, p, pick_gemm(L, which, M, pick_env(L, grouped ? PF_GROUPED : PF_PGEMM)), st);
  };
  int rc;
  // QKV
  rc = launch(KQKV, gq, gemm_operands(L, KQKV, l, L->big, rows, M, np_from_d));
  if (rc || last_kernel == KQKV || l == c.num_layers - 1) return rc;
  // attention
  const AttnP a = attn_operands(L, l, L->big, rows, M);   // (slot_is_row = 0: prompt rows name their slot)
  const dim3 ag((unsigned)((M + kAttnWaves - 1) / kAttnWaves), (unsigned)c.num_heads);
  if (!c.kv_dtype && L->sw.attn_pf2 && L->pf_ntiles > 0 && c.head_dim == 64) {   // bf16 KV: tiles of 16 rows on the matrix pipes
    const int tasks = L->pf_ntiles * c.num_heads;
    hipLaunchKernelGGL(k_attn_pf2, dim3((tasks + 3) / 4), dim3(256), 0, st, a, (const PfTile*)L->pf_tiles, L->pf_ntiles);
  } else if (c.kv_dtype) hipLaunchKernelGGL((k_attn_pf<1>), ag, dim3(kAttnWaves * 64), 0, st, a);
  else hipLaunchKernelGGL((k_attn_pf<0>), ag, dim3(kAttnWaves * 64), 0, st, a);
  SMI_LAUNCH_CHECK();
  if (last_kernel == KATTN) return SMI_OK;
  // o_proj
  rc = launch(KO, go, gemm_operands(L, KO, l, L->big, rows, M, np_from_d));
  if (rc || last_kernel == KO) return rc;
  // gate_up
  rc = launch(KGU, gg, gemm_operands(L, KGU, l, L->big, rows, M, np_from_o));
  if (rc || last_kernel == KGU) return rc;
  // down
  GemmP d = gemm_operands(L, KD, l, L->big, rows, M, np_from_o);   // (never the last layer's: gamma_next is the next LN1)
  d.wperm = L->wd_parts;
  return launch(KD, gd, d);
}

// All layers for the M prompt rows of one pass: K/V of every row appended, hidden states of the last layer never needed.
int launch_layers_big(smi_llm* L, const RowDesc* rows, int M, int family, hipStream_t st) {
  for (int l = 0; l < L->cfg.num_layers; ++l) {
    const int rc = launch_layer_big(L, l, rows, M, family, KD, st);
    if (rc) return rc;
  }
  return SMI_OK;
}

// A workspace for R rows, allocated in the struct's order and zeroed where `zero` (the decode rows').
int work_alloc(const smi_llm* L, Work& w, size_t R, bool zero) {
  int rc;
  auto a = [&](auto& buf, size_t bytes, const char* what) { return zero ? buf.alloc_zero(bytes, what) : buf.alloc(bytes, what); };
  if ((rc = a(w.h, R * L->H * 4, "workspace h")) || (rc = a(w.q, R * L->Q * 4, "workspace q")) ||
      (rc = a(w.xs_h, R * L->H * 6, "workspace xs_h")) || (rc = a(w.xs_attn, R * L->Q * 6, "workspace xs_attn")) ||
      (rc = a(w.xs_act, R * L->I * 6, "workspace xs_act")) || (rc = a(w.ss, R * L->NTh * 4 * 4, "workspace ss"))) return rc;
  return SMI_OK;
}

// The prefill workspace and its split-K slab grow together: both go, then both come back (the slab first) for `rows` rows.
int ensure_big(smi_llm* L, int rows) {
  if (rows <= L->big_rows) return SMI_OK;
  L->big = Work{};
  L->big_rows = 0;
  L->pslab.reset();
  // split-K partial sums: up to kPgSegD segments x NTh tiles x (min(rows, kPgSplitRows) / 16) m-tiles x 1 KiB
  const size_t mt = ((size_t)(rows < kPgSplitRows ? rows : kPgSplitRows) + 15) / 16;
  int rc;
  if ((rc = L->pslab.alloc((size_t)16 * L->NTh * mt * 1024, "prefill split-K slab")) || (rc = work_alloc(L, L->big, (size_t)rows, false))) return rc;
  L->big_rows = rows;
  return SMI_OK;
}

int launch_embed(smi_llm* L, const RowDesc* rows, int M, hipStream_t st) {
  hipLaunchKernelGGL(k_embed, dim3((M + 3) / 4), dim3(256), 0, st, (const uint16_t*)sec(L, SMI_LLM_LM_HEAD, 0), L->KTh, rows, M,
                     (const float*)sec(L, SMI_LLM_LN1, 0), L->dec.h, L->dec.xs_h, L->dec.ss, L->NTh * 4, L->exact);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

// All layers for M rows.  kv_only_last: skip everything after the last layer's KV append
// (prefill rows whose hidden state is never read).
int launch_layers(smi_llm* L, const RowDesc* rows, int M, bool kv_only_last, hipStream_t st) {
  int rc;
  for (int l = 0; l < L->cfg.num_layers; ++l) {
    if ((rc = launch_one(L, KQKV, l, rows, M, nullptr, st))) return rc;
    if (kv_only_last && l == L->cfg.num_layers - 1) break;
    if ((rc = launch_one(L, KATTN, l, rows, M, nullptr, st))) return rc;
    if ((rc = launch_one(L, KO, l, rows, M, nullptr, st))) return rc;
    if ((rc = launch_one(L, KGU, l, rows, M, nullptr, st))) return rc;
    if ((rc = launch_one(L, KD, l, rows, M, nullptr, st))) return rc;
  }
  return SMI_OK;
}

int launch_step(smi_llm* L, int M, hipStream_t st) {
  int rc;
  if (eng_usable(L, L->rows, M)) {   // one live row: all layers in one persistent launch (smi_eng.h), same bits
    if ((rc = eng_launch(L, st))) return rc;
  } else if ((rc = launch_layers(L, L->rows, M, false, st))) return rc;
  if ((rc = launch_one(L, KLM, 0, L->rows, M, nullptr, st))) return rc;
  return launch_one(L, KFIN, 0, L->rows, M, nullptr, st);
}

int ensure_plan(smi_llm* L, size_t rows) {
  if (rows * sizeof(RowDesc) <= L->plan.bytes()) return SMI_OK;
  return L->plan.ensure((rows + 1024) * sizeof(RowDesc), "prefill plan");
}

// smi_llm_poll's gather: one block per listed slot.  Word 0 of the slot's staging record holds {count, finished}, words 1 .. cap the
// history entries from[i] .. (the lanes run over t; the history is [t][kMaxRows], so a slot's ids are kMaxRows words apart).
// Entries past the sequence's count are left as they are: the host reads none of them.
struct PollArgs {
  int32_t slot[kMaxRows];
  int32_t from[kMaxRows];
};
__global__ __launch_bounds__(64) void k_poll(const int64_t* hist, const int32_t* count, const int32_t* finished, int max_steps,
                                             PollArgs a, int cap, int64_t* stage) {
  const int i = blockIdx.x, sl = a.slot[i], from = a.from[i];
  int64_t* rec = stage + (size_t)i * (1 + cap);
  const int cnt = count[sl];
  if (threadIdx.x == 0) {
    int2 head; head.x = cnt; head.y = finished[sl];
    *(int2*)rec = head;
  }
  int end = cnt < max_steps ? cnt : max_steps;           // (the history holds max_steps entries per slot)
  if (end - from > cap) end = from + cap;                 // (from <= max_steps here or the loop is empty: no overflow)
  for (int t = from + (int)threadIdx.x; t < end; t += 64) rec[1 + (t - from)] = hist[(size_t)t * kMaxRows + sl];
}

// ------------------------------------------------------------------------------------------
// Park and resume (smi_llm_slots_save / smi_llm_slots_restore; include/sparkmi.h states the contract).  A sequence's snapshot
// ("blob") is one contiguous piece of caller-owned device memory:
//   BlobHdr                      host-written fields (lengths, stamps, the records as admitted), and 32 bytes the gather kernel
//                                writes: the row descriptor (slot field zero), count, finished
//   SeqRec                       only with bias entries / stop sequences
//   K/V   [layer][K, V][kv head][position 0 .. npos)[row bytes]   npos = cache positions written = len - 1
//   hist  [nhist] int64          the sequence's column of the history, dense (nhist = len - plen = its token index)
//   lp    [nhist] f32            only with return_log_probs
//   phist [vocab] u16            only with a penalty record
//   pctx  [plen] int32           only with no_repeat_ngram_size
// every part starts on a 16-byte boundary (the tail of a part is padding, written as zero by the save and never read).
// Nothing in a blob names the slot it came from.
// ------------------------------------------------------------------------------------------
struct BlobHdr {
  char magic[8];                  // "SMISLOT1"
  uint32_t hdr_bytes;             // sizeof(BlobHdr) (+ sizeof(SeqRec)): where the K/V part starts
  uint32_t feat;                  // the slot's feature byte (smi_llm::slot_feat)
  uint64_t total_bytes;
  uint64_t cfg_stamp;             // FNV-1a of the handle's smi_llm_cfg
  uint64_t handle_id, session_gen;   // which handle, which smi_llm_session_begin of it
  int32_t len, plen, nhist, seqid;   // slot_len, prompt length, history entries, admission number
  uint64_t reserved;              // 0
  uint64_t check;                 // FNV-1a of the host-written bytes of the header (this field and `dev` as zero), SeqRec included
  struct Dev { RowDesc row; int32_t count, finished, pad[2]; } dev;   // written by k_slot_cols<true>
  SampRec samp; PenRec pen; int32_t lp, ngram, ngplen, pad; AllowRec allow;
};
static_assert(sizeof(BlobHdr) % 16 == 0 && sizeof(SeqRec) % 16 == 0 && offsetof(BlobHdr, dev) % 16 == 0, "blob parts are 16-byte aligned");

// One listed slot of a save / restore call.  Offsets are in 16-byte units from the blob's start; 0 = the sequence has no such part.
struct SlotXfer {
  unsigned char* blob;
  int32_t slot, npos, nhist, npctx;
  uint32_t o_kv, o_hist, o_lp, o_phist, o_pctx, pad;
};
struct ParkP {
  SlotXfer s[kMaxRows];
  unsigned char* kcache;      // layer 0's K cache (layer l at + l * layer_bytes)
  unsigned char* vcache;
  size_t layer_bytes;
  int n_kv, max_pos;
  int piece_shift;            // log2(16-byte pieces per 64-element row): 3 (bf16) or 4 (f32)
  KvMap km;
  RowDesc* rows; int B;       // the live row list (save: the slot's row goes into the blob)
  int64_t* hist; float* lp; uint16_t* phist; int32_t* pctx;
  int32_t *count, *finished;
  int V;
};
constexpr int kParkPieces = 4;   // 16-byte pieces per thread of k_slot_kv, all loads before the stores

// The K/V part: cache positions [0, npos) of each listed slot <-> its blob, every layer, K and V, every kv head, in 16-byte
// pieces, the cache side addressed through KvMap as k_kv_fork does (bf16 / f32, contiguous / paged: the same code); the blob side
// is dense, so consecutive lanes touch consecutive pieces on both sides (a cache row is 128 or 256 contiguous bytes).
// grid: x = blocks of 256 * kParkPieces (position, piece) pairs of the call's longest slot, y = listed slot,
// z = (layer, K / V, kv head).  A block past its own slot's last piece exits at once.
template <bool SAVE>
__global__ __launch_bounds__(256) void k_slot_kv(ParkP p) {
  const SlotXfer& x = p.s[blockIdx.y];
  const int total = x.npos << p.piece_shift;   // pieces of one (layer, K / V, kv head) plane
  const int u0 = (int)blockIdx.x * (256 * kParkPieces) + (int)threadIdx.x;
  if ((int)blockIdx.x * (256 * kParkPieces) >= total) return;
  const int kvh = (int)blockIdx.z % p.n_kv, isv = ((int)blockIdx.z / p.n_kv) & 1, layer = (int)blockIdx.z / (2 * p.n_kv);
  unsigned char* base = (isv ? p.vcache : p.kcache) + (size_t)layer * p.layer_bytes;
  const size_t rb = (size_t)16 << p.piece_shift;   // bytes of one row
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (a native vector: c[] and v[] below stay in registers)
  u32x4* plane = (u32x4*)x.blob + (size_t)x.o_kv + (size_t)blockIdx.z * (size_t)total;
  // Every thread forms all its addresses and issues all its loads before its first store.  A piece past the plane's end is
  // clamped to the last one (total >= 1 here), so the loads are unconditional; only the stores are predicated.
  u32x4* c[kParkPieces];
  u32x4 v[kParkPieces];
#pragma unroll
  for (int k = 0; k < kParkPieces; ++k) {
    const int u = min(u0 + 256 * k, total - 1);
    const int pos = u >> p.piece_shift, piece = u & ((1 << p.piece_shift) - 1);
    c[k] = (u32x4*)(base + kv_row(p.km, x.slot, kvh, p.n_kv, p.max_pos, pos) * rb) + piece;
    v[k] = SAVE ? *c[k] : plane[u];
  }
#pragma unroll
  for (int k = 0; k < kParkPieces; ++k) {
    if (u0 + 256 * k >= total) continue;
    if (SAVE) plane[u0 + 256 * k] = v[k];
    else *c[k] = v[k];
  }
}

// The rest of a sequence's device state: its column of hist (and of lp), strided by kMaxRows on the engine side and dense in
// the blob; its row of phist; its row of pctx up to the prompt length; count / finished and (save) its row descriptor.  Only
// the parts the SlotXfer names.  grid: x = a few blocks that stride over each part, y = listed slot.
template <bool SAVE>
__global__ __launch_bounds__(256) void k_slot_cols(ParkP p) {
  const SlotXfer& x = p.s[blockIdx.y];
  const int sl = x.slot;
  const int t0 = (int)(blockIdx.x * 256 + threadIdx.x), T = (int)gridDim.x * 256;
  uint4* b16 = (uint4*)x.blob;
  {
    int64_t* bh = (int64_t*)(b16 + x.o_hist);
    for (int t = t0; t < (SAVE ? (x.nhist + 1) & ~1 : x.nhist); t += T) {   // (save: the part's padding is written as zero)
      if (SAVE) bh[t] = t < x.nhist ? p.hist[(size_t)t * kMaxRows + sl] : 0;
      else p.hist[(size_t)t * kMaxRows + sl] = bh[t];
    }
  }
  if (x.o_lp) {
    float* bl = (float*)(b16 + x.o_lp);
    for (int t = t0; t < (SAVE ? (x.nhist + 3) & ~3 : x.nhist); t += T) {
      if (SAVE) bl[t] = t < x.nhist ? p.lp[(size_t)t * kMaxRows + sl] : 0.f;
      else p.lp[(size_t)t * kMaxRows + sl] = bl[t];
    }
  }
  if (x.o_phist) {
    uint16_t* row = p.phist + (size_t)sl * p.V;
    if ((p.V & 7) == 0) {   // every slot's row starts on a 16-byte boundary
      uint4 *r4 = (uint4*)row, *bp = b16 + x.o_phist;
      for (int t = t0; t < (p.V >> 3); t += T) {
        if (SAVE) bp[t] = r4[t];
        else r4[t] = bp[t];
      }
    } else {
      uint16_t* bp = (uint16_t*)(b16 + x.o_phist);
      for (int t = t0; t < (SAVE ? (p.V + 7) & ~7 : p.V); t += T) {
        if (SAVE) bp[t] = t < p.V ? row[t] : (uint16_t)0;
        else row[t] = bp[t];
      }
    }
  }
  if (x.o_pctx) {
    int32_t *row = p.pctx + (size_t)sl * p.max_pos, *bp = (int32_t*)(b16 + x.o_pctx);
    for (int t = t0; t < (SAVE ? (x.npctx + 3) & ~3 : x.npctx); t += T) {
      if (SAVE) bp[t] = t < x.npctx ? row[t] : 0;
      else row[t] = bp[t];
    }
  }
  if (blockIdx.x == 0) {
    BlobHdr::Dev* d = (BlobHdr::Dev*)(x.blob + offsetof(BlobHdr, dev));
    if (SAVE) {
      if ((int)threadIdx.x < p.B && p.rows[threadIdx.x].slot == sl) {   // exactly one live row names a busy slot
        const RowDesc* r = p.rows + threadIdx.x;
        d->row.slot = 0; d->row.pos = r->pos; d->row.token = r->token; d->row.flags = r->flags;
        d->count = p.count[sl]; d->finished = p.finished[sl]; d->pad[0] = 0; d->pad[1] = 0;
      }
    } else if (threadIdx.x == 0) {   // (the host puts the row into the live row list)
      p.count[sl] = d->count;
      p.finished[sl] = d->finished;
    }
  }
}

// The diagnostics switches, in the order of DESIGN 6.1, each with what was measured for its default.
Switches read_switches() {
  Switches w;
  // helper-block prefetch per producer: bit 0 QKV (gate_up's first half), bit 1 attention (second half), bit 2 down_proj (the next
  // layer's QKV / o_proj); SPARKMI_PREFETCH=<mask> picks, SPARKMI_NO_PREFETCH=1 is mask 0
  // Default since k_down1 (round 3): QKV's helpers at ONE row only.  Measured on one box, alternating processes, graph step at one
  // row: mask 0 566-571 us, 1 563-564, 2 581, 3 583, 4 597, 5 602, 6 658, 7 665 (down_proj's 256-thread blocks make slow helpers);
  // at 4 rows mask 0 727 us, 3 748, 7 739-745 (profiles/r03_prefetch.txt).  SPARKMI_PREFETCH=<mask> applies up to 8 rows as before.
  w.prefetch_mask = 1; w.prefetch_rows = 1;
  if (const char* e = smi_env("SPARKMI_PREFETCH")) { w.prefetch_mask = atoi(e) & 7; w.prefetch_rows = 8; }
  { const char* e = smi_env("SPARKMI_PF_QKV"); w.pf_qkv_eighths = e ? atoi(e) : 2; if (w.pf_qkv_eighths < 0 || w.pf_qkv_eighths > 8) w.pf_qkv_eighths = 2; }
  if (smi_env("SPARKMI_NO_PREFETCH")) w.prefetch_mask = 0;
  { const char* e = smi_env("SPARKMI_PF_INLINE"); w.pf_inline = !(e && e[0] == '0'); }
  { const char* e = smi_env("SPARKMI_TUNE2"); w.tune2 = e ? atoi(e) : 0; }
  // OFF by default (diagnostics build: SPARKMI_FUSE2_ROWS=n enables it up to n <= 8 rows).  Measured at 0.5B, graph step, one box
  // (profiles/r04_fused_oproj_last_arriver.txt): 8 rows 730 -> 863 us (attention 3.9 -> 14.1 us for the 4.3-us o_proj launch it
  // replaces), 2 rows 616 -> 640, one row (a retired switch, against the per-head partials every gate_up block sums) 543 -> 581:
  // the arrival count + the reads of write-through partials cost 3-4 us at one row, where a kernel boundary costs 1.8.
  { const char* e = smi_env("SPARKMI_FUSE2_ROWS"); w.fuse2_rows = e ? atoi(e) : 0; if (w.fuse2_rows > kFuse2Max) w.fuse2_rows = kFuse2Max; }
  { const char* e = smi_env("SPARKMI_PG_SPLIT_ROWS"); w.pg_split_rows = e ? atoi(e) : kPgSplitRows; if (w.pg_split_rows > kPgSplitRows) w.pg_split_rows = kPgSplitRows; }
  {
    const char* names[4] = {"SPARKMI_PGEMM_MIN_QKV", "SPARKMI_PGEMM_MIN_O", "SPARKMI_PGEMM_MIN_GU", "SPARKMI_PGEMM_MIN_D"};
    // measured crossovers (tools/prefill_time.py mix / mix2, profiles/README.md): gate_up from ~300 rows (its grouped form re-reads
    // the operand triples once per 32 columns), down_proj from ~900, the two short-K GEMMs from ~1300
    const int dflt[4] = {1280, 1280, 288, 896};
    const char* common = smi_env("SPARKMI_PGEMM_MIN_ROWS");   // all four kernels alike; a kernel's own switch overrides it
    w.pg_forced = common != nullptr;
    for (int i = 0; i < 4; ++i) { const char* e = smi_env(names[i]); w.pg_forced |= e != nullptr; w.pg_min[i] = e ? atoi(e) : common ? atoi(common) : dflt[i]; }
  }
  { const char* e = smi_env("SPARKMI_ATTN_PF2"); w.attn_pf2 = !(e && e[0] == '0'); }
  w.no_fuse_o = smi_env("SPARKMI_NO_FUSE_O") != nullptr;
  // the int8 screen of the one-row greedy lm_head: on from kLmScreenMinBytes of lm_head section (the 0.5B shape); SPARKMI_LM_SCREEN=1
  // forces it on at any size (the tests' tiny shapes), =0 off (A/B at the 0.5B shape)
  { const char* e = smi_env("SPARKMI_LM_SCREEN"); w.lm_screen = e ? (e[0] != '0' ? 1 : 0) : -1; }
  return w;
}

// lm_head sections from this size take the int8 screen at one greedy row.  Fixed just under the 0.5B shape's 297.5 MB (166 000 x
// 896 bf16), the one size it was measured at: the screen trades 149 MB of the stream for two more launches, which a small
// vocabulary does not pay back.
constexpr size_t kLmScreenMinBytes = (size_t)256 << 20;
bool lm_screen_fits(const smi_llm* L) { return !L->exact && L->KTh <= 32; }
// The int8 copy of the lm_head section and the screen's buffers: once per handle, outside any capture (smi_llm_create; the
// diagnostics hook of a handle that was created without).  Synchronises.
int lm_screen_build(smi_llm* L) {
  if (L->scr_ready) return SMI_OK;
  SMI_REQUIRE(lm_screen_fits(L), "lm_screen_build: bf16 weights and at most 32 k tiles");
  const size_t NT = (size_t)L->NTlm, KT64 = (size_t)(L->KTh + 1) / 2;
  L->scr_blocks = L->lm_blocks;
  int rc;
  if ((rc = L->scr_q8.alloc_zero(NT * KT64 * 1024, "lm_head int8 copy")) || (rc = L->scr_s8.alloc(NT * 16 * 4, "lm_head int8 scales")) ||
      (rc = L->scr_sq8.alloc(NT * 16 * 4, "lm_head int8 row sums")) || (rc = L->scr_ub.alloc(NT * 4, "screen upper bounds")) ||
      (rc = L->scr_lb.alloc((size_t)L->scr_blocks * 4, "screen lower bounds")) || (rc = L->scr_list.alloc_zero((NT + 1) * 4, "screen list")))
    return rc;
#ifdef SMI_DIAG
  if ((rc = L->scr_log.alloc_zero((size_t)4097 * 4, "screen log"))) return rc;
#endif
  hipLaunchKernelGGL(k_lm_pack8, dim3((unsigned)NT), dim3(256), 0, 0, (const uint16_t*)sec(L, SMI_LLM_LM_HEAD, 0), L->KTh, (int)KT64, L->cfg.vocab_size,
                     (unsigned char*)L->scr_q8, (float*)L->scr_s8, (float*)L->scr_sq8);
  SMI_LAUNCH_CHECK();
  SMI_HIP(hipDeviceSynchronize());
  L->scr_ready = 1;
  return SMI_OK;
}

}  // namespace

extern "C" {

size_t smi_llm_arena_bytes(const smi_llm_cfg* cfg) {
  if (!cfg_ok(cfg)) return 0;
  return make_layout(cfg).total;
}

int smi_llm_arena_section(const smi_llm_cfg* cfg, int section, int layer, size_t* offset, size_t* bytes) {
  SMI_REQUIRE(cfg_ok(cfg), "smi_llm_arena_section: invalid config");
  SMI_REQUIRE(section >= 0 && section < SMI_LLM_NUM_SECTIONS, "bad section %d", section);
  Layout L = make_layout(cfg);
  if (section >= SMI_LLM_FINAL_NORM) {
    SMI_REQUIRE(layer == 0, "global section takes layer 0");
    if (offset) *offset = L.off[section];
  } else {
    SMI_REQUIRE(layer >= 0 && layer < cfg->num_layers, "bad layer %d", layer);
    if (offset) *offset = L.layers_base + (size_t)layer * L.layer_stride + L.off[section];
  }
  if (bytes) *bytes = L.bytes[section];
  return SMI_OK;
}

int smi_llm_create(const smi_llm_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_llm** out) {
  SMI_REQUIRE(out, "smi_llm_create: out is null");
  *out = nullptr;
  SMI_REQUIRE(cfg_ok(cfg), "smi_llm_create: config outside the kernel contract (head_dim 64, hidden/intermediate %% 32, slots<=32)");
  Layout lay = make_layout(cfg);
  SMI_REQUIRE(arena_dev && arena_bytes >= lay.total, "smi_llm_create: arena too small (%zu < %zu)", arena_bytes, lay.total);
  SMI_REQUIRE(((uintptr_t)arena_dev & 255) == 0, "smi_llm_create: arena must be 256-byte aligned");
  {   // the arena says how it was packed (include/sparkmi.h: smi_llm_arena_tag); a mismatch with the config is an error, not wrong logits
    static_assert(sizeof(smi_llm_arena_tag) == 256, "arena tag is one 256-byte section");
    smi_llm_arena_tag tag;
    SMI_HIP(hipMemcpy(&tag, (const unsigned char*)arena_dev + lay.off[SMI_LLM_TAG], sizeof(tag), hipMemcpyDeviceToHost));
    SMI_REQUIRE(memcmp(tag.magic, "SMIARENA", 8) == 0, "smi_llm_create: the arena carries no layout tag (section SMI_LLM_TAG): not packed for this library, or for other dimensions");
    SMI_REQUIRE(tag.abi_version == SMI_ABI_VERSION, "smi_llm_create: arena packed for ABI %d, this library is ABI %d", tag.abi_version, SMI_ABI_VERSION);
    SMI_REQUIRE(tag.weights_exact == cfg->weights_exact, "smi_llm_create: the arena holds %s matrices, the config asks for %s (smi_llm_cfg.weights_exact)",
                tag.weights_exact ? "fp32 (exact-weights)" : "bf16-tiled", cfg->weights_exact ? "fp32" : "bf16 tiles");
    SMI_REQUIRE(tag.wd_plain == cfg->wd_plain, "smi_llm_create: the arena's W_down tiles are packed %s, the config says %s (smi_llm_cfg.wd_plain)",
                tag.wd_plain ? "in the plain tile order" : "row-part-major", cfg->wd_plain ? "plain" : "row-part-major");
    SMI_REQUIRE(tag.vocab_size == cfg->vocab_size && tag.hidden_size == cfg->hidden_size && tag.num_layers == cfg->num_layers &&
                tag.num_heads == cfg->num_heads && tag.num_kv_heads == cfg->num_kv_heads && tag.intermediate_size == cfg->intermediate_size &&
                tag.max_positions == cfg->max_positions, "smi_llm_create: the arena was packed for other dimensions than this config");
  }
  // shapes
  smi_llm* L = new smi_llm();   // value-initialised: every field is zero / empty but those whose declaration names a default
  L->cfg = *cfg; L->lay = lay; L->arena = (const unsigned char*)arena_dev;
  L->H = cfg->hidden_size; L->Q = cfg->num_heads * cfg->head_dim; L->KV = cfg->num_kv_heads * cfg->head_dim;
  L->I = cfg->intermediate_size;
  L->KTh = L->H / 32; L->KTq = L->Q / 32; L->KTi = L->I / 32;
  L->NTqkv = (L->Q + 2 * L->KV) / 16; L->NTh = L->H / 16; L->NTgu = 2 * L->I / 16; L->NTlm = lay.vpad / 16;
  L->lm_cap = (L->NTlm + 3) / 4;                       // partial-argmax slots (two-m-tile path: one per block)
  L->lm_blocks = L->lm_cap < 512 ? L->lm_cap : 512;    // persistent path: 2 resident blocks per CU
  L->max_steps = cfg->max_positions;
  L->wd_parts = cfg->wd_plain ? 0 : 1;   // the arena's W_down tile order comes with its config (never from the environment)
  L->exact = cfg->weights_exact;
  L->hseq.assign(kMaxRows, SeqRec{});
  { static std::atomic<uint64_t> handles{0}; L->handle_id = ++handles; }
  const size_t esz = cfg->kv_dtype ? 4 : 2;
  L->paged = cfg->kv_page_tokens > 0;
  L->kv_layer_elems = (size_t)cfg->max_slots * cfg->num_kv_heads * cfg->max_positions * kHeadDim;
  if (L->paged) {
    while ((1 << L->pshift) < cfg->kv_page_tokens) ++L->pshift;
    L->ppslot = cfg->max_positions >> L->pshift;
    L->kv_layer_elems = (size_t)cfg->kv_pages * cfg->num_kv_heads * cfg->kv_page_tokens * kHeadDim;
    L->hptab.assign((size_t)cfg->max_slots * L->ppslot, 0);
    for (int pg = cfg->kv_pages - 1; pg >= 0; --pg) L->free_pages.push_back(pg);
    L->page_ref.assign((size_t)cfg->kv_pages, 0);
  }
  const size_t kvbytes = L->kv_layer_elems * esz * cfg->num_layers;
  // switches
  L->sw = read_switches();
  // the fused o_proj reads bf16 tiles; the one-row fused kernel has 32-bit K / V piece offsets
  L->fuse_o = !L->sw.no_fuse_o && fuse_o_fits(cfg->num_heads, L->NTh, L->KTh) && !L->exact && cfg->max_positions <= kFuseMaxPos;
  // device memory, in this order: a buffer's address depends on what was allocated before it, so a new buffer goes to the end
  // of the list and the earlier ones keep the placement they had without it (a: as allocated, z: zeroed)
  int rc = work_alloc(L, L->dec, kMaxRows, true);
  auto a = [&](auto& buf, size_t bytes, const char* what) { if (!rc) rc = buf.alloc(bytes, what); };
  auto z = [&](auto& buf, size_t bytes, const char* what) { if (!rc) rc = buf.alloc_zero(bytes, what); };
  a(L->part_o, (size_t)kFuse2Max * kMaxOHeads * L->H * 4, "part_o");
  z(L->fuse_cnt, (size_t)kFuse2Max * kFuseQB * 4, "fuse_cnt");
  a(L->h2, (size_t)L->H * 4, "h2");
  a(L->dpart, (size_t)16 * L->NTh * 4 * 64 * 16, "dpart");
  z(L->rows, kMaxRows * sizeof(RowDesc), "rows");
  a(L->pval, (size_t)L->lm_cap * kMaxRows * 4, "pval");
  a(L->pidx, (size_t)L->lm_cap * kMaxRows * 4, "pidx");
  a(L->hist, (size_t)L->max_steps * kMaxRows * 8, "hist");
  z(L->count, kMaxRows * 4, "count");
  z(L->finished, kMaxRows * 4, "finished");
  z(L->step, 4, "step");
  z(L->ctl, sizeof(Ctl), "ctl");
  if (L->paged) z(L->ptab, L->hptab.size() * 4, "ptab");
  a(L->logits, (size_t)kMaxRows * cfg->vocab_size * 4, "logits");
  a(L->phist, (size_t)cfg->max_slots * cfg->vocab_size * 2, "phist");   // (a penalised admission zeroes its slot's row)
  a(L->tok, kMaxRows * 4, "tok");
  a(L->cand_v, (size_t)kMaxRows * kCandCap * 4, "cand_v");
  a(L->cand_i, (size_t)kMaxRows * kCandCap * 4, "cand_i");
  z(L->cand_n, kMaxRows * 4, "cand_n");
  a(L->stamps, (size_t)4096 * 8 * 8, "stamps");
  z(L->kcache, kvbytes, "kcache");
  z(L->vcache, kvbytes, "vcache");
  // log-probabilities (smi_llm_admit_logprobs)
  a(L->lp, (size_t)L->max_steps * kMaxRows * 4, "lp");
  a(L->lp_part, (size_t)kMaxRows * kLpBlocks * 4, "lp_part");
  a(L->lp_rowc, (size_t)kMaxRows * sizeof(float2), "lp_rowc");
  // the restricted lm_head's tile list (smi_llm_admit_constrained): {count, tiles}; zeros = no tile, entry 0 a valid tile index
  z(L->tlist, ((size_t)L->NTlm + 1) * 4, "tlist");
  // per-slot bias / stop records (smi_llm_admit_biased): all zero = none
  z(L->seq, (size_t)kMaxRows * sizeof(SeqRec), "seq");
  // the n-gram ban's prompt ids per slot (smi_llm_admit_ngram): a row is written by the admission that reads it
  z(L->pctx, (size_t)cfg->max_slots * cfg->max_positions * 4, "pctx");
  // smi_llm_poll's staging: {count, finished, ids[cap]} per listed slot, cap <= max_steps, and its pinned host copy
  a(L->poll_dev, (size_t)kMaxRows * (1 + (size_t)L->max_steps) * 8, "poll_dev");
  a(L->poll_host, (size_t)kMaxRows * (1 + (size_t)L->max_steps) * 8, "poll_host");
  // the large LDS window of every LdsBig kernel, once per device and outside any stream capture
  if (!rc) rc = lds_big_opt_in();
  // the one-row greedy lm_head's int8 screen: the weights do not change, so the copy is built here, once, where steps will take it
  L->scr_on = lm_screen_fits(L) && (L->sw.lm_screen == 1 || (L->sw.lm_screen < 0 && lay.bytes[SMI_LLM_LM_HEAD] >= kLmScreenMinBytes));
  if (!rc && L->scr_on) rc = lm_screen_build(L);
  if (!rc && (hipEventCreate(&L->ev0) != hipSuccess || hipEventCreate(&L->ev1) != hipSuccess)) {
    smi_set_error("hipEventCreate failed");
    rc = SMI_EHIP;
  }
  // The one-row decode engine is opt-in (SPARKMI_ENGINE=1, or smi_llm_set_engine later: it is built on first request --
  // 0.8 GB of re-packed weights): measured on MI355X at the 0.5B shape a layer takes 26.3 us in the engine against 23.4 us
  // as four launches -- five in-launch hand-offs of 2.5-4.5 us cost more than the four kernel boundaries they replace
  // (profiles/r03_engine_ab.txt).
#ifdef SMI_DIAG
  snprintf(L->eng.why, sizeof(L->eng.why), "off (opt-in: SPARKMI_ENGINE=1 or smi_llm_set_engine)");
  { const char* e = smi_env("SPARKMI_ENGINE");
    if (!rc && e && e[0] == '1' && !(rc = eng_create(L))) L->eng_on = L->eng.enabled;
  }
#endif
  if (rc) {
    smi_llm_destroy(L);
    return rc;
  }
  *out = L;
  return SMI_OK;
}

int smi_llm_destroy(smi_llm* L) {
  if (!L) return SMI_OK;
  graphs_flush(L);
  if (L->ev0) (void)hipEventDestroy(L->ev0);
  if (L->ev1) (void)hipEventDestroy(L->ev1);
  delete L;   // every device buffer goes with its owner
  return SMI_OK;
}

int smi_llm_set_sampling(smi_llm* L, int do_sample, float temperature, int top_k, float top_p, uint64_t seed) {
  SMI_REQUIRE(L, "smi_llm_set_sampling: null handle");
  if (do_sample) {
    SMI_REQUIRE(temperature > 0.f, "smi_llm_set_sampling: temperature must be > 0");
    SMI_REQUIRE(top_k >= 1 && top_k <= kSampleCap, "smi_llm_set_sampling: top_k must be in 1..%d", kSampleCap);
    SMI_REQUIRE(top_p > 0.f && top_p <= 1.f, "smi_llm_set_sampling: top_p must be in (0, 1]");
    if (top_k > L->cfg.vocab_size) top_k = L->cfg.vocab_size;
  }
  // mode, temperature, top-k and top-p are kernel parameters of the captured step; the seed lives in device memory (Ctl)
  const bool changed = L->do_sample != (do_sample ? 1 : 0) ||
                       (do_sample && (L->temperature != temperature || L->top_k != top_k || L->top_p != top_p));
  L->do_sample = do_sample ? 1 : 0;
  L->temperature = temperature; L->top_k = top_k; L->top_p = top_p; L->seed = seed;
  L->hctl.seed = seed;   // uploaded with the next prefill / session_begin too
  SMI_HIP(hipMemcpy(&L->ctl->seed, &seed, sizeof(seed), hipMemcpyHostToDevice));
  if (changed) graphs_flush(L);
  return SMI_OK;
}

// Prefill attention tiles of a row group (k_attn_pf2): runs of up to 16 rows that are consecutive tokens of one KV slot.  Host only.
static void pf_tiles_build(const RowDesc* rows, int M, std::vector<PfTile>& T) {
  T.clear();
  for (int i = 0; i < M;) {
    const RowDesc& a0 = rows[i];
    int n = 1;
    while (n < 16 && i + n < M && rows[i + n].slot == a0.slot && rows[i + n].pos == a0.pos + n) ++n;
    T.push_back(PfTile{i, n, a0.slot, a0.pos});
    i += n;
  }
}

// The tiles of the row group in flight (host_rows: its M rows on the host), built and sent to L->pf_tiles where the cache type and
// the handle's settings take k_attn_pf2; L->pf_ntiles = 0 otherwise.
static int pf_tiles_upload(smi_llm* L, const RowDesc* host_rows, int M, hipStream_t st) {
  L->pf_ntiles = 0;
  if (L->cfg.kv_dtype || !L->sw.attn_pf2) return SMI_OK;
  std::vector<PfTile>& T = L->host_tiles;
  pf_tiles_build(host_rows, M, T);
  if (T.size() * sizeof(PfTile) > L->pf_tiles.bytes())
    if (int rc = L->pf_tiles.ensure((T.size() + 256) * sizeof(PfTile), "prefill attention tiles")) return rc;
  // (pageable source: staged before the call returns; host_tiles is rebuilt only by the next group, behind this copy)
  SMI_HIP(hipMemcpyAsync(L->pf_tiles, T.data(), T.size() * sizeof(PfTile), hipMemcpyHostToDevice, st));
  L->pf_ntiles = (int)T.size();
  return SMI_OK;
}

// Runs every prompt token but each sequence's last through the layers (K/V appended at slots[b]) and leaves the n
// "last prompt token" rows at L->plan + *tail_off (device) and in L->host_rows (host) for the first step.
// Argument checks of a prefill / admission, made BEFORE anything of the handle's state (KV pages, sequence numbers, the
// `started` flag) is touched: a call that fails here changes nothing.
static int validate_prompts(const smi_llm* L, const int64_t* ids, const int32_t* lens, int B, int P_max) {
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(lens[b] >= 1 && lens[b] <= P_max, "smi_llm_prefill: lens[%d]=%d outside 1..%d", b, lens[b], P_max);
    SMI_REQUIRE(lens[b] < L->cfg.max_positions, "smi_llm_prefill: prompt %d longer than max_positions", b);
    for (int t = 0; t < lens[b]; ++t) {
      const int64_t id = ids[(size_t)b * P_max + t];
      SMI_REQUIRE(id >= 0 && id < L->cfg.vocab_size, "smi_llm_prefill: token id %lld out of range", (long long)id);
    }
  }
  return SMI_OK;
}

// Forked admission: n_ret[b] takes of prompt b (null: one each) -- the prompt rows run once, in slots[b], and the tail holds one
// row per take, in tail_slots (prompt-major).  `extra` rows (the fork copy's work list) go up with the plan, at *tail_off + kMaxRows.
static int prefill_prompts(smi_llm* L, const int64_t* ids, const int32_t* lens, int B, int P_max, const int32_t* slots,
                           size_t* tail_off, hipStream_t st, const int32_t* n_ret = nullptr, const int32_t* tail_slots = nullptr,
                           const std::vector<RowDesc>* extra = nullptr) {
  size_t total = 0;
  { const int rcv = validate_prompts(L, ids, lens, B, P_max); if (rcv) return rcv; }
  for (int b = 0; b < B; ++b) total += lens[b] - 1;
  {
    int longest = 0;
    for (int b = 0; b < B; ++b) longest = lens[b] > longest ? lens[b] : longest;
    L->attn_seg = segs_for(longest);
  }
  // Every prompt token but each sequence's last is a row (slot, pos, token); the B last tokens run as the first regular step
  // (lm_head + argmax).  WHICH kernels a sequence's prompt rows run through is decided by ITS OWN row count alone:
  //   class 0  up to kMaxRows rows        the decode kernels, kMaxRows-row chunks (rows are independent there: any chunking, same bits)
  //   class 1  kMaxRows + 1 .. kPfLong-1  row-grouped decode GEMMs + the prefill attention (empty: kPfLong = kMaxRows + 1)
  //   class 2  kPfLong rows and more      the prefill GEMM family (k_pgemm, segmented o_proj / down_proj sums) + the prefill attention
  // and every class is its own pass over the layers, so a sequence's K/V rows -- and, K/V being rounded to bf16, its tokens --
  // are the same bits whatever else the call holds (round 3 picked the kernels from the call's TOTAL rows).
  // Diagnostics keep the old single pass: SPARKMI_PREFILL_CHUNKS (chunks only), SPARKMI_PGEMM_MIN_* (per kernel by total rows);
  // the exact-weights mode always takes chunks.
  const bool chunks_only = smi_env("SPARKMI_PREFILL_CHUNKS") != nullptr || L->exact;
  auto cls_of = [&](int b) -> int {
    const int r = lens[b] - 1;
    if (chunks_only) return 0;
    if (L->sw.pg_forced) return total > (size_t)kMaxRows ? 3 : 0;   // 3: one pass, kernels by the pass's row count (launch_layers_big)
    return r <= kMaxRows ? 0 : r < kPfLong ? 1 : 2;
  };
  size_t ncls[4] = {0, 0, 0, 0};
  for (int b = 0; b < B; ++b) ncls[cls_of(b)] += lens[b] - 1;
  const size_t nchunks = (ncls[0] + kMaxRows - 1) / kMaxRows;
  // plan: [class 2 rows][class 1 rows][class 3 rows][class 0 rows, padded to whole chunks][the B last-token rows]
  const size_t off2 = 0, off1 = ncls[2], off3 = off1 + ncls[1], off0 = off3 + ncls[3], tail = off0 + nchunks * kMaxRows;
  int rc;
  const size_t nextra = extra ? extra->size() : 0;
  if ((rc = ensure_plan(L, tail + kMaxRows + nextra))) return rc;
  L->host_rows.assign(tail + kMaxRows + nextra, RowDesc{0, 0, 0, 0});
  {
    size_t w[4] = {off0, off1, off2, off3};
    for (int b = 0; b < B; ++b) {
      size_t& r = w[cls_of(b)];
      for (int t = 0; t + 1 < lens[b]; ++t) L->host_rows[r++] = RowDesc{slots[b], t, (int32_t)ids[(size_t)b * P_max + t], 0};
    }
  }
  for (int b = 0, j = 0; b < B; ++b)
    for (int r = 0; r < (n_ret ? n_ret[b] : 1); ++r, ++j)   // flags = tokens emitted
      L->host_rows[tail + j] = RowDesc{tail_slots ? tail_slots[j] : slots[b], lens[b] - 1, (int32_t)ids[(size_t)b * P_max + lens[b] - 1], 0};
  for (size_t e = 0; e < nextra; ++e) L->host_rows[tail + kMaxRows + e] = (*extra)[e];
  SMI_HIP(hipMemcpyAsync(L->plan, L->host_rows.data(), L->host_rows.size() * sizeof(RowDesc), hipMemcpyHostToDevice, st));
  // measured (tools/prefill_time.py, profiles/README.md): 32-row chunks ~1.4 ms each; row-grouped decode GEMMs
  // ~1.5 ms + 9 us/row; the prefill GEMM ~15 ms + 5 us/row (crossover near 3000 rows)
  const size_t pass_off[3] = {off2, off1, off3}, pass_rows[3] = {ncls[2], ncls[1], ncls[3]};
  const int pass_family[3] = {PF_PGEMM, PF_GROUPED, PF_PGEMM};   // (class 3: the family argument is overridden per kernel by pg_min)
  for (int ps = 0; ps < 3; ++ps) {
    if (pass_rows[ps] == 0) continue;
    // whole groups of up to kBigRows rows through the row-grouped decode GEMMs / the prefill GEMM (k_pgemm)
    constexpr size_t kBigRows = 4096;
    if ((rc = ensure_big(L, (int)(pass_rows[ps] < kBigRows ? pass_rows[ps] : kBigRows)))) return rc;
    for (size_t q0 = 0; q0 < pass_rows[ps]; q0 += kBigRows) {
      const size_t r0 = pass_off[ps] + q0;
      const int M = (int)((pass_rows[ps] - q0) < kBigRows ? (pass_rows[ps] - q0) : kBigRows);
      const RowDesc* rows = L->plan + r0;
      if ((rc = pf_tiles_upload(L, L->host_rows.data() + r0, M, st))) return rc;
      hipLaunchKernelGGL(k_embed, dim3((M + 3) / 4), dim3(256), 0, st, (const uint16_t*)sec(L, SMI_LLM_LM_HEAD, 0), L->KTh, rows, M,
                         (const float*)sec(L, SMI_LLM_LN1, 0), L->big.h, L->big.xs_h, L->big.ss, pf_nparts_in(L, M, pass_family[ps]), 0);
      SMI_LAUNCH_CHECK();
      if ((rc = launch_layers_big(L, rows, M, pass_family[ps], st))) return rc;
    }
  }
  for (size_t c = 0; c < nchunks; ++c) {
    const int M = (int)((ncls[0] - c * kMaxRows) < (size_t)kMaxRows ? (ncls[0] - c * kMaxRows) : kMaxRows);
    const RowDesc* rows = L->plan + off0 + c * kMaxRows;
    if ((rc = launch_embed(L, rows, M, st))) return rc;
    if ((rc = launch_layers(L, rows, M, true, st))) return rc;
  }
  *tail_off = tail;
  return SMI_OK;
}

// The live set changed: rows 0 .. n-1 of the device row list belong to slots[0 .. n-1], in that order.  The next decode picks the
// cached step of the new row count.
static void live_set(smi_llm* L, const int* slots, int n) {
  L->B = n;
  L->live_order.assign(slots, slots + n);
  L->identity_slots = 1;
  L->lm_restrict = n > 0;
  for (int b = 0; b < n; ++b) {
    L->identity_slots &= slots[b] == b;
    L->lm_restrict &= (L->slot_feat[slots[b]] & F_ALLOW) != 0;
  }
  L->graph = nullptr;
}

static int validate_eos(const int64_t* eos_ids, int n_eos) {
  SMI_REQUIRE(n_eos >= 0 && n_eos <= SMI_MAX_EOS && (n_eos == 0 || eos_ids), "eos list: 0..%d ids", SMI_MAX_EOS);
  return SMI_OK;
}

// A new generation (nseq > 0: its sequences are numbered 0 .. nseq-1 up front) or session (nseq = 0: admissions number them).  No
// slot holds a sequence: records, pages, lengths, live rows; eos ids + seed + the slots' sequence numbers and the zeroed counters
// go to the device before anything of the generation is enqueued.  `started` is set only when all of it went through.
static int gen_reset(smi_llm* L, const int64_t* eos_ids, int n_eos, int nseq, hipStream_t st) {
  L->started = 0;
  for (int b = 0; b < kMaxRows; ++b) L->hctl.seqid[b] = nseq ? b : 0;
  slots_clear(L);
  L->admit_seq = nseq;
  if (L->paged)
    for (int b = 0; b < kMaxRows; ++b) pages_release(L, b);
  memset(L->slot_busy, 0, sizeof(L->slot_busy));
  memset(L->slot_len, 0, sizeof(L->slot_len));
  memset(L->slot_plen, 0, sizeof(L->slot_plen));
  ++L->session_gen;   // blobs of the earlier sessions are refused from here on
  live_set(L, nullptr, 0);
  for (int e = 0; e < SMI_MAX_EOS; ++e) L->hctl.eos[e] = e < n_eos ? (long long)eos_ids[e] : -1;
  L->hctl.n_eos = n_eos;
  L->hctl.seed = L->seed;
  SMI_HIP(hipMemcpyAsync(L->ctl, &L->hctl, sizeof(Ctl), hipMemcpyHostToDevice, st));
  SMI_HIP(hipMemsetAsync(L->count, 0, kMaxRows * 4, st));
  SMI_HIP(hipMemsetAsync(L->finished, 0, kMaxRows * 4, st));
  SMI_HIP(hipMemsetAsync(L->step, 0, 4, st));
  L->session = nseq == 0;
  L->started = 1;
  return SMI_OK;
}

// Plain generation is the session state with slots 0 .. B-1 busy: the rows are written by the prefill plan itself, so nothing
// is read back from the device (admit does) and the call does not synchronise.
int smi_llm_prefill(smi_llm* L, const int64_t* ids, const int32_t* lens, int B, int P_max, const int64_t* eos_ids, int n_eos,
                    void* stream) {
  SMI_REQUIRE(L && ids && lens, "smi_llm_prefill: null argument");
  SMI_REQUIRE(B >= 1 && B <= L->cfg.max_slots, "smi_llm_prefill: B=%d outside 1..%d", B, L->cfg.max_slots);
  hipStream_t st = (hipStream_t)stream;
  int32_t slots[kMaxRows];
  for (int b = 0; b < kMaxRows; ++b) slots[b] = b;
  int rc;
  if ((rc = validate_prompts(L, ids, lens, B, P_max)) || (rc = validate_eos(eos_ids, n_eos))) return rc;   // nothing touched yet
  if (L->paged) {   // a new generation: every page back to the pool, then what the prompts need
    // the demand is checked against the WHOLE pool first (everything is about to be free), so a prompt set that cannot fit
    // fails here with the previous generation's pages, table and `started` flag untouched
    long need = 0;
    for (int b = 0; b < B; ++b) need += (lens[b] + (1 << L->pshift) - 1) >> L->pshift;
    if (need > L->cfg.kv_pages) {
      smi_set_error("KV page pool too small for these prompts: %ld pages of %d tokens needed, the pool has %d", need, 1 << L->pshift, L->cfg.kv_pages);
      return SMI_ENOMEM;
    }
  }
  if ((rc = gen_reset(L, eos_ids, n_eos, B, st))) return rc;
  if ((rc = pages_ensure(L, slots, lens, B, st))) { L->started = 0; return rc; }   // (cannot happen after the check above; the old generation is gone by now)
  for (int b = 0; b < B; ++b) { L->slot_busy[b] = 1; L->slot_len[b] = lens[b] + 1; L->slot_plen[b] = lens[b]; }   // (the first step, enqueued below, takes position lens[b])
  live_set(L, slots, B);
  // the captured decode step is kept across utterances: eos ids and the seed live in device memory (Ctl); smi_llm_decode
  // re-captures only when the row count, the context-segment count or the slot mapping differ from the captured ones
  size_t tail = 0;
  if ((rc = prefill_prompts(L, ids, lens, B, P_max, slots, &tail, st))) { L->started = 0; return rc; }
  if (hipMemcpyAsync(L->rows, L->plan + tail, kMaxRows * sizeof(RowDesc), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    L->started = 0;
    smi_set_error("smi_llm_prefill: copying the first step's rows failed");
    return SMI_EHIP;
  }
  if ((rc = launch_embed(L, L->rows, B, st)) || (rc = launch_step(L, B, st))) { L->started = 0; return rc; }
  return SMI_OK;
}

// ---- continuous batching: sequences join (admit) and leave (retire) between decode steps ----
int smi_llm_session_begin(smi_llm* L, const int64_t* eos_ids, int n_eos, void* stream) {
  SMI_REQUIRE(L, "smi_llm_session_begin: null handle");
  { const int rcv = validate_eos(eos_ids, n_eos); if (rcv) return rcv; }
  return gen_reset(L, eos_ids, n_eos, 0, (hipStream_t)stream);
}

// the live row set changed: refresh the device rows, the per-row residual / operand state, and drop the graph
static int session_set_rows(smi_llm* L, const std::vector<RowDesc>& live, hipStream_t st) {
  int slots[kMaxRows];
  for (size_t b = 0; b < live.size(); ++b) slots[b] = live[b].slot;
  live_set(L, slots, (int)live.size());
  if (L->B == 0) return SMI_OK;
  L->host_rows.assign(kMaxRows, RowDesc{0, 0, 0, 0});
  for (int b = 0; b < L->B; ++b) L->host_rows[b] = live[b];
  SMI_HIP(hipMemcpyAsync(L->rows, L->host_rows.data(), kMaxRows * sizeof(RowDesc), hipMemcpyHostToDevice, st));
  SMI_HIP(hipStreamSynchronize(st));    // host_rows is reused by the next call
  return launch_embed(L, L->rows, L->B, st);   // h = E[token], first-norm operand, sum of squares of every live row
}

static int session_live_rows(smi_llm* L, std::vector<RowDesc>& live, hipStream_t st) {
  live.assign((size_t)L->B, RowDesc{0, 0, 0, 0});
  SMI_HIP(hipStreamSynchronize(st));
  if (L->B) SMI_HIP(hipMemcpy(live.data(), L->rows, (size_t)L->B * sizeof(RowDesc), hipMemcpyDeviceToHost));
  return SMI_OK;
}

// Checks of the sampling records of an admission (before anything of the handle is touched, like validate_prompts).
static int validate_sampling(const smi_sample_params* sp, int n) {
  if (!sp) return SMI_OK;
  for (int b = 0; b < n; ++b) {
    const smi_sample_params& r = sp[b];
    SMI_REQUIRE(r.mode == SMI_SAMPLING_INHERIT || r.mode == SMI_SAMPLING_GREEDY || r.mode == SMI_SAMPLING_SAMPLE,
                "smi_llm_admit_sampled: params[%d].mode=%d is not an SMI_SAMPLING_* value", b, r.mode);
    if (r.mode != SMI_SAMPLING_SAMPLE) continue;
    SMI_REQUIRE(r.temperature > 0.f && std::isfinite(r.temperature), "smi_llm_admit_sampled: params[%d].temperature must be finite and > 0", b);
    SMI_REQUIRE(r.top_k >= 1 && r.top_k <= kSampleCap, "smi_llm_admit_sampled: params[%d].top_k=%d outside 1..%d", b, r.top_k, kSampleCap);
    SMI_REQUIRE(r.top_p > 0.f && r.top_p <= 1.f, "smi_llm_admit_sampled: params[%d].top_p must be in (0, 1]", b);
    SMI_REQUIRE(r.has_seed == 0 || r.has_seed == 1, "smi_llm_admit_sampled: params[%d].has_seed must be 0 or 1", b);
  }
  return SMI_OK;
}

static SampRec samp_record(const smi_sample_params* sp, int V) {
  SampRec r;
  memset(&r, 0, sizeof(r));
  if (!sp || sp->mode == SMI_SAMPLING_INHERIT) return r;
  r.mode = sp->mode;
  if (sp->mode != SMI_SAMPLING_SAMPLE) return r;
  r.top_k = sp->top_k < V ? sp->top_k : V;
  r.inv_temp = 1.0f / sp->temperature;   // the handle's settings are applied the same way (1 / T in the launch)
  r.top_p = sp->top_p;
  r.seed = sp->seed;
  r.has_seed = sp->has_seed;
  return r;
}

// The history rows of an admission's penalised sequences, before their first step: zeroed, then the prompt bits (records that
// penalise their prompt).  Rows without a record are never touched.
static int pen_histories(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const int32_t* slots, hipStream_t st) {
  const size_t V = (size_t)L->cfg.vocab_size;
  std::vector<int32_t>& idx = L->host_pen_idx;
  idx.clear();
  for (int b = 0; b < n; ++b) {
    const PenRec& r = L->hctl.pen[slots[b]];
    if (!r.on) continue;
    SMI_HIP(hipMemsetAsync(L->phist + (size_t)slots[b] * V, 0, V * 2, st));
    if (r.prompt)
      for (int t = 0; t < lens[b]; ++t) idx.push_back((int32_t)((size_t)slots[b] * V + (size_t)ids[(size_t)b * P_max + t]));
  }
  if (idx.empty()) return SMI_OK;
  if (idx.size() * 4 > L->pen_idx.bytes())
    if (int rc = L->pen_idx.ensure((idx.size() + 4096) * 4, "penalty prompt ids")) return rc;
  // (pageable source: staged before the call returns; host_pen_idx is rebuilt only by the next admission)
  SMI_HIP(hipMemcpyAsync(L->pen_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pen_prompt, dim3((unsigned)((idx.size() + 255) / 256)), dim3(256), 0, st, L->phist, L->pen_idx, (int)idx.size());
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

// Checks of one penalty record (smi_llm_admit_penalized, smi_llm_debug_penalize).
static int validate_penalty(const smi_llm* L, const smi_penalty_params& r, int b) {
  SMI_REQUIRE(std::isfinite(r.repetition_penalty) && r.repetition_penalty > 0.f,
              "smi_llm_admit_penalized: pens[%d].repetition_penalty must be finite and > 0", b);
  SMI_REQUIRE(std::isfinite(r.presence_penalty) && r.presence_penalty >= -2.f && r.presence_penalty <= 2.f,
              "smi_llm_admit_penalized: pens[%d].presence_penalty must be in [-2, 2]", b);
  SMI_REQUIRE(std::isfinite(r.frequency_penalty) && r.frequency_penalty >= -2.f && r.frequency_penalty <= 2.f,
              "smi_llm_admit_penalized: pens[%d].frequency_penalty must be in [-2, 2]", b);
  SMI_REQUIRE(r.min_new_tokens >= 0 && r.min_new_tokens <= L->cfg.max_positions,
              "smi_llm_admit_penalized: pens[%d].min_new_tokens=%d outside 0..%d", b, r.min_new_tokens, L->cfg.max_positions);
  SMI_REQUIRE(r.penalize_prompt == 0 || r.penalize_prompt == 1, "smi_llm_admit_penalized: pens[%d].penalize_prompt must be 0 or 1", b);
  SMI_REQUIRE(r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0, "smi_llm_admit_penalized: pens[%d].reserved must be 0", b);
  return SMI_OK;
}

static PenRec pen_record(const smi_penalty_params* pp) {
  PenRec r;
  memset(&r, 0, sizeof(r));
  if (!pp || (pp->repetition_penalty == 1.f && pp->presence_penalty == 0.f && pp->frequency_penalty == 0.f && pp->min_new_tokens == 0))
    return r;   // neutral: not penalised
  r.rep = pp->repetition_penalty; r.pres = pp->presence_penalty; r.freq = pp->frequency_penalty;
  r.min_new = pp->min_new_tokens; r.prompt = pp->penalize_prompt; r.on = 1;
  return r;
}

// Checks of one allow record (smi_llm_admit_constrained; before anything of the handle is touched).  pen: the take's penalty
// record or null.
static int validate_allow(const smi_llm* L, const smi_allow_params& a, const smi_penalty_params* pen, int j) {
  const int V = L->cfg.vocab_size;
  SMI_REQUIRE(a.n_ranges >= 0 && a.n_ranges <= SMI_MAX_ALLOW_RANGES, "smi_llm_admit_constrained: allow[%d].n_ranges=%d outside 0..%d", j,
              a.n_ranges, SMI_MAX_ALLOW_RANGES);
  SMI_REQUIRE(a.reserved == 0, "smi_llm_admit_constrained: allow[%d].reserved must be 0", j);
  long covered = 0;
  for (int i = 0; i < a.n_ranges; ++i) {
    SMI_REQUIRE(a.lo[i] >= 0 && a.lo[i] < a.hi[i] && a.hi[i] <= V, "smi_llm_admit_constrained: allow[%d] range %d = [%d, %d) is not inside [0, %d) or empty",
                j, i, a.lo[i], a.hi[i], V);
    SMI_REQUIRE(i == 0 || a.hi[i - 1] <= a.lo[i], "smi_llm_admit_constrained: allow[%d] ranges %d and %d are not sorted and disjoint", j, i - 1, i);
    covered += a.hi[i] - a.lo[i];
  }
  if (pen && pen->min_new_tokens > 0 && a.n_ranges > 0) {   // some id of the set must stay selectable while eos is banned
    long eos_in = 0;
    for (int e = 0; e < L->hctl.n_eos; ++e) {
      const long long id = L->hctl.eos[e];
      bool dup = false;
      for (int f = 0; f < e; ++f) dup |= L->hctl.eos[f] == id;
      if (dup) continue;
      for (int i = 0; i < a.n_ranges; ++i) eos_in += id >= a.lo[i] && id < a.hi[i];
    }
    SMI_REQUIRE(covered > eos_in, "smi_llm_admit_constrained: allow[%d] holds only eos ids but min_new_tokens=%d bans them", j, pen->min_new_tokens);
  }
  return SMI_OK;
}

// The device record of an allow record: n = 0 for none and for a neutral one (no ranges, or ranges that cover [0, V)).
static AllowRec allow_record(const smi_allow_params* a, int V) {
  AllowRec r;
  memset(&r, 0, sizeof(r));
  if (!a || a->n_ranges == 0) return r;
  long covered = 0;
  for (int i = 0; i < a->n_ranges; ++i) covered += a->hi[i] - a->lo[i];
  if (covered == V) return r;
  r.n = a->n_ranges;
  for (int i = 0; i < a->n_ranges; ++i) { r.lo[i] = a->lo[i]; r.hi[i] = a->hi[i]; }
  return r;
}

// The restricted lm_head's tile list -> device, in stream order: the 16-id vocabulary tiles that hold an id of some constrained
// slot's set (live or being admitted), ascending.  Nothing to do while no slot is constrained (the list is not read).
static int allow_tiles_upload(smi_llm* L, hipStream_t st) {
  if (!(step_feat(L) & F_ALLOW)) return SMI_OK;
  std::vector<char> mark((size_t)L->NTlm, 0);
  for (int sl = 0; sl < kMaxRows; ++sl) {
    if (!(L->slot_feat[sl] & F_ALLOW)) continue;
    const AllowRec& a = L->hctl.allow[sl];
    for (int i = 0; i < a.n; ++i)
      for (int t = a.lo[i] >> 4; t <= (a.hi[i] - 1) >> 4; ++t) mark[(size_t)t] = 1;
  }
  std::vector<int32_t>& T = L->host_tlist;
  T.assign(1, 0);
  for (int t = 0; t < L->NTlm; ++t)
    if (mark[(size_t)t]) T.push_back(t);
  T[0] = (int32_t)T.size() - 1;
  // (pageable source: staged before the call returns; host_tlist is rebuilt only by the next admission or retirement)
  SMI_HIP(hipMemcpyAsync(L->tlist, T.data(), T.size() * 4, hipMemcpyHostToDevice, st));
  return SMI_OK;
}

// The static survivor count of a take: the ids of its allowed set (the vocabulary without one) minus the distinct last ids of
// its -inf bias entries, minus the eos ids when min_new_tokens > 0.  al / pen / q: the take's records or null.
static long survivors(const smi_llm* L, const smi_allow_params* al, const smi_penalty_params* pen, const smi_seq_params* q) {
  const int V = L->cfg.vocab_size;
  const bool con = al && al->n_ranges > 0;
  auto allowed = [&](long long id) {
    if (!con) return true;
    for (int i = 0; i < al->n_ranges; ++i)
      if (id >= al->lo[i] && id < al->hi[i]) return true;
    return false;
  };
  long covered = V;
  if (con) { covered = 0; for (int i = 0; i < al->n_ranges; ++i) covered += al->hi[i] - al->lo[i]; }
  std::vector<long long> gone;   // distinct ids of the set that cannot be chosen
  auto drop = [&](long long id) {
    if (id < 0 || id >= V || !allowed(id)) return;
    for (long long g : gone) if (g == id) return;
    gone.push_back(id);
  };
  if (q)
    for (int i = 0; i < q->n_bias; ++i)
      if (std::isinf(q->bias[i])) drop(q->bias_ids[(size_t)i * SMI_MAX_SEQ_LEN + q->bias_len[i] - 1]);
  if (pen && pen->min_new_tokens > 0)
    for (int e = 0; e < L->hctl.n_eos; ++e) drop(L->hctl.eos[e]);
  return covered - (long)gone.size();
}

// Checks of one bias / stop record (smi_llm_admit_biased, smi_llm_debug_seqbias; before anything of the handle is touched).
// al / pen: the take's allow and penalty records or null (al has passed validate_allow).
static int validate_seq(const smi_llm* L, const smi_seq_params& q, const smi_allow_params* al, const smi_penalty_params* pen, int j) {
  const int V = L->cfg.vocab_size;
  SMI_REQUIRE(q.n_bias >= 0 && q.n_bias <= SMI_MAX_BIAS_SEQS, "smi_llm_admit_biased: seq[%d].n_bias=%d outside 0..%d", j, q.n_bias, SMI_MAX_BIAS_SEQS);
  SMI_REQUIRE(q.n_stop >= 0 && q.n_stop <= SMI_MAX_STOP_SEQS, "smi_llm_admit_biased: seq[%d].n_stop=%d outside 0..%d", j, q.n_stop, SMI_MAX_STOP_SEQS);
  SMI_REQUIRE(q.reserved[0] == 0 && q.reserved[1] == 0, "smi_llm_admit_biased: seq[%d].reserved must be 0", j);
  auto same = [](const int32_t* a, int la, const int32_t* b, int lb) { return la == lb && memcmp(a, b, (size_t)la * 4) == 0; };
  for (int i = 0; i < q.n_bias; ++i) {
    const int len = q.bias_len[i];
    const int32_t* e = q.bias_ids + (size_t)i * SMI_MAX_SEQ_LEN;
    SMI_REQUIRE(len >= 1 && len <= SMI_MAX_SEQ_LEN, "smi_llm_admit_biased: seq[%d].bias_len[%d]=%d outside 1..%d", j, i, len, SMI_MAX_SEQ_LEN);
    for (int t = 0; t < len; ++t)
      SMI_REQUIRE(e[t] >= 0 && e[t] < V, "smi_llm_admit_biased: seq[%d] bias entry %d holds id %d outside [0, %d)", j, i, e[t], V);
    SMI_REQUIRE(!std::isnan(q.bias[i]) && !(std::isinf(q.bias[i]) && q.bias[i] > 0.f),
                "smi_llm_admit_biased: seq[%d].bias[%d] must be finite or -inf", j, i);
    for (int f = 0; f < i; ++f)
      SMI_REQUIRE(!same(e, len, q.bias_ids + (size_t)f * SMI_MAX_SEQ_LEN, q.bias_len[f]),
                  "smi_llm_admit_biased: seq[%d] bias entries %d and %d are the same sequence", j, f, i);
  }
  for (int i = 0; i < q.n_stop; ++i) {
    const int len = q.stop_len[i];
    const int32_t* e = q.stop_ids + (size_t)i * SMI_MAX_SEQ_LEN;
    SMI_REQUIRE(len >= 1 && len <= SMI_MAX_SEQ_LEN, "smi_llm_admit_biased: seq[%d].stop_len[%d]=%d outside 1..%d", j, i, len, SMI_MAX_SEQ_LEN);
    for (int t = 0; t < len; ++t)
      SMI_REQUIRE(e[t] >= 0 && e[t] < V, "smi_llm_admit_biased: seq[%d] stop sequence %d holds id %d outside [0, %d)", j, i, e[t], V);
    for (int f = 0; f < i; ++f)
      SMI_REQUIRE(!same(e, len, q.stop_ids + (size_t)f * SMI_MAX_SEQ_LEN, q.stop_len[f]),
                  "smi_llm_admit_biased: seq[%d] stop sequences %d and %d are the same", j, f, i);
  }
  // a survivor is left, with the eos ids and again without them while min_new_tokens bans them
  SMI_REQUIRE(survivors(L, al, nullptr, &q) > 0, "smi_llm_admit_biased: seq[%d] bans every id the row could emit", j);
  if (pen && pen->min_new_tokens > 0)
    SMI_REQUIRE(survivors(L, al, pen, &q) > 0, "smi_llm_admit_biased: seq[%d] leaves only eos ids but min_new_tokens=%d bans them", j, pen->min_new_tokens);
  return SMI_OK;
}

// Checks of one no_repeat_ngram_size (smi_llm_admit_ngram; before anything of the handle is touched).  al / pen / q: the take's
// allow, penalty and bias records or null (they have passed their own checks).  A step bans at most max_positions - 1 distinct
// ids, so a row with n > 0 needs max_positions survivors: the allowed set (or the vocabulary) minus the distinct last ids of
// the -inf bias entries, minus the eos ids when min_new_tokens > 0 -- then no row reaches selection with every logit -inf.
static int validate_ngram(const smi_llm* L, int32_t n, const smi_allow_params* al, const smi_penalty_params* pen, const smi_seq_params* q, int j) {
  SMI_REQUIRE(n >= 0 && n <= SMI_MAX_NGRAM, "smi_llm_admit_ngram: no_repeat_ngram[%d]=%d outside 0..%d", j, n, SMI_MAX_NGRAM);
  if (n == 0) return SMI_OK;
  const long left = survivors(L, al, pen, q);
  SMI_REQUIRE(left >= (long)L->cfg.max_positions,
              "smi_llm_admit_ngram: no_repeat_ngram[%d]=%d needs %d selectable ids (max_positions), the row has %ld", j, n,
              L->cfg.max_positions, left);
  return SMI_OK;
}

// The device record of a bias / stop record admitted with the prompt ids[0 .. len); all zero for none and for a neutral one.
static SeqRec seq_record(const smi_seq_params* q, const int64_t* ids, int len) {
  SeqRec r;
  memset(&r, 0, sizeof(r));
  if (!q || (q->n_bias == 0 && q->n_stop == 0)) return r;
  r.n_bias = q->n_bias; r.n_stop = q->n_stop; r.plen = len;
  r.n_ptail = len < SMI_MAX_SEQ_LEN - 1 ? len : SMI_MAX_SEQ_LEN - 1;
  for (int k = 1; k <= r.n_ptail; ++k) r.ptail[SMI_MAX_SEQ_LEN - 1 - k] = (int32_t)ids[len - k];
  for (int i = 0; i < q->n_bias; ++i) {
    r.blen[i] = q->bias_len[i]; r.bias[i] = q->bias[i];
    for (int t = 0; t < q->bias_len[i]; ++t) r.bids[i][t] = q->bias_ids[(size_t)i * SMI_MAX_SEQ_LEN + t];
  }
  for (int i = 0; i < q->n_stop; ++i) {
    r.slen[i] = q->stop_len[i];
    for (int t = 0; t < q->stop_len[i]; ++t) r.sids[i][t] = q->stop_ids[(size_t)i * SMI_MAX_SEQ_LEN + t];
  }
  return r;
}

// One admission, as the smi_llm_admit* entry points hand it over.  n_ret[b] takes of prompt b (null or all ones: one each);
// the record arrays hold one record per take (N = sum of n_ret), and a null array is no record for any take.  An entry point
// names the members it takes; the ones after them are null, so a new kind of record is a new last member.
struct AdmitReq {
  const int64_t* ids; const int32_t* lens; int n, P_max;
  const int32_t* n_ret;
  const smi_sample_params* params;
  const smi_penalty_params* pens;
  const int32_t* want_lp;
  const smi_allow_params* allow;
  const smi_seq_params* seq;
  const int32_t* ngram;
};

// What a KV slot holds of its sequence on the host: the admission number, the records of Ctl and the feature bits.
struct SlotRecs {
  int32_t seqid; SampRec samp; PenRec pen; int32_t lp; AllowRec allow; int32_t ngram, ngplen; uint8_t feat;
};
static SlotRecs recs_get(const smi_llm* L, int sl) {
  return SlotRecs{L->hctl.seqid[sl], L->hctl.samp[sl], L->hctl.pen[sl], L->hctl.lp[sl], L->hctl.allow[sl], L->hctl.ngram[sl],
                  L->hctl.ngplen[sl], L->slot_feat[sl]};
}
static void recs_put(smi_llm* L, int sl, const SlotRecs& r) {
  L->hctl.seqid[sl] = r.seqid; L->hctl.samp[sl] = r.samp; L->hctl.pen[sl] = r.pen; L->hctl.lp[sl] = r.lp; L->hctl.allow[sl] = r.allow;
  L->hctl.ngram[sl] = r.ngram; L->hctl.ngplen[sl] = r.ngplen;
  L->slot_feat[sl] = r.feat;
}

// ---- the steps every way into a KV slot shares: an admission (admit) and the return of a parked sequence
// (smi_llm_slots_restore) take slots, install records and enter the live row list through these ----
// The n lowest free KV slots, in order; returns how many there are (fewer than n: the caller refuses).
static int slots_take_free(const smi_llm* L, int n, int32_t* slots) {
  const int slot_cap = L->cfg.max_slots < kMaxRows ? L->cfg.max_slots : kMaxRows;
  int k = 0;
  for (int sl = 0; sl < slot_cap && k < n; ++sl)
    if (!L->slot_busy[sl]) slots[k++] = sl;
  return k;
}
// The records of N new sequences go into their slots, on the host and on the device: Ctl (with the sequence numbers), the union
// of the constrained slots' tiles, the bias / stop records (which add F_BIAS / F_STOP to the feature byte).  A slot whose device
// bias / stop record is all zero and stays so is not touched.  old[] receives what the slots held; on an error the caller
// calls recs_withdraw.
static int recs_install(smi_llm* L, const char* who, const int32_t* slots, int N, const SlotRecs* recs, const SeqRec* seqs, SlotRecs* old,
                        hipStream_t st) {
  for (int j = 0; j < N; ++j) {
    old[j] = recs_get(L, slots[j]);
    recs_put(L, slots[j], recs[j]);
  }
  if (hipMemcpyAsync(L->ctl, &L->hctl, sizeof(Ctl), hipMemcpyHostToDevice, st) != hipSuccess) {
    smi_set_error("%s: uploading the generation controls failed", who);
    return SMI_EHIP;
  }
  { const int rc = allow_tiles_upload(L, st); if (rc) return rc; }   // the union now holds the new sequences' tiles
  for (int j = 0; j < N; ++j) {
    const int sl = slots[j];
    const SeqRec& rec = seqs[j];
    const int on = rec.n_bias > 0 || rec.n_stop > 0;
    L->slot_feat[sl] |= (rec.n_bias > 0 ? F_BIAS : 0) | (rec.n_stop > 0 ? F_STOP : 0);
    if (!on && !L->seq_dirty[sl]) continue;
    L->hseq[(size_t)sl] = rec;
    L->seq_dirty[sl] = on;
    // (pageable source: staged before the call returns; hseq[sl] is rewritten only by a later entry into the slot)
    if (hipMemcpyAsync(L->seq + sl, &L->hseq[(size_t)sl], sizeof(SeqRec), hipMemcpyHostToDevice, st) != hipSuccess) {
      L->seq_dirty[sl] = 1;
      smi_set_error("%s: uploading the sequence records failed", who);
      return SMI_EHIP;
    }
  }
  return SMI_OK;
}
// Nobody entered after all: records and pages (and page references) as before (the device copy is rewritten by the next entry;
// seq_dirty stays: the next entry rewrites the device record).
static void recs_withdraw(smi_llm* L, const int32_t* slots, int N, const SlotRecs* old) {
  for (int j = 0; j < N; ++j) { recs_put(L, slots[j], old[j]); slot_clear(L, slots[j]); }
  if (L->paged)
    for (int j = 0; j < N; ++j) pages_release(L, slots[j]);
}
// The N sequences are in their slots: busy, with their lengths, their rows behind the live ones; every live row is re-embedded
// from E[token] (session_set_rows).
static int slots_enter(smi_llm* L, std::vector<RowDesc>& live, const int32_t* slots, int N, const RowDesc* rows, const int32_t* plen,
                       const int32_t* len, int32_t* slots_out, hipStream_t st) {
  for (int j = 0; j < N; ++j) {
    live.push_back(rows[j]);
    L->slot_busy[slots[j]] = 1;
    L->slot_len[slots[j]] = len[j];
    L->slot_plen[slots[j]] = plen[j];
    slots_out[j] = slots[j];
  }
  return session_set_rows(L, live, st);
}

static int admit(smi_llm* L, const AdmitReq& rq, int32_t* slots_out, hipStream_t st) {
  const int64_t* ids = rq.ids;
  const int32_t *lens = rq.lens, *n_ret = rq.n_ret, *want_lp = rq.want_lp;
  const int n = rq.n, P_max = rq.P_max;
  const smi_sample_params* params = rq.params;
  const smi_penalty_params* pens = rq.pens;
  const smi_allow_params* allow = rq.allow;
  const smi_seq_params* seq = rq.seq;
  const int32_t* ngram = rq.ngram;
  SMI_REQUIRE(L && ids && lens && slots_out, "smi_llm_admit: null argument");
  if (!L->started || !L->session) { smi_set_error("smi_llm_admit outside a session (smi_llm_session_begin first)"); return SMI_ESTATE; }
  const int slot_cap = L->cfg.max_slots < kMaxRows ? L->cfg.max_slots : kMaxRows;
  int N = n;   // output sequences (takes)
  bool forked = false;
  if (n_ret && n >= 1) {
    N = 0;
    for (int b = 0; b < n; ++b) {
      SMI_REQUIRE(n_ret[b] >= 1 && n_ret[b] <= kMaxRows, "smi_llm_admit_forked: n_return[%d]=%d outside 1..%d", b, n_ret[b], kMaxRows);
      N += n_ret[b];
      forked |= n_ret[b] > 1;
    }
  }
  SMI_REQUIRE(n >= 1 && L->B + N <= slot_cap, "smi_llm_admit: %d new + %d live sequences exceed %d slots", N, L->B, slot_cap);
  { const int rcs = validate_sampling(params, N); if (rcs) return rcs; }   // nothing touched yet
  if (pens)
    for (int j = 0; j < N; ++j) { const int rcp = validate_penalty(L, pens[j], j); if (rcp) return rcp; }
  if (want_lp)
    for (int j = 0; j < N; ++j)
      SMI_REQUIRE(want_lp[j] == 0 || want_lp[j] == 1, "smi_llm_admit_logprobs: return_log_probs[%d]=%d must be 0 or 1", j, want_lp[j]);
  if (allow)
    for (int j = 0; j < N; ++j) { const int rca = validate_allow(L, allow[j], pens ? &pens[j] : nullptr, j); if (rca) return rca; }
  if (seq)
    for (int j = 0; j < N; ++j) {
      const int rcq = validate_seq(L, seq[j], allow ? &allow[j] : nullptr, pens ? &pens[j] : nullptr, j);
      if (rcq) return rcq;
    }
  if (ngram)
    for (int j = 0; j < N; ++j) {
      const int rcn = validate_ngram(L, ngram[j], allow ? &allow[j] : nullptr, pens ? &pens[j] : nullptr, seq ? &seq[j] : nullptr, j);
      if (rcn) return rcn;
    }
  int rc;
  std::vector<RowDesc> live;
  if ((rc = session_live_rows(L, live, st))) return rc;
  int32_t slots[kMaxRows];   // one per take, lowest free first
  SMI_REQUIRE(slots_take_free(L, N, slots) == N, "smi_llm_admit: no free KV slot");
  if ((rc = validate_prompts(L, ids, lens, n, P_max))) return rc;   // nothing touched yet
  // take j belongs to prompt src[j]; the first take of a prompt is its leader, the slot its prompt rows are prefilled in
  int32_t src[kMaxRows], lead[kMaxRows], lens_j[kMaxRows];
  for (int b = 0, j = 0; b < n; ++b) {
    lead[b] = slots[j];
    for (int r = 0; r < (n_ret ? n_ret[b] : 1); ++r, ++j) { src[j] = b; lens_j[j] = lens[b]; }
  }
  const int P = L->paged ? 1 << L->pshift : 0;
  auto shared_pages = [&](int b) { return (lens[b] - 1) >> L->pshift; };   // S = floor((L - 1) / P): positions < S P <= L - 1
  if (L->paged && forked) {   // the whole demand first: a short pool takes nothing (pages_ensure below cannot fail after this)
    long need = 0;
    for (int b = 0; b < n; ++b) {
      const int own = (lens[b] + P - 1) >> L->pshift;
      need += own + (long)(n_ret[b] - 1) * (own - shared_pages(b));
    }
    if (need > (long)L->free_pages.size()) {
      smi_set_error("KV page pool exhausted: %ld more pages of %d tokens needed, %zu of %d free (retire a sequence or enlarge kv_pages)",
                    need, P, L->free_pages.size(), L->cfg.kv_pages);
      return SMI_ENOMEM;
    }
  }
  if (L->paged && (rc = pages_ensure(L, lead, lens, n, st))) return rc;   // all or nothing: a short pool admits nobody
  if (L->paged && forked) {   // followers: the leader's first S pages shared, their own pages from page S on
    int32_t fsl[kMaxRows], flen[kMaxRows];
    int nf = 0;
    for (int j = 0; j < N; ++j)
      if (slots[j] != lead[src[j]]) {
        pages_share(L, lead[src[j]], slots[j], shared_pages(src[j]));
        fsl[nf] = slots[j]; flen[nf++] = lens_j[j];
      }
    if ((rc = pages_ensure(L, fsl, flen, nf, st))) {
      for (int j = 0; j < N; ++j) pages_release(L, slots[j]);
      return rc;
    }
  }
  // the records go up with the sequence numbers, before the admission's own step: its finalize emits the first token
  const int seq0 = L->admit_seq;
  SlotRecs old[kMaxRows], recs[kMaxRows];
  std::vector<SeqRec> seqs((size_t)N);   // the bias / stop records of the new takes (a fork's followers get their prompt's tail)
  for (int j = 0; j < N; ++j) {
    SlotRecs& r = recs[j];
    r.seqid = L->admit_seq++;
    r.samp = samp_record(params ? &params[j] : nullptr, L->cfg.vocab_size);
    r.pen = pen_record(pens ? &pens[j] : nullptr);
    r.lp = want_lp ? want_lp[j] : 0;
    r.allow = allow_record(allow ? &allow[j] : nullptr, L->cfg.vocab_size);
    r.ngram = ngram ? ngram[j] : 0;
    r.ngplen = r.ngram > 0 ? lens_j[j] : 0;
    r.feat = (r.samp.mode == SMI_SAMPLING_SAMPLE ? F_SAMPLE : 0) | (r.pen.on ? F_PEN : 0) | (r.lp ? F_LP : 0) | (r.allow.n > 0 ? F_ALLOW : 0) |
             (r.ngram > 0 ? F_NGRAM : 0);   // (F_BIAS / F_STOP: recs_install, from the sequence record)
    seqs[(size_t)j] = seq_record(seq ? &seq[j] : nullptr, ids + (size_t)src[j] * P_max, lens_j[j]);
  }
  // undo: nothing was admitted -- sequence numbers, records and pages (and page references) as before
  auto undo = [&]() {
    recs_withdraw(L, slots, N, old);
    L->admit_seq = seq0;
  };
  if ((rc = recs_install(L, "smi_llm_admit", slots, N, recs, seqs.data(), old, st))) { undo(); return rc; }
  // the prompt ids of the takes that ban n-grams -> their slots' rows of the context store (a fork's followers get their
  // leader's prompt); a slot admitted without the feature never reads its row
  if (ngram) {
    std::vector<int32_t>& H = L->host_pctx;
    H.clear();
    for (int j = 0; j < N; ++j)
      if (ngram[j] > 0)
        for (int t = 0; t < lens_j[j]; ++t) H.push_back((int32_t)ids[(size_t)src[j] * P_max + t]);
    size_t at = 0;
    for (int j = 0; j < N; ++j) {
      if (ngram[j] <= 0) continue;
      // (pageable source: staged before the call returns; host_pctx is rebuilt only by the next admission)
      if (hipMemcpyAsync(L->pctx + (size_t)slots[j] * L->cfg.max_positions, H.data() + at, (size_t)lens_j[j] * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
        undo();
        smi_set_error("smi_llm_admit_ngram: uploading the prompt ids failed");
        return SMI_EHIP;
      }
      at += (size_t)lens_j[j];
    }
  }
  // the fork copy's work list: each follower gets the leader's positions it does not share -- 0 .. L-2 (contiguous), S P .. L-2
  // (paged); position L-1 and on are written by the follower's own steps
  std::vector<RowDesc> fork;
  int fork_span = 0;
  if (forked)
    for (int j = 0; j < N; ++j) {
      const int b = src[j], p0 = L->paged ? shared_pages(b) << L->pshift : 0, p1 = lens[b] - 1;
      if (slots[j] == lead[b] || p1 <= p0) continue;
      fork.push_back(RowDesc{lead[b], slots[j], p0, p1});
      fork_span = p1 - p0 > fork_span ? p1 - p0 : fork_span;
    }
  size_t tail = 0;
  if ((rc = prefill_prompts(L, ids, lens, n, P_max, lead, &tail, st, n_ret, slots, fork.empty() ? nullptr : &fork))) { undo(); return rc; }
  if (!fork.empty()) {   // after the leaders' prompt rows, before the takes' first step
    ForkP fp;
    fp.work = (const int4*)(L->plan + tail + kMaxRows);
    fp.kcache = (unsigned char*)L->kcache.get(); fp.vcache = (unsigned char*)L->vcache.get();
    fp.piece_shift = L->cfg.kv_dtype ? 4 : 3;
    fp.layer_bytes = L->kv_layer_elems * (L->cfg.kv_dtype ? 4 : 2);
    fp.n_kv = L->cfg.num_kv_heads; fp.max_pos = L->cfg.max_positions;
    fp.km = kv_map(L);
    const dim3 grid((unsigned)(((size_t)fork_span << fp.piece_shift) + 255) / 256, (unsigned)fork.size(),
                    (unsigned)(L->cfg.num_layers * 2 * L->cfg.num_kv_heads));
    hipLaunchKernelGGL(k_kv_fork, grid, dim3(256), 0, st, fp);
    SMI_LAUNCH_CHECK();
  }
  // first token of the new sequences: one step over the new rows alone
  int32_t zeros[kMaxRows] = {0};
  for (int j = 0; j < N; ++j) {
    SMI_HIP(hipMemcpyAsync(L->count + slots[j], zeros, 4, hipMemcpyHostToDevice, st));
    SMI_HIP(hipMemcpyAsync(L->finished + slots[j], zeros, 4, hipMemcpyHostToDevice, st));
  }
  SMI_HIP(hipMemcpyAsync(L->rows, L->plan + tail, kMaxRows * sizeof(RowDesc), hipMemcpyDeviceToDevice, st));
  if (forked) {   // every take's history row gets its own prompt's ids
    std::vector<int64_t> eids((size_t)N * P_max);
    for (int j = 0; j < N; ++j) memcpy(&eids[(size_t)j * P_max], ids + (size_t)src[j] * P_max, (size_t)P_max * 8);
    if ((rc = pen_histories(L, eids.data(), lens_j, N, P_max, slots, st))) return rc;
  } else if ((rc = pen_histories(L, ids, lens, n, P_max, slots, st))) {
    return rc;
  }
  const std::vector<int> before = L->live_order;
  live_set(L, slots, N);   // the admission's step runs over the new rows alone
  if ((rc = launch_embed(L, L->rows, N, st)) || (rc = launch_step(L, N, st))) {
    live_set(L, before.data(), (int)before.size());
    L->lm_restrict = 0;
    return rc;
  }
  std::vector<RowDesc> fresh;
  if ((rc = session_live_rows(L, fresh, st))) return rc;
  int32_t len_j[kMaxRows];
  for (int j = 0; j < N; ++j) len_j[j] = lens_j[j] + 1;
  return slots_enter(L, live, slots, N, fresh.data(), lens_j, len_j, slots_out, st);
}

// The exported admissions: each is the next one with null for what it does not take (include/sparkmi.h).
int smi_llm_admit(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_sampled(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const smi_sample_params* params,
                          int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, nullptr, params}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_penalized(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const smi_sample_params* params,
                            const smi_penalty_params* pens, int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, nullptr, params, pens}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_logprobs(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const smi_sample_params* params,
                           const smi_penalty_params* pens, const int32_t* want_lp, int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, nullptr, params, pens, want_lp}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_forked(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const int32_t* n_ret,
                         const smi_sample_params* params, const smi_penalty_params* pens, const int32_t* want_lp, int32_t* slots_out,
                         void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, n_ret, params, pens, want_lp}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_constrained(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const int32_t* n_ret,
                              const smi_sample_params* params, const smi_penalty_params* pens, const int32_t* want_lp,
                              const smi_allow_params* allow, int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, n_ret, params, pens, want_lp, allow}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_biased(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const int32_t* n_ret,
                         const smi_sample_params* params, const smi_penalty_params* pens, const int32_t* want_lp,
                         const smi_allow_params* allow, const smi_seq_params* seq, int32_t* slots_out, void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, n_ret, params, pens, want_lp, allow, seq}, slots_out, (hipStream_t)stream);
}
int smi_llm_admit_ngram(smi_llm* L, const int64_t* ids, const int32_t* lens, int n, int P_max, const int32_t* n_ret,
                        const smi_sample_params* params, const smi_penalty_params* pens, const int32_t* want_lp,
                        const smi_allow_params* allow, const smi_seq_params* seq, const int32_t* no_repeat_ngram, int32_t* slots_out,
                        void* stream) {
  return admit(L, AdmitReq{ids, lens, n, P_max, n_ret, params, pens, want_lp, allow, seq, no_repeat_ngram}, slots_out, (hipStream_t)stream);
}

int smi_llm_retire(smi_llm* L, int slot, void* stream) {
  SMI_REQUIRE(L && slot >= 0 && slot < kMaxRows, "smi_llm_retire: bad argument");
  if (!L->started || !L->session) { smi_set_error("smi_llm_retire outside a session"); return SMI_ESTATE; }
  SMI_REQUIRE(L->slot_busy[slot], "smi_llm_retire: slot %d is not live", slot);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  std::vector<RowDesc> live;
  if ((rc = session_live_rows(L, live, st))) return rc;
  for (size_t i = 0; i < live.size(); ++i)
    if (live[i].slot == slot) { live.erase(live.begin() + (long)i); break; }
  L->slot_busy[slot] = 0;
  L->slot_len[slot] = 0;
  slot_clear(L, slot);
  if (L->paged) pages_release(L, slot);   // its pages go back to the pool (stale table entries are never read: no live row names the slot)
  if ((rc = allow_tiles_upload(L, st))) return rc;
  return session_set_rows(L, live, st);
}

// Several sequences leave at once, without a host round trip: the device row list is compacted in place (order kept), the
// per-row state of the rows that moved is rebuilt from their descriptors (as after any change of the live set), the slots
// (and their pages) are free again.  Their histories stay readable (smi_llm_slots_tokens) until a later admission reuses a slot.
int smi_llm_retire_many(smi_llm* L, const int32_t* slots, int n, void* stream) {
  SMI_REQUIRE(L && slots && n >= 1 && n <= kMaxRows, "smi_llm_retire_many: bad argument");
  if (!L->started || !L->session) { smi_set_error("smi_llm_retire_many outside a session"); return SMI_ESTATE; }
  unsigned long long drop = 0;
  for (int i = 0; i < n; ++i) {
    SMI_REQUIRE(slots[i] >= 0 && slots[i] < kMaxRows && L->slot_busy[slots[i]] && !((drop >> slots[i]) & 1ull), "smi_llm_retire_many: slot %d is not live (or listed twice)", slots[i]);
    drop |= 1ull << slots[i];
  }
  SMI_REQUIRE((int)L->live_order.size() == L->B, "smi_llm_retire_many: live row list out of step");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rows_drop, dim3(1), dim3(64), 0, st, L->rows, L->B, drop);
  SMI_LAUNCH_CHECK();
  std::vector<int> keep;
  for (int sl : L->live_order) if (!((drop >> sl) & 1ull)) keep.push_back(sl);
  for (int i = 0; i < n; ++i) {
    L->slot_busy[slots[i]] = 0;
    L->slot_len[slots[i]] = 0;
    slot_clear(L, slots[i]);
    if (L->paged) pages_release(L, slots[i]);
  }
  live_set(L, keep.data(), (int)keep.size());
  { const int rct = allow_tiles_upload(L, st); if (rct) return rct; }
  if (L->B == 0) return SMI_OK;
  return launch_embed(L, L->rows, L->B, st);
}

// ---- park and resume: a sequence leaves its KV slot as a blob in caller-owned device memory and comes back later, into any
// free slot (include/sparkmi.h; the blob's layout is at BlobHdr) ----
static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
// Where the parts of a blob lie, from what its header says: a sequence of `len` cache positions (len - 1 of them written),
// prompt length plen, feature byte feat.  Part offsets in bytes (0: absent).
struct BlobLay { size_t hdr, kv, hist, lp, phist, pctx, total; int npos, nhist, npctx; };
static BlobLay blob_layout(const smi_llm* L, int len, int plen, unsigned feat) {
  BlobLay b;
  memset(&b, 0, sizeof(b));
  b.npos = len - 1;
  b.nhist = len - plen < L->max_steps ? len - plen : L->max_steps;
  b.npctx = (feat & F_NGRAM) ? plen : 0;
  b.hdr = sizeof(BlobHdr) + ((feat & (F_BIAS | F_STOP)) ? sizeof(SeqRec) : 0);
  const size_t pos_bytes = (size_t)L->cfg.num_layers * 2 * L->cfg.num_kv_heads * kHeadDim * (L->cfg.kv_dtype ? 4 : 2);
  size_t o = b.hdr;
  b.kv = o; o += (size_t)b.npos * pos_bytes;
  b.hist = o; o += up16((size_t)b.nhist * 8);
  if (feat & F_LP) { b.lp = o; o += up16((size_t)b.nhist * 4); }
  if (feat & F_PEN) { b.phist = o; o += up16((size_t)L->cfg.vocab_size * 2); }
  if (feat & F_NGRAM) { b.pctx = o; o += up16((size_t)b.npctx * 4); }
  b.total = o;
  return b;
}
static SlotXfer blob_xfer(const BlobLay& b, void* blob, int slot) {
  SlotXfer x;
  memset(&x, 0, sizeof(x));
  x.blob = (unsigned char*)blob; x.slot = slot; x.npos = b.npos; x.nhist = b.nhist; x.npctx = b.npctx;
  x.o_kv = (uint32_t)(b.kv >> 4); x.o_hist = (uint32_t)(b.hist >> 4); x.o_lp = (uint32_t)(b.lp >> 4);
  x.o_phist = (uint32_t)(b.phist >> 4); x.o_pctx = (uint32_t)(b.pctx >> 4);
  return x;
}
// the feature byte a record set gives (admit builds the same bits record by record)
static unsigned recs_feat(const BlobHdr& h, const SeqRec* q) {
  return (h.samp.mode == SMI_SAMPLING_SAMPLE ? F_SAMPLE : 0) | (h.pen.on ? F_PEN : 0) | (h.lp ? F_LP : 0) | (h.allow.n > 0 ? F_ALLOW : 0) |
         (h.ngram > 0 ? F_NGRAM : 0) | (q && q->n_bias > 0 ? F_BIAS : 0) | (q && q->n_stop > 0 ? F_STOP : 0);
}
// The header's checksum: its host-written bytes (`check` and the kernel-written `dev` as zero) and the SeqRec behind it.
static uint64_t blob_check(const unsigned char* hdr, size_t hdr_bytes) {
  BlobHdr h;
  memcpy(&h, hdr, sizeof(h));
  h.check = 0;
  memset(&h.dev, 0, sizeof(h.dev));
  return fnv1a(hdr + sizeof(BlobHdr), hdr_bytes - sizeof(BlobHdr), fnv1a(&h, sizeof(h)));
}
// the two launches of a save (SAVE) or restore over the listed slots; every bound comes from host-checked values
static int park_launch(smi_llm* L, bool save, const SlotXfer* xs, int n, hipStream_t st) {
  ParkP p;
  memset(&p, 0, sizeof(p));
  int npos = 0, items = 1;
  const int V = L->cfg.vocab_size;
  for (int i = 0; i < n; ++i) {
    p.s[i] = xs[i];
    npos = xs[i].npos > npos ? xs[i].npos : npos;
    const int ph = xs[i].o_phist ? ((V & 7) ? V : V >> 3) : 0;
    const int m = xs[i].nhist > ph ? (xs[i].nhist > xs[i].npctx ? xs[i].nhist : xs[i].npctx) : (ph > xs[i].npctx ? ph : xs[i].npctx);
    items = m > items ? m : items;
  }
  p.kcache = (unsigned char*)L->kcache.get(); p.vcache = (unsigned char*)L->vcache.get();
  p.piece_shift = L->cfg.kv_dtype ? 4 : 3;
  p.layer_bytes = L->kv_layer_elems * (L->cfg.kv_dtype ? 4 : 2);
  p.n_kv = L->cfg.num_kv_heads; p.max_pos = L->cfg.max_positions;
  p.km = kv_map(L);
  p.rows = L->rows; p.B = L->B;
  p.hist = L->hist; p.lp = L->lp; p.phist = L->phist; p.pctx = L->pctx; p.count = L->count; p.finished = L->finished;
  p.V = V;
  if (npos > 0) {
    const unsigned per = 256 * kParkPieces;
    const dim3 grid((unsigned)((((size_t)npos << p.piece_shift) + per - 1) / per), (unsigned)n, (unsigned)(L->cfg.num_layers * 2 * L->cfg.num_kv_heads));
    if (save) hipLaunchKernelGGL(k_slot_kv<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_slot_kv<false>, grid, dim3(256), 0, st, p);
    SMI_LAUNCH_CHECK();
  }
  const int bx = (items + 255) / 256;
  const dim3 cgrid((unsigned)(bx < 64 ? bx : 64), (unsigned)n);
  if (save) hipLaunchKernelGGL(k_slot_cols<true>, cgrid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(k_slot_cols<false>, cgrid, dim3(256), 0, st, p);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}
static int park_state(const smi_llm* L, const char* who) {
  if (!L->started || !L->session) { smi_set_error("%s outside a session (smi_llm_session_begin first)", who); return SMI_ESTATE; }
  return SMI_OK;
}

int smi_llm_slot_blob_bytes(smi_llm* L, int slot, size_t* bytes) {
  SMI_REQUIRE(L && bytes, "smi_llm_slot_blob_bytes: null argument");
  { const int rcs = park_state(L, "smi_llm_slot_blob_bytes"); if (rcs) return rcs; }
  SMI_REQUIRE(slot >= 0 && slot < kMaxRows && L->slot_busy[slot], "smi_llm_slot_blob_bytes: slot %d is not busy", slot);
  *bytes = blob_layout(L, L->slot_len[slot], L->slot_plen[slot], L->slot_feat[slot]).total;
  return SMI_OK;
}

int smi_llm_slots_save(smi_llm* L, const int32_t* slots, int n, void* const* blobs_dev, const size_t* caps, size_t* used, void* stream) {
  SMI_REQUIRE(L && slots && blobs_dev && caps && used && n >= 1 && n <= kMaxRows, "smi_llm_slots_save: bad argument");
  { const int rcs = park_state(L, "smi_llm_slots_save"); if (rcs) return rcs; }
  SMI_REQUIRE((int)L->live_order.size() == L->B, "smi_llm_slots_save: live row list out of step");
  unsigned long long seen = 0;
  BlobLay lay[kMaxRows];
  size_t stage = 0;
  for (int i = 0; i < n; ++i) {   // every check before the first byte is written
    const int sl = slots[i];
    SMI_REQUIRE(sl >= 0 && sl < kMaxRows && L->slot_busy[sl] && !((seen >> sl) & 1ull), "smi_llm_slots_save: slot %d is not busy (or listed twice)", sl);
    seen |= 1ull << sl;
    lay[i] = blob_layout(L, L->slot_len[sl], L->slot_plen[sl], L->slot_feat[sl]);
    SMI_REQUIRE(blobs_dev[i] && ((uintptr_t)blobs_dev[i] & 15) == 0, "smi_llm_slots_save: blobs_dev[%d] must be a 16-byte aligned device address", i);
    SMI_REQUIRE(caps[i] >= lay[i].total, "smi_llm_slots_save: caps[%d]=%zu, the sequence in slot %d needs %zu bytes", i, caps[i], sl, lay[i].total);
    stage += lay[i].hdr;
  }
  hipStream_t st = (hipStream_t)stream;
  L->host_blob.assign(stage, 0);
  SlotXfer xs[kMaxRows];
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = slots[i];
    unsigned char* hb = L->host_blob.data() + at;
    BlobHdr h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "SMISLOT1", 8);
    h.hdr_bytes = (uint32_t)lay[i].hdr; h.feat = L->slot_feat[sl]; h.total_bytes = lay[i].total;
    h.cfg_stamp = fnv1a(&L->cfg, sizeof(L->cfg)); h.handle_id = L->handle_id; h.session_gen = L->session_gen;
    h.len = L->slot_len[sl]; h.plen = L->slot_plen[sl]; h.nhist = lay[i].nhist; h.seqid = L->hctl.seqid[sl];
    h.samp = L->hctl.samp[sl]; h.pen = L->hctl.pen[sl]; h.lp = L->hctl.lp[sl]; h.ngram = L->hctl.ngram[sl]; h.ngplen = L->hctl.ngplen[sl];
    h.allow = L->hctl.allow[sl];
    memcpy(hb, &h, sizeof(h));
    if (lay[i].hdr > sizeof(BlobHdr)) memcpy(hb + sizeof(BlobHdr), &L->hseq[(size_t)sl], sizeof(SeqRec));
    h.check = blob_check(hb, lay[i].hdr);
    memcpy(hb, &h, sizeof(h));
    // (pageable source: staged before the call returns; host_blob is rebuilt only by the next save)
    SMI_HIP(hipMemcpyAsync(blobs_dev[i], hb, lay[i].hdr, hipMemcpyHostToDevice, st));
    xs[i] = blob_xfer(lay[i], blobs_dev[i], sl);
    used[i] = lay[i].total;
    at += lay[i].hdr;
  }
  return park_launch(L, true, xs, n, st);
}

int smi_llm_slots_restore(smi_llm* L, const void* const* blobs_dev, const size_t* bytes, int n, int32_t* slots_out, void* stream) {
  SMI_REQUIRE(L && blobs_dev && bytes && slots_out && n >= 1 && n <= kMaxRows, "smi_llm_slots_restore: bad argument");
  { const int rcs = park_state(L, "smi_llm_slots_restore"); if (rcs) return rcs; }
  hipStream_t st = (hipStream_t)stream;
  const size_t hmax = sizeof(BlobHdr) + sizeof(SeqRec);
  for (int i = 0; i < n; ++i) {
    SMI_REQUIRE(blobs_dev[i] && ((uintptr_t)blobs_dev[i] & 15) == 0, "smi_llm_slots_restore: blobs_dev[%d] must be a 16-byte aligned device address", i);
    SMI_REQUIRE(bytes[i] >= sizeof(BlobHdr), "smi_llm_slots_restore: blob %d is truncated (%zu bytes)", i, bytes[i]);
  }
  std::vector<unsigned char> hh((size_t)n * hmax, 0);
  for (int i = 0; i < n; ++i)
    SMI_HIP(hipMemcpyAsync(hh.data() + (size_t)i * hmax, blobs_dev[i], bytes[i] < hmax ? bytes[i] : hmax, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  // every blob is checked before anything of the handle is touched
  BlobLay lay[kMaxRows];
  const uint64_t stamp = fnv1a(&L->cfg, sizeof(L->cfg));
  for (int i = 0; i < n; ++i) {
    const unsigned char* hb = hh.data() + (size_t)i * hmax;
    BlobHdr h;
    memcpy(&h, hb, sizeof(h));
    SMI_REQUIRE(memcmp(h.magic, "SMISLOT1", 8) == 0, "smi_llm_slots_restore: blob %d is not a sequence snapshot", i);
    SMI_REQUIRE((h.hdr_bytes == sizeof(BlobHdr) || h.hdr_bytes == hmax) && h.hdr_bytes <= bytes[i] && h.feat < (1u << kFeatBits) &&
                (h.hdr_bytes == hmax) == ((h.feat & (F_BIAS | F_STOP)) != 0), "smi_llm_slots_restore: blob %d has a corrupt header", i);
    SMI_REQUIRE(h.check == blob_check(hb, h.hdr_bytes), "smi_llm_slots_restore: blob %d has a corrupt header (checksum)", i);
    if (h.cfg_stamp != stamp) { smi_set_error("smi_llm_slots_restore: blob %d was saved under another configuration", i); return SMI_ESTATE; }
    if (h.handle_id != L->handle_id || h.session_gen != L->session_gen) {
      smi_set_error("smi_llm_slots_restore: blob %d is of another handle or an earlier session of this one", i);
      return SMI_ESTATE;
    }
    SMI_REQUIRE(h.plen >= 1 && h.len > h.plen && h.len <= L->cfg.max_positions, "smi_llm_slots_restore: blob %d has corrupt lengths", i);
    lay[i] = blob_layout(L, h.len, h.plen, h.feat);
    SMI_REQUIRE(lay[i].total == h.total_bytes && h.nhist == lay[i].nhist, "smi_llm_slots_restore: blob %d has a corrupt header (sizes)", i);
    SMI_REQUIRE(bytes[i] == lay[i].total, "smi_llm_slots_restore: blob %d is %zu bytes, its header says %zu", i, bytes[i], lay[i].total);
    const SeqRec* q = h.hdr_bytes == hmax ? (const SeqRec*)(hb + sizeof(BlobHdr)) : nullptr;
    SMI_REQUIRE(recs_feat(h, q) == h.feat && h.ngplen == ((h.feat & F_NGRAM) ? h.plen : 0) && (!q || q->plen == h.plen),
                "smi_llm_slots_restore: blob %d: records and feature byte disagree", i);
    SMI_REQUIRE(h.dev.row.pos == h.len - 1 && h.dev.row.flags == h.len - h.plen && h.dev.row.token >= 0 && h.dev.row.token < L->cfg.vocab_size &&
                h.dev.count >= 0 && h.dev.count <= h.dev.row.flags && (h.dev.finished == 0 || h.dev.finished == 1),
                "smi_llm_slots_restore: blob %d has a corrupt row state", i);
  }
  int32_t slots[kMaxRows];   // lowest free first, as an admission takes them
  { const int k = slots_take_free(L, n, slots);
    if (k < n) { smi_set_error("smi_llm_slots_restore: %d snapshots, %d free KV slots", n, k); return SMI_ESTATE; } }
  // what the headers say, as the shared admission steps take it: the records (the sequence keeps its admission number;
  // admit_seq does not move), the bias / stop records, the rows, the lengths
  SlotRecs old[kMaxRows], recs[kMaxRows];
  std::vector<SeqRec> seqs((size_t)n);
  RowDesc rows[kMaxRows];
  int32_t lens[kMaxRows], plens[kMaxRows];
  SlotXfer xs[kMaxRows];
  for (int i = 0; i < n; ++i) {
    const unsigned char* hb = hh.data() + (size_t)i * hmax;
    BlobHdr h;
    memcpy(&h, hb, sizeof(h));
    recs[i] = SlotRecs{h.seqid, h.samp, h.pen, h.lp, h.allow, h.ngram, h.ngplen, (uint8_t)h.feat};
    memset(&seqs[(size_t)i], 0, sizeof(SeqRec));
    if (h.hdr_bytes == hmax) memcpy(&seqs[(size_t)i], hb + sizeof(BlobHdr), sizeof(SeqRec));
    rows[i] = h.dev.row;
    rows[i].slot = slots[i];
    lens[i] = h.len; plens[i] = h.plen;
    xs[i] = blob_xfer(lay[i], const_cast<void*>(blobs_dev[i]), slots[i]);
  }
  int rc;
  std::vector<RowDesc> live;
  if ((rc = session_live_rows(L, live, st))) return rc;
  // pages of its own, whatever the original shared; all or nothing: a short pool restores nobody (the slots hold no page yet)
  if (L->paged && (rc = pages_ensure(L, slots, lens, n, st))) return rc;
  if ((rc = recs_install(L, "smi_llm_slots_restore", slots, n, recs, seqs.data(), old, st)) || (rc = park_launch(L, false, xs, n, st))) {
    recs_withdraw(L, slots, n, old);
    return rc;
  }
  return slots_enter(L, live, slots, n, rows, plens, lens, slots_out, st);
}

// Tokens of several slots in one device round trip: out_host [n][cap], n_out[n], finished[n].
int smi_llm_slots_tokens(smi_llm* L, const int32_t* slots, int n, int64_t* out_host, int cap, int32_t* n_out, int32_t* finished, void* stream) {
  SMI_REQUIRE(L && slots && out_host && n_out && finished && n >= 1 && n <= kMaxRows && cap >= 1, "smi_llm_slots_tokens: bad argument");
  for (int i = 0; i < n; ++i) SMI_REQUIRE(slots[i] >= 0 && slots[i] < kMaxRows, "smi_llm_slots_tokens: slot %d out of range", slots[i]);
  hipStream_t st = (hipStream_t)stream;
  int32_t cnt[kMaxRows], fin[kMaxRows];
  SMI_HIP(hipMemcpyAsync(cnt, L->count, kMaxRows * 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipMemcpyAsync(fin, L->finished, kMaxRows * 4, hipMemcpyDeviceToHost, st));
  int steps = cap < L->max_steps ? cap : L->max_steps;
  std::vector<int64_t> hist((size_t)steps * kMaxRows);
  SMI_HIP(hipMemcpyAsync(hist.data(), L->hist, hist.size() * 8, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    int k = cnt[slots[i]] < steps ? cnt[slots[i]] : steps;
    for (int t = 0; t < k; ++t) out_host[(size_t)i * cap + t] = hist[(size_t)t * kMaxRows + slots[i]];
    n_out[i] = k;
    finished[i] = fin[slots[i]];
  }
  return SMI_OK;
}

// The tokens the listed slots have emitted since from[i], at most cap each, in one small round trip (include/sparkmi.h): k_poll
// packs them, one copy of n * (8 + 8 * cap) bytes brings them to the pinned buffer.  Launched on the caller's stream between
// decode calls -- never inside the captured step.
int smi_llm_poll(smi_llm* L, const int32_t* slots, const int32_t* from, int n, int64_t* out_host, int cap, int32_t* n_out,
                 int32_t* count, int32_t* finished, void* stream) {
  SMI_REQUIRE(L && slots && from && out_host && n_out && count && finished && n >= 1 && n <= kMaxRows && cap >= 1, "smi_llm_poll: bad argument");
  for (int i = 0; i < n; ++i) {
    SMI_REQUIRE(slots[i] >= 0 && slots[i] < kMaxRows, "smi_llm_poll: slot %d out of range", slots[i]);
    SMI_REQUIRE(from[i] >= 0, "smi_llm_poll: from[%d]=%d < 0", i, from[i]);
  }
  hipStream_t st = (hipStream_t)stream;
  const int capd = cap < L->max_steps ? cap : L->max_steps;   // no sequence has more history than that
  PollArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n; ++i) { a.slot[i] = slots[i]; a.from[i] = from[i] < L->max_steps ? from[i] : L->max_steps; }
  hipLaunchKernelGGL(k_poll, dim3(n), dim3(64), 0, st, L->hist, L->count, L->finished, L->max_steps, a, capd, L->poll_dev);
  SMI_LAUNCH_CHECK();
  SMI_HIP(hipMemcpyAsync(L->poll_host, L->poll_dev, (size_t)n * (8 + 8 * (size_t)capd), hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    const int64_t* rec = L->poll_host + (size_t)i * (1 + capd);
    int32_t head[2];
    memcpy(head, rec, 8);
    int end = head[0] < L->max_steps ? head[0] : L->max_steps;
    if (end - a.from[i] > capd) end = a.from[i] + capd;
    const int k = end > a.from[i] ? end - a.from[i] : 0;
    if (k) memcpy(out_host + (size_t)i * cap, rec + 1, (size_t)k * 8);
    n_out[i] = k;
    count[i] = head[0];
    finished[i] = head[1];
  }
  return SMI_OK;
}

// Log-probabilities of several slots in one device round trip: out_host [n][cap], n_out[n] (as smi_llm_slots_tokens).
int smi_llm_slots_logprobs(smi_llm* L, const int32_t* slots, int n, float* out_host, int cap, int32_t* n_out, void* stream) {
  SMI_REQUIRE(L && slots && out_host && n_out && n >= 1 && n <= kMaxRows && cap >= 1, "smi_llm_slots_logprobs: bad argument");
  for (int i = 0; i < n; ++i) SMI_REQUIRE(slots[i] >= 0 && slots[i] < kMaxRows, "smi_llm_slots_logprobs: slot %d out of range", slots[i]);
  for (int i = 0; i < n; ++i)
    if (!L->hctl.lp[slots[i]]) {
      smi_set_error("smi_llm_slots_logprobs: the sequence in slot %d was admitted without return_log_probs", slots[i]);
      return SMI_ESTATE;
    }
  hipStream_t st = (hipStream_t)stream;
  int32_t cnt[kMaxRows];
  SMI_HIP(hipMemcpyAsync(cnt, L->count, kMaxRows * 4, hipMemcpyDeviceToHost, st));
  int steps = cap < L->max_steps ? cap : L->max_steps;
  std::vector<float> lp((size_t)steps * kMaxRows);
  SMI_HIP(hipMemcpyAsync(lp.data(), L->lp, lp.size() * 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i) {
    int k = cnt[slots[i]] < steps ? cnt[slots[i]] : steps;
    for (int t = 0; t < k; ++t) out_host[(size_t)i * cap + t] = lp[(size_t)t * kMaxRows + slots[i]];
    n_out[i] = k;
  }
  return SMI_OK;
}

// Tokens a live (or just finished) slot has emitted since it was admitted; *finished: it has produced eos.
int smi_llm_slot_tokens(smi_llm* L, int slot, int64_t* out, int cap, int32_t* n_out, int32_t* finished, void* stream) {
  SMI_REQUIRE(L && out && n_out && finished && slot >= 0 && slot < kMaxRows && cap >= 0, "smi_llm_slot_tokens: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int32_t cnt = 0, fin = 0;
  SMI_HIP(hipMemcpyAsync(&cnt, L->count + slot, 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipMemcpyAsync(&fin, L->finished + slot, 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  int n = cnt < cap ? cnt : cap;
  if (n > L->max_steps) n = L->max_steps;
  if (n > 0) SMI_HIP(hipMemcpy2D(out, 8, L->hist + slot, kMaxRows * 8, 8, (size_t)n, hipMemcpyDeviceToHost));
  *n_out = n;
  *finished = fin;
  return SMI_OK;
}

// K back-to-back decode steps over the live rows, captured on a stream of its own and instantiated: *out, or null when the
// capture or the instantiation failed (the runtime's error state is cleared either way).
// Every sequence of the generation or session -- the busy slots -- and the cache positions each will have used after n_steps more
// steps; returns how many there are, *bound the largest of their lengths.
static int busy_after(const smi_llm* L, int n_steps, int* sl, int* len, int* bound) {
  int n = 0;
  *bound = 0;
  for (int s = 0; s < kMaxRows; ++s)
    if (L->slot_busy[s]) {
      sl[n] = s; len[n] = L->slot_len[s] + n_steps;
      *bound = len[n] > *bound ? len[n] : *bound;
      ++n;
    }
  return n;
}

static int capture_steps(smi_llm* L, int K, hipGraphExec_t* out) {
  *out = nullptr;
  hipStream_t cs;
  SMI_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    int rc = SMI_OK;
    for (int k = 0; k < K && rc == SMI_OK; ++k) rc = launch_step(L, L->B, cs);
    const hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc == SMI_OK && e == hipSuccess && g && hipGraphInstantiate(out, g, nullptr, nullptr, 0) != hipSuccess) *out = nullptr;
    if (g) (void)hipGraphDestroy(g);
  }
  (void)hipStreamDestroy(cs);
  (void)hipGetLastError();
  return SMI_OK;
}

int smi_llm_decode(smi_llm* L, int n_steps, void* stream) {
  SMI_REQUIRE(L, "smi_llm_decode: null handle");
  if (!L->started) { smi_set_error("smi_llm_decode before smi_llm_prefill"); return SMI_ESTATE; }
  SMI_REQUIRE(n_steps >= 0, "smi_llm_decode: n_steps < 0");
  if (L->B == 0 || n_steps == 0) return SMI_OK;
  int sl[kMaxRows], need[kMaxRows], bound = 0;
  const int n = busy_after(L, n_steps, sl, need, &bound);
  for (int i = 0; i < n; ++i)
    SMI_REQUIRE(need[i] <= L->cfg.max_positions, "smi_llm_decode: %d more steps would take slot %d past max_positions=%d", n_steps, sl[i],
                L->cfg.max_positions);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = pages_ensure(L, sl, need, n, st))) return rc;   // paged cache: the pages of those positions first, all or nothing
  // context bound of this call -> attention segments (the partial buffer must exist before a capture starts)
  L->attn_seg = segs_for(bound);
  if (L->attn_seg > 1 && (rc = ensure_apart(L, (size_t)kMaxRows * L->cfg.num_heads * L->attn_seg * 66))) return rc;
  const unsigned feat = step_feat(L);
  if (L->cfg.use_graph) {
    const uint64_t key = graph_key(L, feat, 0);
    if (!L->graph || L->graph_id != key) {
      auto hit = L->graph_cache.find(key);
      L->graph = hit != L->graph_cache.end() ? hit->second : nullptr;
      L->graph_id = key;
    }
    if (!L->graph) {
      if (L->graph_cache.size() >= 192) graphs_flush(L);
      if ((rc = capture_steps(L, 1, &L->graph))) return rc;
      if (!L->graph) { smi_set_error("hipGraph capture of the decode step failed"); return SMI_EHIP; }
      L->graph_cache[key] = L->graph;
    }
  }
  // Several steps per replay (K = kGraphSteps): the call replays the K-step graph n_steps / K times and the one-step graph for the
  // rest.  The K-step graph of a key is only built by a call long enough to replay it twice (a capture of 8 x 98 nodes is not
  // free; short serving strides keep to the one-step graph); a failed capture leaves the call to the one-step graph.
  int s0 = 0;
  if (L->cfg.use_graph && n_steps >= kGraphSteps) {
    constexpr int K = kGraphSteps;
    const uint64_t keyk = graph_key(L, feat, K);
    hipGraphExec_t gk = nullptr;
    auto hit = L->graph_cache.find(keyk);
    if (hit != L->graph_cache.end()) gk = hit->second;
    else if (n_steps >= 2 * K && L->graph_cache.size() < 192) {
      if ((rc = capture_steps(L, K, &gk))) return rc;
      if (gk) L->graph_cache[keyk] = gk;
    }
    for (; gk && s0 + K <= n_steps; s0 += K) {
      SMI_HIP(hipGraphLaunch(gk, st));
      L->graph_last[gk] = st;
    }
  }
  for (int s = s0; s < n_steps; ++s) {
    if (L->cfg.use_graph) {
      SMI_HIP(hipGraphLaunch(L->graph, st));
      L->graph_last[L->graph] = st;
    } else if ((rc = launch_step(L, L->B, st))) {
      return rc;
    }
  }
  for (int i = 0; i < n; ++i) L->slot_len[sl[i]] = need[i];
  return SMI_OK;
}

int smi_llm_all_done(smi_llm* L, int* all_done, void* stream) {
  SMI_REQUIRE(L && all_done, "smi_llm_all_done: null argument");
  int32_t fin[kMaxRows];
  SMI_HIP(hipMemcpyAsync(fin, L->finished, sizeof(fin), hipMemcpyDeviceToHost, (hipStream_t)stream));
  SMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  { const int rce = eng_check(L); if (rce) return rce; }
  int d = 1;
  for (int b = 0; b < L->B; ++b) d &= fin[b] != 0;
  *all_done = d;
  return SMI_OK;
}

// Tokens emitted and eos flags of every KV slot in one round trip (continuous-batching drivers poll this every few steps)
int smi_llm_status(smi_llm* L, int32_t* count_host, int32_t* finished_host, void* stream) {
  SMI_REQUIRE(L && count_host && finished_host, "smi_llm_status: null argument");
  hipStream_t st = (hipStream_t)stream;
  SMI_HIP(hipMemcpyAsync(count_host, L->count, kMaxRows * 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipMemcpyAsync(finished_host, L->finished, kMaxRows * 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  return eng_check(L);
}

int smi_llm_steps(smi_llm* L) {
  if (!L) return SMI_EINVAL;
  int32_t s = 0;
  if (hipMemcpy(&s, L->step, 4, hipMemcpyDeviceToHost) != hipSuccess) return SMI_EHIP;
  return s;
}

int smi_llm_kv_pages(smi_llm* L, int32_t* total, int32_t* free_pages) {
  SMI_REQUIRE(L && total && free_pages, "smi_llm_kv_pages: null argument");
  *total = L->paged ? L->cfg.kv_pages : 0;
  *free_pages = L->paged ? (int32_t)L->free_pages.size() : 0;
  return SMI_OK;
}

int smi_llm_get_tokens(smi_llm* L, int64_t* out, int32_t* lens, int cap, void* stream) {
  SMI_REQUIRE(L && out && lens && cap >= 0, "smi_llm_get_tokens: bad argument");
  hipStream_t st = (hipStream_t)stream;
  int32_t cnt[kMaxRows], step = 0;
  SMI_HIP(hipMemcpyAsync(cnt, L->count, sizeof(cnt), hipMemcpyDeviceToHost, st));
  SMI_HIP(hipMemcpyAsync(&step, L->step, 4, hipMemcpyDeviceToHost, st));
  SMI_HIP(hipStreamSynchronize(st));
  { const int rce = eng_check(L); if (rce) return rce; }
  if (step > L->max_steps) step = L->max_steps;
  std::vector<int64_t> hist((size_t)step * kMaxRows);
  if (step) SMI_HIP(hipMemcpy(hist.data(), L->hist, hist.size() * 8, hipMemcpyDeviceToHost));
  for (int b = 0; b < L->B; ++b) {
    int n = cnt[b] < cap ? cnt[b] : cap;
    if (n > step) n = step;
    lens[b] = n;
    for (int s = 0; s < n; ++s) out[(size_t)b * cap + s] = hist[(size_t)s * kMaxRows + b];
  }
  return SMI_OK;
}

int smi_llm_forward_logits(smi_llm* L, const int64_t* ids, int S, float* logits_dev, void* stream) {
  SMI_REQUIRE(L && ids && logits_dev, "smi_llm_forward_logits: null argument");
  SMI_REQUIRE(S >= 1 && S < L->cfg.max_positions, "smi_llm_forward_logits: S=%d outside 1..max_positions-1", S);
  hipStream_t st = (hipStream_t)stream;
  const size_t nchunks = ((size_t)S + kMaxRows - 1) / kMaxRows;
  int rc;
  L->attn_seg = segs_for(S);
  if (L->paged) {
    for (int b = 0; b < kMaxRows; ++b) pages_release(L, b);
    const int s0 = 0;
    if ((rc = pages_ensure(L, &s0, &S, 1, st))) return rc;
  }
  if ((rc = ensure_plan(L, nchunks * kMaxRows))) return rc;
  L->host_rows.assign(nchunks * kMaxRows, RowDesc{0, 0, 0, 0});
  for (int t = 0; t < S; ++t) {
    SMI_REQUIRE(ids[t] >= 0 && ids[t] < L->cfg.vocab_size, "smi_llm_forward_logits: token id out of range");
    L->host_rows[t] = RowDesc{0, t, (int32_t)ids[t], 1};
  }
  SMI_HIP(hipMemcpyAsync(L->plan, L->host_rows.data(), L->host_rows.size() * sizeof(RowDesc), hipMemcpyHostToDevice, st));
  for (size_t c = 0; c < nchunks; ++c) {
    const int M = (int)(((size_t)S - c * kMaxRows) < (size_t)kMaxRows ? ((size_t)S - c * kMaxRows) : kMaxRows);
    const RowDesc* rows = L->plan + c * kMaxRows;
    if ((rc = launch_embed(L, rows, M, st))) return rc;
    if ((rc = launch_layers(L, rows, M, false, st))) return rc;
    if ((rc = launch_one(L, KLM, 0, rows, M, logits_dev + c * kMaxRows * (size_t)L->cfg.vocab_size, st))) return rc;
  }
  L->started = 0;  // the cache now holds this sequence; a generate must prefill again
  return SMI_OK;
}

#ifdef SMI_DIAG   // ---- everything below: include/sparkmi_debug.h, exported by libsparkmi_diag.so only
// Diagnostics: one launch of a decode-step GEMM kernel with in-kernel s_memrealtime stamps
// (10 ns ticks); out[0..7) = mean over blocks of (stamp i - earliest stamp 0), out[7] = blocks.
int smi_llm_debug_stamps(smi_llm* L, int kernel, int layer, double* out) {
  SMI_REQUIRE(L && out && L->started, "smi_llm_debug_stamps: needs a started generation");
  // kernel + 32: the layer's earlier kernels run first (un-stamped, with their helper blocks), so the stamped kernel finds in
  // the caches what it finds inside a decode step -- the in-kernel evidence for (or against) the helpers' prefetch
  const bool with_producers = (kernel & 32) != 0;
  kernel &= 31;
  SMI_REQUIRE(kernel == KQKV || kernel == KO || kernel == KGU || kernel == KD || kernel == KLM, "smi_llm_debug_stamps: GEMM kernels only");
  SMI_REQUIRE(!(kernel == KLM && L->B <= 16 && L->KTh <= 32), "smi_llm_debug_stamps: the persistent lm_head has no stamps");
  SMI_HIP(hipMemset(L->stamps, 0, (size_t)4096 * 64));
  graphs_flush(L);   // (the stamped kernels are other instantiations)
  int rc = SMI_OK;
  if (with_producers) {
    if (layer > 0) rc = launch_one(L, KD, layer - 1, L->rows, L->B, nullptr, 0);   // (its helpers warm this layer's QKV / o_proj slices)
    for (int k = KQKV; k < kernel && rc == SMI_OK; ++k) rc = launch_one(L, k, layer, L->rows, L->B, nullptr, 0);
    if (rc) return rc;
  }
  L->stamps_on = 1;
  rc = launch_one(L, kernel, layer, L->rows, L->B, nullptr, 0);
  L->stamps_on = 0;
  if (rc) return rc;
  SMI_HIP(hipDeviceSynchronize());
  // the launch's grid depends on the row count: the blocks that ran are the ones that left an entry stamp
  std::vector<unsigned long long> h((size_t)4096 * 8);
  SMI_HIP(hipMemcpy(h.data(), L->stamps, h.size() * 8, hipMemcpyDeviceToHost));
  int nblk = 0;
  while (nblk < 4096 && h[(size_t)nblk * 8]) ++nblk;
  SMI_REQUIRE(nblk > 0, "smi_llm_debug_stamps: the kernel left no stamps");
  unsigned long long t0 = ~0ull;
  for (int b = 0; b < nblk; ++b) t0 = h[(size_t)b * 8] < t0 ? h[(size_t)b * 8] : t0;
  for (int i = 0; i < 7; ++i) {
    double s = 0;
    for (int b = 0; b < nblk; ++b) s += (double)(h[(size_t)b * 8 + i] - t0);
    out[i] = s / nblk * 0.01;   // microseconds
  }
  double cyc = 0, us = 0;   // shader clock during the kernel: cycles / (stamp6 - stamp0)
  for (int b = 0; b < nblk; ++b) { cyc += (double)h[(size_t)b * 8 + 7]; us += (double)(h[(size_t)b * 8 + 6] - h[(size_t)b * 8]) * 0.01; }
  out[7] = us > 0 ? cyc / us : 0;   // MHz
  return SMI_OK;
}

int smi_llm_time_kernel(smi_llm* L, int kernel, int layer, int iters, float* ms_avg, void* stream) {
  SMI_REQUIRE(L && ms_avg && iters > 0, "smi_llm_time_kernel: bad argument");
  SMI_REQUIRE((kernel >= 0 && kernel <= 8) || (kernel >= 16 && kernel <= 16 + KD), "smi_llm_time_kernel: kernel id %d", kernel);
  if (!L->started) { smi_set_error("smi_llm_time_kernel needs a started generation (prefill first)"); return SMI_ESTATE; }
  if (L->paged && kernel != 7) { smi_set_error("smi_llm_time_kernel: the per-kernel probes need a contiguous KV cache (kv_page_tokens = 0)"); return SMI_ESTATE; }
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (kernel == 8) {
    // all layers of one step for the live rows: ONE launch of the one-row engine where it applies, else the layer kernels
    // back to back (each launch takes the previous one's residual row as its input: the values drift, the timing does not)
    const bool eng = eng_usable(L, L->rows, L->B);
    if ((rc = eng ? eng_launch(L, st) : launch_layers(L, L->rows, L->B, false, st))) return rc;
    SMI_HIP(hipEventRecord(L->ev0, st));
    for (int i = 0; i < iters; ++i)
      if ((rc = eng ? eng_launch(L, st) : launch_layers(L, L->rows, L->B, false, st))) return rc;
    SMI_HIP(hipEventRecord(L->ev1, st));
    L->started = 0;   // the residual row no longer belongs to the generation
  } else if (kernel == 7) {
    if ((rc = smi_llm_decode(L, 1, stream))) return rc;  // builds the graph if needed
    SMI_HIP(hipEventRecord(L->ev0, st));
    if ((rc = smi_llm_decode(L, iters, stream))) return rc;
    SMI_HIP(hipEventRecord(L->ev1, st));
  } else if (kernel >= 16) {
    // In-sequence cost of one layer kernel: (time of iters layers) - (time of the same layers without it).
    // Its producers run, so what they leave in L2 (the helper prefetch) is what it finds -- the
    // duration it has inside the decode graph, which the back-to-back loop below cannot show.
    const int k = kernel - 16, nl = L->cfg.num_layers;
    SMI_REQUIRE(k >= KQKV && k <= KD, "smi_llm_time_kernel: in-sequence timing is for the layer kernels");
    // both sequences are captured into hipGraphs and replayed, like the decode step itself: eager launches of
    // 5-us kernels can be bound by the host's launch rate, which would then be what the difference measures
    float t[2] = {0.f, 0.f};
    for (int pass = 0; pass < 2; ++pass) {
      hipStream_t cs;
      SMI_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
      hipGraph_t g = nullptr;
      hipGraphExec_t ge = nullptr;
      rc = SMI_OK;
      hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
      if (e == hipSuccess) {
        for (int i = 0; i < iters && rc == SMI_OK; ++i) {
          const int l = (layer + i) % nl;
          for (int kk = KQKV; kk <= KD && rc == SMI_OK; ++kk)
            if (!(pass == 1 && kk == k)) rc = launch_one(L, kk, l, L->rows, L->B, nullptr, cs);
        }
        e = hipStreamEndCapture(cs, &g);
      }
      if (e == hipSuccess && rc == SMI_OK && g) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
      if (g) (void)hipGraphDestroy(g);
      (void)hipStreamDestroy(cs);
      if (e != hipSuccess || rc != SMI_OK || !ge) {
        if (ge) (void)hipGraphExecDestroy(ge);
        (void)hipGetLastError();
        if (rc != SMI_OK) return rc;
        smi_set_error("smi_llm_time_kernel: graph capture of the layer sequence failed");
        return SMI_EHIP;
      }
      hipError_t le = hipGraphLaunch(ge, st);                       // warm (also brings the L2 / MALL into steady state)
      if (le == hipSuccess) le = hipEventRecord(L->ev0, st);
      if (le == hipSuccess) le = hipGraphLaunch(ge, st);
      if (le == hipSuccess) le = hipEventRecord(L->ev1, st);
      if (le == hipSuccess) le = hipEventSynchronize(L->ev1);
      if (le == hipSuccess) le = hipEventElapsedTime(&t[pass], L->ev0, L->ev1);
      (void)hipGraphExecDestroy(ge);
      if (le != hipSuccess) { smi_set_error("smi_llm_time_kernel: graph replay failed: %s", hipGetErrorString(le)); return SMI_EHIP; }
    }
    *ms_avg = (t[0] - t[1]) / iters;
    return SMI_OK;
  } else {
    const int nl = L->cfg.num_layers;
    if (kernel == KFIN) {
      int sl[kMaxRows], len[kMaxRows], bound = 0;
      const int n = busy_after(L, iters + 1, sl, len, &bound);
      SMI_REQUIRE(bound <= L->cfg.max_positions, "smi_llm_time_kernel: finalize probe would pass max_positions");
      for (int i = 0; i < n; ++i) L->slot_len[sl[i]] = len[i];
    }
    if ((rc = launch_one(L, kernel, layer % nl, L->rows, L->B, nullptr, st))) return rc;
    SMI_HIP(hipEventRecord(L->ev0, st));
    for (int i = 0; i < iters; ++i) {
      // walk the layers so the weights come from HBM, not from the Infinity Cache
      const int l = kernel >= KLM ? 0 : (layer + 1 + i) % nl;
      if ((rc = launch_one(L, kernel, l, L->rows, L->B, nullptr, st))) return rc;
    }
    SMI_HIP(hipEventRecord(L->ev1, st));
  }
  SMI_HIP(hipEventSynchronize(L->ev1));
  float ms = 0.f;
  SMI_HIP(hipEventElapsedTime(&ms, L->ev0, L->ev1));
  *ms_avg = ms / iters;
  return SMI_OK;
}

// ---- one-row decode engine (smi_eng.h)
int smi_llm_engine(smi_llm* L, int32_t* enabled, int32_t* info, char* why, int n) {
  SMI_REQUIRE(L, "smi_llm_engine: null handle");
  if (enabled) *enabled = L->eng.enabled && L->eng_on;
  if (info) { info[0] = L->eng.ncu; info[1] = L->eng.maxlen; info[2] = L->eng.lds; info[3] = L->eng.enabled; }
  if (why && n > 0) { strncpy(why, L->eng.why, (size_t)n - 1); why[n - 1] = 0; }
  return SMI_OK;
}

int smi_llm_set_engine(smi_llm* L, int on) {
  SMI_REQUIRE(L, "smi_llm_set_engine: null handle");
  int v = on ? 1 : 0;
  if (v && !L->eng.enabled) {   // first request: build it (plan, 0.8 GB weight stream); stays off, with the reason, where it does not apply
    SMI_HIP(hipDeviceSynchronize());
    const int rce = eng_create(L);
    if (rce) return rce;
    v = L->eng.enabled;
  }
  if (v != L->eng_on) { SMI_HIP(hipDeviceSynchronize()); graphs_flush(L); }   // captured steps hold one path or the other
  L->eng_on = v;
  return SMI_OK;
}

int smi_llm_engine_plan(const smi_llm_cfg* cfg, int ncu, int32_t* stats) {
  SMI_REQUIRE(cfg_ok(cfg) && stats, "smi_llm_engine_plan: invalid argument");
  EngPlanHost P;
  char why[128] = "";
  const int Q = cfg->num_heads * cfg->head_dim, KV = cfg->num_kv_heads * cfg->head_dim;
  if (!eng_build_plan(cfg->hidden_size, Q, KV, cfg->intermediate_size, cfg->num_heads, ncu, P, why, sizeof(why))) {
    smi_set_error("engine plan: %s", why);
    return SMI_EINVAL;
  }
  // every (matrix, part, chain set, round) exactly once, in a stream whose order matches the jobs
  long total = 0, want = 0;
  for (int ph = 0; ph < 4; ++ph) want += (long)P.g.nparts[ph] * P.g.part_imgs[ph];
  std::vector<unsigned char> seen[4];
  for (int ph = 0; ph < 4; ++ph) seen[ph].assign((size_t)P.g.nparts[ph] * 4 * 64, 0);
  for (int c = 0; c < ncu; ++c)
    for (int w = 0; w < kEngWaves; ++w) {
      const EngWavePlan& wp = P.cu[c].w[w];
      for (int ph = 0; ph < 4; ++ph)
        for (int j = wp.jstart[ph]; j < wp.jstart[ph + 1]; ++j) {
          const EngJob& jb = wp.jobs[j];
          SMI_REQUIRE(P.cu[c].parts[P.cu[c].pstart[ph] + jb.slot] == jb.part, "engine plan: job slot does not name its part");
          SMI_REQUIRE((int)jb.goff + jb.nimg <= (int)P.cu[c].len_cu, "engine plan: job beyond the CU's stream");
          for (int r = 0; r < jb.nimg; ++r) {
            const uint32_t d = P.desc[(size_t)c * P.maxlen + jb.goff + r];
            SMI_REQUIRE(d == (((uint32_t)ph << 30) | ((uint32_t)jb.set << 26) | ((uint32_t)r << 16) | jb.part), "engine plan: stream order differs from the job order");
            unsigned char& f = seen[ph][((size_t)jb.part * 4 + jb.set) * 64 + r];
            SMI_REQUIRE(r < 64 && !f, "engine plan: image listed twice");
            f = 1;
            ++total;
          }
        }
    }
  SMI_REQUIRE(total == want, "engine plan: %ld images placed, %ld expected", total, want);
  const EngLds lds = eng_lds(cfg->hidden_size, P.g.KT[EPH_DOWN], P.g.KT[EPH_QKV] > P.g.KT[EPH_O] ? P.g.KT[EPH_QKV] : P.g.KT[EPH_O]);
  stats[0] = P.maxlen; stats[1] = P.max_wave_phase_imgs; stats[2] = P.max_slots; stats[3] = P.max_jobs;
  stats[4] = P.min_load; stats[5] = P.max_load; stats[6] = lds.total; stats[7] = (int32_t)(total);
  return SMI_OK;
}

// Tests: the residual row of sequence row 0 as the last step left it (input of the next step's first layer).
int smi_llm_debug_hidden(smi_llm* L, float* out_host, int n) {
  SMI_REQUIRE(L && out_host && n >= L->H, "smi_llm_debug_hidden: out holds %d floats, %d needed", n, L ? L->H : 0);
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(out_host, L->dec.h, (size_t)L->H * 4, hipMemcpyDeviceToHost));
  return eng_check(L);
}

// Tests / debugging: raw copy of one scratch buffer (what: 0 q [Q] f32, 1 attention operand triples, 2 act triples, 3 h operand
// triples, 4 h [H] f32, 5 engine granules [2][per buffer] u64, 6 partial sums of squares [H / 4], 7 layer-0 K cache of slot 0
// head 0, 8 h + o_proj [H] (fused path), 9 the live rows' logits [rows][V] f32 as the last step's lm_head left them, 16 .. 20 the prefill workspace's q, attention triples, act triples, h triples, h for the
// rows of the last smi_llm_debug_prefill_layer); returns the bytes copied in *got.
int smi_llm_debug_read(smi_llm* L, int what, void* out_host, size_t cap, size_t* got) {
  SMI_REQUIRE(L && out_host && got, "smi_llm_debug_read: null argument");
  const void* src = nullptr;
  size_t n = 0;
  const size_t R = L->B > 0 ? (size_t)L->B : 1;   // buffers 0..4 and 6 hold one entry per live row
  const size_t P = (size_t)L->dbg_pf_rows;        // buffers 16..20: the rows of the last smi_llm_debug_prefill_layer
  switch (what) {
    case 0: src = L->dec.q; n = R * L->Q * 4; break;
    case 1: src = L->dec.xs_attn; n = R * L->Q * 6; break;
    case 2: src = L->dec.xs_act; n = R * L->I * 6; break;
    case 3: src = L->dec.xs_h; n = R * L->H * 6; break;
    case 4: src = L->dec.h; n = R * L->H * 4; break;
    case 5: src = L->eng.gran; n = L->eng.gran ? (size_t)2 * L->eng.gran_per_buf * 8 : 0; break;
    case 6: src = L->dec.ss; n = R * L->H; break;
    case 7: src = L->kcache; n = (size_t)L->cfg.max_positions * kHeadDim * 2; break;
    case 8: src = L->h2; n = (size_t)L->H * 4; break;
    case 9: src = L->logits; n = R * L->cfg.vocab_size * 4; break;
    case 16: src = L->big.q; n = P * L->Q * 4; break;
    case 17: src = L->big.xs_attn; n = P * L->Q * 6; break;
    case 18: src = L->big.xs_act; n = P * L->I * 6; break;
    case 19: src = L->big.xs_h; n = P * L->H * 6; break;
    case 20: src = L->big.h; n = P * L->H * 4; break;
    default: smi_set_error("smi_llm_debug_read: what=%d", what); return SMI_EINVAL;
  }
  SMI_REQUIRE(src && n <= cap, "smi_llm_debug_read: buffer %d holds %zu bytes, out holds %zu", what, n, cap);
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(out_host, src, n, hipMemcpyDeviceToHost));
  *got = n;
  return SMI_OK;
}

// ---- op-level tests (sparkmi_debug.h): one layer's kernels, stage by stage, on caller-given rows -- through launch_one, i.e. the
// launch builders, kernel choices and epilogue fusions of a real step
// (paged cache: the slot gets pages for positions 0 .. pos0 + n - 1 first, and everything issued so far is done on return)
static int debug_kv_check(smi_llm* L, int layer, int slot, int pos0, int n) {
  SMI_REQUIRE(L, "debug KV access: null handle");
  SMI_REQUIRE(layer >= 0 && layer < L->cfg.num_layers && slot >= 0 && slot < L->cfg.max_slots && pos0 >= 0 && n >= 0 &&
              n <= L->cfg.max_positions && pos0 <= L->cfg.max_positions - n,
              "debug KV access: layer %d slot %d positions %d..%d out of range", layer, slot, pos0, pos0 + n);
  const int tokens = pos0 + n;
  SMI_TRY(pages_ensure(L, &slot, &tokens, 1, nullptr));
  SMI_HIP(hipDeviceSynchronize());
  return SMI_OK;
}
// kv_row on the host, through the host mirror of the page table: where position `pos` of (slot, kv head) lives, in rows of 64
// elements, and how many of the positions pos .. pos + n - 1 follow it in memory (paged: to the end of pos's page)
static size_t debug_kv_run(const smi_llm* L, int slot, int kh, int pos, int n, int* run) {
  const size_t nkv = (size_t)L->cfg.num_kv_heads;
  if (!L->paged) { *run = n; return ((size_t)slot * nkv + kh) * L->cfg.max_positions + pos; }
  const int P = 1 << L->pshift, off = pos & (P - 1);
  *run = n < P - off ? n : P - off;
  const size_t pg = (size_t)L->hptab[(size_t)slot * L->ppslot + (pos >> L->pshift)];
  return ((pg * nkv + kh) << L->pshift) + off;
}

// paged cache: every slot with need[slot] > 0 gets pages for its positions 0 .. need[slot] - 1 (all or nothing), table uploaded
static int debug_pages(smi_llm* L, const std::vector<int>& need) {
  std::vector<int> sl, tok;
  for (int s = 0; s < (int)need.size(); ++s)
    if (need[s] > 0) { sl.push_back(s); tok.push_back(need[s]); }
  SMI_TRY(pages_ensure(L, sl.data(), tok.data(), (int)sl.size(), nullptr));
  SMI_HIP(hipDeviceSynchronize());
  return SMI_OK;
}

// k_host / v_host [n][num_kv_heads][64] fp32 in transformers' dim order, keys ALREADY rotated (what a KV cache holds); written to
// positions pos0 .. pos0 + n - 1 of `slot` in the cache's own dtype and row order (K: RoPE pairs adjacent, include/sparkmi.h)
int smi_llm_debug_set_kv(smi_llm* L, int layer, int slot, int pos0, int n, const float* k_host, const float* v_host) {
  { const int rc = debug_kv_check(L, layer, slot, pos0, n); if (rc) return rc; }
  SMI_REQUIRE(k_host && v_host, "smi_llm_debug_set_kv: null argument");
  const int nkv = L->cfg.num_kv_heads, f32 = L->cfg.kv_dtype;
  const size_t esz = f32 ? 4 : 2;
  std::vector<unsigned char> buf((size_t)n * kHeadDim * esz);
  for (int isv = 0; isv < 2; ++isv)
    for (int kh = 0; kh < nkv; ++kh) {
      for (int t = 0; t < n; ++t)
        for (int i = 0; i < kHeadDim; ++i) {
          const int d = isv ? i : (i >> 1) + 32 * (i & 1);   // K rows sit as RoPE pairs (0, 32, 1, 33, ...)
          const float x = (isv ? v_host : k_host)[((size_t)t * nkv + kh) * kHeadDim + d];
          if (f32) ((float*)buf.data())[(size_t)t * kHeadDim + i] = x;
          else {
            uint32_t u; memcpy(&u, &x, 4);
            ((uint16_t*)buf.data())[(size_t)t * kHeadDim + i] = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
          }
        }
      unsigned char* base = (unsigned char*)kv_layer(L, isv ? L->vcache : L->kcache, layer);
      for (int t = 0, run; t < n; t += run) {   // one copy per run of rows that sit together (paged: per page)
        const size_t row0 = debug_kv_run(L, slot, kh, pos0 + t, n - t, &run);
        SMI_HIP(hipMemcpy(base + row0 * kHeadDim * esz, buf.data() + (size_t)t * kHeadDim * esz, (size_t)run * kHeadDim * esz, hipMemcpyHostToDevice));
      }
    }
  return SMI_OK;
}

// the reverse: positions pos0 .. pos0 + n - 1 of `slot` as fp32 [n][num_kv_heads][64] in transformers' dim order
int smi_llm_debug_get_kv(smi_llm* L, int layer, int slot, int pos0, int n, float* k_host, float* v_host) {
  { const int rc = debug_kv_check(L, layer, slot, pos0, n); if (rc) return rc; }
  SMI_REQUIRE(k_host && v_host, "smi_llm_debug_get_kv: null argument");
  const int nkv = L->cfg.num_kv_heads, f32 = L->cfg.kv_dtype;
  const size_t esz = f32 ? 4 : 2;
  std::vector<unsigned char> buf((size_t)n * kHeadDim * esz);
  for (int isv = 0; isv < 2; ++isv)
    for (int kh = 0; kh < nkv; ++kh) {
      const unsigned char* base = (const unsigned char*)kv_layer(L, isv ? L->vcache : L->kcache, layer);
      for (int t = 0, run; t < n; t += run) {
        const size_t row0 = debug_kv_run(L, slot, kh, pos0 + t, n - t, &run);
        SMI_HIP(hipMemcpy(buf.data() + (size_t)t * kHeadDim * esz, base + row0 * kHeadDim * esz, (size_t)run * kHeadDim * esz, hipMemcpyDeviceToHost));
      }
      for (int t = 0; t < n; ++t)
        for (int i = 0; i < kHeadDim; ++i) {
          const int d = isv ? i : (i >> 1) + 32 * (i & 1);
          float x;
          if (f32) x = ((const float*)buf.data())[(size_t)t * kHeadDim + i];
          else { const uint32_t u = (uint32_t)((const uint16_t*)buf.data())[(size_t)t * kHeadDim + i] << 16; memcpy(&x, &u, 4); }
          (isv ? v_host : k_host)[((size_t)t * nkv + kh) * kHeadDim + d] = x;
        }
    }
  return SMI_OK;
}

// The pages `slot` holds, in position order, from the host mirror of the page table: *n = their count (0: contiguous cache, or a
// slot without pages), the first min(*n, cap) in out.
int smi_llm_debug_page_table(smi_llm* L, int slot, int32_t* out, int cap, int32_t* n) {
  SMI_REQUIRE(L && n && cap >= 0 && (out || cap == 0), "smi_llm_debug_page_table: bad argument");
  SMI_REQUIRE(slot >= 0 && slot < L->cfg.max_slots, "smi_llm_debug_page_table: slot %d", slot);
  *n = L->paged ? L->slot_pages[slot] : 0;
  for (int i = 0; i < *n && i < cap; ++i) out[i] = L->hptab[(size_t)slot * L->ppslot + i];
  return SMI_OK;
}

// rows_host: M (slot, pos) pairs; hidden_host [M][hidden] fp32 = the residual rows entering `layer`.  Runs that layer's kernels up
// to and including `stage` (0 QKV + bias + RoPE + KV append, 1 attention, 2 o_proj + residual, 3 gate_up + SwiGLU, 4 down_proj +
// residual) for those rows through launch_one; results are then read with smi_llm_debug_read / smi_llm_debug_get_kv.  Ends the
// current generation (the handle needs a prefill before it generates again).
int smi_llm_debug_layer(smi_llm* L, int layer, int M, const int32_t* rows_host, const float* hidden_host, int stage) {
  SMI_REQUIRE(L && rows_host && hidden_host && M >= 1 && M <= kMaxRows, "smi_llm_debug_layer: bad argument");
  SMI_REQUIRE(layer >= 0 && layer < L->cfg.num_layers && stage >= 0 && stage <= 4, "smi_llm_debug_layer: layer %d stage %d", layer, stage);
  SMI_HIP(hipDeviceSynchronize());
  graphs_flush(L);
  std::vector<RowDesc> rows(kMaxRows, RowDesc{0, 0, 0, 0});
  std::vector<int> need(L->cfg.max_slots, 0);   // paged cache: positions each slot must have pages for
  int maxpos = 0, ident = 1;
  for (int m = 0; m < M; ++m) {
    const int sl = rows_host[2 * m], ps = rows_host[2 * m + 1];
    SMI_REQUIRE(sl >= 0 && sl < L->cfg.max_slots && ps >= 0 && ps < L->cfg.max_positions, "smi_llm_debug_layer: row %d = (slot %d, pos %d)", m, sl, ps);
    rows[m] = RowDesc{sl, ps, 0, 0};
    maxpos = ps > maxpos ? ps : maxpos;
    ident &= sl == m;
    need[sl] = ps + 1 > need[sl] ? ps + 1 : need[sl];
  }
  SMI_TRY(debug_pages(L, need));
  SMI_HIP(hipMemcpy(L->rows, rows.data(), rows.size() * sizeof(RowDesc), hipMemcpyHostToDevice));
  L->B = M; L->identity_slots = ident; L->session = 0; L->started = 0;
  L->attn_seg = segs_for(maxpos + 1);
  DevBuf<float> src;
  if (src.alloc((size_t)M * L->H * 4, "smi_llm_debug_layer: hidden rows")) return SMI_EHIP;
  if (hipMemcpy(src, hidden_host, (size_t)M * L->H * 4, hipMemcpyHostToDevice) != hipSuccess) { smi_set_error("smi_llm_debug_layer: upload failed"); return SMI_EHIP; }
  int rc = SMI_OK;
  {   // from here every way out passes the synchronise below: the kernels are done before src goes
    hipLaunchKernelGGL(k_load_hidden, dim3((M + 3) / 4), dim3(256), 0, 0, src, L->KTh, M, (const float*)sec(L, SMI_LLM_LN1, layer), L->dec.h, L->dec.xs_h,
                       L->dec.ss, L->NTh * 4);
    if (hipGetLastError() != hipSuccess) { rc = SMI_EHIP; smi_set_error("smi_llm_debug_layer: k_load_hidden launch failed"); }
  }
  const bool fused = fuse_o_now(L, L->rows, M);
  const int last = (fused && stage == 2) ? KGU : KQKV + stage;   // one fused row: h + o_proj is formed by gate_up's prologue (read buffer 8)
  for (int k = KQKV; k <= last && rc == SMI_OK; ++k) rc = launch_one(L, k, layer, L->rows, M, nullptr, 0);
  if (hipDeviceSynchronize() != hipSuccess && rc == SMI_OK) { rc = SMI_EHIP; smi_set_error("smi_llm_debug_layer: kernels failed: %s", hipGetErrorString(hipGetLastError())); }
  return rc;
}

// The prompt pass's counterpart of smi_llm_debug_layer: n_seq runs of consecutive positions (seq_host: (slot, first position, rows)
// triples, plan order) as ONE row group in the big workspace, layer `layer`'s kernels up to `stage` through launch_layer_big -- the
// function every layer of a real pass goes through -- with the tiles of pf_tiles_upload and the partial layout of pf_nparts_in.
// stage 5: the whole layer, then the next layer's QKV (the one reader of the RMSNorm partials down_proj leaves).
int smi_llm_debug_prefill_layer(smi_llm* L, int layer, int stage, int n_seq, const int32_t* seq_host, const float* hidden_host, int family) {
  static_assert(SMI_PF_GROUPED == PF_GROUPED && SMI_PF_PGEMM == PF_PGEMM, "sparkmi_debug.h names the pass families");
  SMI_REQUIRE(L && seq_host && hidden_host && n_seq >= 1, "smi_llm_debug_prefill_layer: bad argument");
  SMI_REQUIRE(family == PF_GROUPED || family == PF_PGEMM, "smi_llm_debug_prefill_layer: family %d", family);
  SMI_REQUIRE(layer >= 0 && layer < L->cfg.num_layers && stage >= 0 && stage <= 5, "smi_llm_debug_prefill_layer: layer %d stage %d", layer, stage);
  SMI_REQUIRE(stage == 0 || layer < L->cfg.num_layers - 1, "smi_llm_debug_prefill_layer: the last layer of a prompt pass ends with its K/V append (stage 0 only)");
  SMI_REQUIRE(!L->exact, "smi_llm_debug_prefill_layer: the exact-weights mode has no prompt pass of its own (it runs chunks)");
  long long total = 0;
  int longest = 0;
  for (int b = 0; b < n_seq; ++b) {
    const int sl = seq_host[3 * b], p0 = seq_host[3 * b + 1], n = seq_host[3 * b + 2];
    SMI_REQUIRE(sl >= 0 && sl < L->cfg.max_slots && p0 >= 0 && n >= 1 && n <= L->cfg.max_positions && p0 <= L->cfg.max_positions - n,
                "smi_llm_debug_prefill_layer: sequence %d = (slot %d, positions %d .. +%d) outside the cache", b, sl, p0, n);
    for (int a = 0; a < b; ++a) SMI_REQUIRE(seq_host[3 * a] != sl, "smi_llm_debug_prefill_layer: sequences %d and %d share slot %d", a, b, sl);
    total += n;
    longest = p0 + n > longest ? p0 + n : longest;
  }
  SMI_REQUIRE(total >= 1 && total <= 4096, "smi_llm_debug_prefill_layer: %lld rows (a row group holds 1 .. 4096)", total);
  const int M = (int)total;
  SMI_HIP(hipDeviceSynchronize());
  graphs_flush(L);
  L->B = 0; L->session = 0; L->started = 0; L->dbg_pf_rows = 0;
  L->attn_seg = segs_for(longest);
  int rc;
  {
    std::vector<int> need(L->cfg.max_slots, 0);
    for (int b = 0; b < n_seq; ++b) need[seq_host[3 * b]] = seq_host[3 * b + 1] + seq_host[3 * b + 2];
    if ((rc = debug_pages(L, need))) return rc;
  }
  if ((rc = ensure_plan(L, (size_t)M))) return rc;
  if ((rc = ensure_big(L, M))) return rc;
  L->host_rows.clear();
  for (int b = 0; b < n_seq; ++b)
    for (int t = 0; t < seq_host[3 * b + 2]; ++t) L->host_rows.push_back(RowDesc{seq_host[3 * b], seq_host[3 * b + 1] + t, 0, 0});
  SMI_HIP(hipMemcpy(L->plan, L->host_rows.data(), (size_t)M * sizeof(RowDesc), hipMemcpyHostToDevice));
  if ((rc = pf_tiles_upload(L, L->host_rows.data(), M, 0))) return rc;
  DevBuf<float> src;
  if (src.alloc((size_t)M * L->H * 4, "smi_llm_debug_prefill_layer: hidden rows")) return SMI_EHIP;
  if (hipMemcpy(src, hidden_host, (size_t)M * L->H * 4, hipMemcpyHostToDevice) != hipSuccess) { smi_set_error("smi_llm_debug_prefill_layer: upload failed"); return SMI_EHIP; }
  {   // from here every way out passes the synchronise below: the kernels are done before src goes
    hipLaunchKernelGGL(k_load_hidden, dim3((M + 3) / 4), dim3(256), 0, 0, src, L->KTh, M, (const float*)sec(L, SMI_LLM_LN1, layer), L->big.h, L->big.xs_h,
                       L->big.ss, pf_nparts_in(L, M, family));
    if (hipGetLastError() != hipSuccess) { rc = SMI_EHIP; smi_set_error("smi_llm_debug_prefill_layer: k_load_hidden launch failed"); }
  }
  if (rc == SMI_OK) rc = launch_layer_big(L, layer, L->plan, M, family, stage < 5 ? KQKV + stage : KD, 0);
  if (rc == SMI_OK && stage == 5) rc = launch_layer_big(L, layer + 1, L->plan, M, family, KQKV, 0);
  if (hipDeviceSynchronize() != hipSuccess && rc == SMI_OK) { rc = SMI_EHIP; smi_set_error("smi_llm_debug_prefill_layer: kernels failed: %s", hipGetErrorString(hipGetLastError())); }
  if (rc == SMI_OK) L->dbg_pf_rows = M;
  return rc;
}

// Host only: the k_attn_pf2 tiles pf_tiles_build makes of M (slot, pos) rows, as (m0, n, slot, pos0) quadruples; *n = their count
// (at most cap are written).
int smi_llm_pf_tiles(const int32_t* rows_host, int M, int32_t* out, int cap, int32_t* n) {
  SMI_REQUIRE(rows_host && n && M >= 0 && cap >= 0 && (out || cap == 0), "smi_llm_pf_tiles: bad argument");
  std::vector<RowDesc> rows((size_t)M);
  for (int m = 0; m < M; ++m) rows[m] = RowDesc{rows_host[2 * m], rows_host[2 * m + 1], 0, 0};
  std::vector<PfTile> T;
  pf_tiles_build(rows.data(), M, T);
  for (size_t i = 0; i < T.size() && i < (size_t)cap; ++i) { out[4 * i] = T[i].m0; out[4 * i + 1] = T[i].n; out[4 * i + 2] = T[i].slot; out[4 * i + 3] = T[i].pos0; }
  *n = (int32_t)T.size();
  return SMI_OK;
}

// Host only: the picks of a layer's four GEMMs and of lm_head (out[0..5): QKV, o_proj, gate_up, down_proj, lm_head) for M rows at
// cfg's shape -- the functions launch_one / launch_layer_big pick with.  flags: the switches as plain values, -1 = as
// smi_llm_create leaves the field without any switch; null: all of them.
int smi_llm_gemm_forms(const smi_llm_cfg* cfg, int M, int layer_pos, const smi_gemm_flags* flags, smi_gemm_form_info* out) {
  SMI_REQUIRE(cfg_ok(cfg) && out && M >= 1, "smi_llm_gemm_forms: invalid argument");
  SMI_REQUIRE(layer_pos >= SMI_LAYER_FIRST && layer_pos <= SMI_LAYER_LAST, "smi_llm_gemm_forms: layer position %d", layer_pos);
  smi_gemm_flags f;
  if (flags) f = *flags;
  else memset(&f, 0xff, sizeof(f));
  SMI_REQUIRE(f.pass == -1 || f.pass == 0 || f.pass == PF_GROUPED || f.pass == PF_PGEMM, "smi_llm_gemm_forms: pass %d", f.pass);
  SMI_REQUIRE(f.pass > 0 || M <= kMaxRows, "smi_llm_gemm_forms: a decode step has 1 .. %d rows", kMaxRows);
  const int H = cfg->hidden_size, Q = cfg->num_heads * cfg->head_dim, KV = cfg->num_kv_heads * cfg->head_dim, I = cfg->intermediate_size;
  const int KTh = H / 32, KTq = Q / 32, KTi = I / 32, NTqkv = (Q + 2 * KV) / 16, NTh = H / 16, NTgu = 2 * I / 16;
  const int NTlm = (int)(make_layout(cfg).vpad / 16), lm_cap = (NTlm + 3) / 4;
  PickEnv e{};
  e.pass = f.pass < 0 ? 0 : f.pass;
  e.exact = f.exact < 0 ? cfg->weights_exact : f.exact;
  e.fused = f.fused < 0 ? (e.pass == 0 && M == 1 && !e.exact && fuse_o_fits(cfg->num_heads, NTh, KTh) ? 1 : 0) : f.fused;
  e.stamps = f.stamps < 0 ? 0 : f.stamps; e.tune2 = f.tune2 < 0 ? 0 : f.tune2;
  e.pf_mask = f.prefetch_mask < 0 ? 1 : f.prefetch_mask; e.pf_rows = f.prefetch_rows < 0 ? 1 : f.prefetch_rows;
  e.kv_f32 = f.kv_f32 < 0 ? (cfg->kv_dtype ? 1 : 0) : f.kv_f32;
  e.pg_split_rows = f.pg_split_rows < 0 ? kPgSplitRows : f.pg_split_rows;
  e.lm_restricted = f.lm_restricted < 0 ? 0 : f.lm_restricted;
  e.lm_blocks = f.lm_blocks < 0 ? (lm_cap < 512 ? lm_cap : 512) : f.lm_blocks;
  e.lm_screen = f.lm_screen < 0 ? 0 : f.lm_screen;
  SMI_REQUIRE(!e.lm_screen || (KTh <= 32 && !e.exact && !e.lm_restricted && M == 1), "smi_llm_gemm_forms: the screened lm_head is one unconstrained row's on the persistent kernel");
  SMI_REQUIRE(!e.lm_restricted || (KTh <= 32 && !e.exact), "smi_llm_gemm_forms: the restricted lm_head is the persistent kernels'");
  GemmPick k[5];
  e.has_pf = e.pass == 0;                                   // QKV's helpers: this layer's gate_up slices
  k[0] = pick_qkv(KTh, NTqkv, M, e);
  e.has_pf = 0;
  k[1] = pick_o(KTq, NTh, cfg->num_heads, M, e);
  k[2] = pick_gu(KTh, NTgu, cfg->num_heads, M, e);
  e.has_pf = e.pass == 0 && layer_pos != SMI_LAYER_LAST;    // down_proj's: the next layer's QKV slices
  k[3] = pick_d(KTi, NTh, M, e);
  e.has_pf = 0; e.pass = 0;
  k[4] = pick_lm(KTh, NTlm, M <= kMaxRows ? M : kMaxRows, e);
  for (int i = 0; i < 5; ++i) {
    SMI_REQUIRE(k[i].form != GF_BAD, "smi_llm_gemm_forms: kernel %d has no form for %d rows and these switches", i, M);
    smi_gemm_form_info& o = out[i];
    memset(&o, 0, sizeof(o));
    gemm_form_name(k[i], o.kernel, sizeof(o.kernel));
    o.launches = k[i].launches;
    if (k[i].launches) { o.grid[0] = k[i].gx; o.grid[1] = k[i].gy; o.block = k[i].block; o.grid2 = k[i].gx2; o.lds_bytes = (int64_t)k[i].lds; }
  }
  return SMI_OK;
}

// Diagnostics: the stamp buffer of the last smi_llm_debug_stamps launch as it is (10 ns ticks of s_memrealtime; k_lm32 leaves
// four stamps per streamed group of its block 0: group start, MFMAs issued + partial sums written, reduce barrier passed, group done)
int smi_llm_debug_raw_stamps(smi_llm* L, unsigned long long* out, int n) {
  SMI_REQUIRE(L && out && n > 0 && n <= 4096 * 8, "smi_llm_debug_raw_stamps: bad argument");
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(out, L->stamps, (size_t)n * 8, hipMemcpyDeviceToHost));
  return SMI_OK;
}

// ---- kernel-alone runs (the six entries below): the state around them, and the table the lm_head would have left.  Each entry
// stages its rows, writes the records its kernels read, commits the controls, composes the stage launchers a decode step is
// composed of (launch_ngram_ban .. launch_finalize; smi_llm_debug_head: launch_one itself) and fetches what they left.
// The scope of one run.  Before: the device idle, every record clean, rows 0 .. n-1 = slots 0 .. n-1 with flags[m] tokens emitted
// (null: none); rc says whether that held.  After, on every way out: clean records again, `dev` freed (with the scope); rows, controls, the lm_head
// partials and the histories no longer belong to a generation.
struct Alone {
  smi_llm* L;
  DevBuf<float> dev;      // a device buffer of the run (smi_llm_debug_head's hidden rows)
  int rc;
  Alone(smi_llm* L_, int n, const int32_t* flags) : L(L_), rc(begin(n, flags)) {}
  Alone(const Alone&) = delete;
  Alone& operator=(const Alone&) = delete;
  ~Alone() {
    slots_clear(L);
    L->started = 0;
  }
  int begin(int n, const int32_t* flags) {
    SMI_HIP(hipDeviceSynchronize());
    slots_clear(L);
    std::vector<RowDesc> rows(kMaxRows, RowDesc{0, 0, 0, 0});
    for (int m = 0; m < n; ++m) rows[m] = RowDesc{m, 0, 0, flags ? flags[m] : 0};
    SMI_HIP(hipMemcpy(L->rows, rows.data(), rows.size() * sizeof(RowDesc), hipMemcpyHostToDevice));
    return SMI_OK;
  }
};
// (maximum, lowest id) of each of the nblk contiguous sets of `per` ids of every logits row [n_rows][V], as the lm_head leaves
// them: pv / pi [n_rows][nblk]
static void block_maxima(const float* logits, int n_rows, int V, int nblk, int per, std::vector<float>& pv, std::vector<int32_t>& pi) {
  pv.assign((size_t)n_rows * nblk, -INFINITY);
  pi.assign((size_t)n_rows * nblk, 0x7fffffff);
  for (int m = 0; m < n_rows; ++m)
    for (int j = 0; j < nblk; ++j)
      for (int i = j * per; i < V && i < (j + 1) * per; ++i) {
        const float x = logits[(size_t)m * V + i];
        if (x > pv[(size_t)m * nblk + j]) { pv[(size_t)m * nblk + j] = x; pi[(size_t)m * nblk + j] = i; }
      }
}
// Row staging: the caller's logits [n][V] into the handle's rows and, per > 0, their maxima over nblk contiguous sets of `per`
// ids where the lm_head leaves them.  copies > 1: the n rows again in the next n rows, and so on.
static int alone_rows(smi_llm* L, const float* logits, int n, int nblk, int per, int copies = 1) {
  const size_t V = (size_t)L->cfg.vocab_size;
  std::vector<float> pv;
  std::vector<int32_t> pi;
  if (per > 0) block_maxima(logits, n, (int)V, nblk, per, pv, pi);
  for (size_t c = 0; c < (size_t)copies; ++c) {
    SMI_HIP(hipMemcpy(L->logits + c * n * V, logits, (size_t)n * V * 4, hipMemcpyHostToDevice));
    if (per > 0) {
      SMI_HIP(hipMemcpy(L->pval + c * n * nblk, pv.data(), pv.size() * 4, hipMemcpyHostToDevice));
      SMI_HIP(hipMemcpy(L->pidx + c * n * nblk, pi.data(), pi.size() * 4, hipMemcpyHostToDevice));
    }
  }
  return SMI_OK;
}
// Row m's context ctx[m][0 .. ctx_len[m]), of which the first prompt_len[m] ids are its prompt: the checks of `who`
// (smi_llm_debug_seqbias: a prompt of 1 or more ids; smi_llm_debug_ngram, `store`: 0 or more, which must fit the prompt store);
// *gen = the tokens the row has emitted.
static int alone_ctx_check(const smi_llm* L, const char* who, int m, const int64_t* ctx, const int32_t* ctx_len, const int32_t* prompt_len,
                           int ctx_cap, bool store, int32_t* gen) {
  const int V = L->cfg.vocab_size, lo = store ? 0 : 1;
  SMI_REQUIRE(prompt_len[m] >= lo && prompt_len[m] <= ctx_len[m] && ctx_len[m] <= ctx_cap && (!store || prompt_len[m] <= L->cfg.max_positions),
              "%s: row %d: %d <= prompt_len <= ctx_len <= ctx_cap%s does not hold", who, m, lo, store ? ", prompt_len <= max_positions" : "");
  SMI_REQUIRE(ctx_len[m] - prompt_len[m] < L->max_steps, "%s: row %d: more generated tokens than the history holds", who, m);
  for (int t = 0; t < ctx_len[m]; ++t)
    SMI_REQUIRE(ctx[(size_t)m * ctx_cap + t] >= 0 && ctx[(size_t)m * ctx_cap + t] < V, "%s: ctx[%d][%d] outside the vocabulary", who, m, t);
  *gen = ctx_len[m] - prompt_len[m];
  return SMI_OK;
}
// Context staging: the generated tokens of every row into the token history, as k_finalize would have left them, and -- `store`
// -- the prompts into the slots' rows of the prompt store.
static int alone_contexts(smi_llm* L, int n, const int64_t* ctx, const int32_t* ctx_len, const int32_t* prompt_len, int ctx_cap, bool store) {
  const int P = L->cfg.max_positions;
  int max_gen = 0;
  for (int m = 0; m < n; ++m) max_gen = ctx_len[m] - prompt_len[m] > max_gen ? ctx_len[m] - prompt_len[m] : max_gen;
  if (store) {
    std::vector<int32_t> pctx((size_t)n * P, 0);
    for (int m = 0; m < n; ++m)
      for (int t = 0; t < prompt_len[m]; ++t) pctx[(size_t)m * P + t] = (int32_t)ctx[(size_t)m * ctx_cap + t];
    SMI_HIP(hipMemcpy(L->pctx, pctx.data(), pctx.size() * 4, hipMemcpyHostToDevice));
  }
  if (max_gen > 0) {
    std::vector<int64_t> hist((size_t)max_gen * kMaxRows, 0);
    for (int m = 0; m < n; ++m)
      for (int t = prompt_len[m]; t < ctx_len[m]; ++t) hist[(size_t)(t - prompt_len[m]) * kMaxRows + m] = ctx[(size_t)m * ctx_cap + t];
    SMI_HIP(hipMemcpy(L->hist, hist.data(), hist.size() * 8, hipMemcpyHostToDevice));
  }
  return SMI_OK;
}
// A sampling row that keeps only its arg-max: k_penalize writes such a row's processed logits back, and k_finalize, handed no
// sampler tokens, takes the arg-max.
static SampRec samp_neutral() {
  SampRec r;
  memset(&r, 0, sizeof(r));
  r.mode = SMI_SAMPLING_SAMPLE; r.top_k = 1; r.inv_temp = 1.f; r.top_p = 1.f;
  return r;
}
// Commit: the controls as the entry wrote them, no row finished and -- where the sampler runs -- empty candidate lists.
static int alone_commit(smi_llm* L, bool sampler) {
  SMI_HIP(hipMemcpy(L->ctl, &L->hctl, sizeof(Ctl), hipMemcpyHostToDevice));
  SMI_HIP(hipMemset(L->finished, 0, kMaxRows * 4));
  if (sampler) SMI_HIP(hipMemset(L->cand_n, 0, kMaxRows * 4));
  return SMI_OK;
}
// Fetch: wait for the launches, then what the caller asks for of the first n rows (each nullable): the logits rows [n][V], the
// tokens k_finalize left in the row descriptors, the finished flags.
static int alone_fetch(smi_llm* L, int n, float* logits_out, int32_t* token_out, int32_t* finished_out) {
  SMI_HIP(hipDeviceSynchronize());
  if (logits_out) SMI_HIP(hipMemcpy(logits_out, L->logits, (size_t)n * L->cfg.vocab_size * 4, hipMemcpyDeviceToHost));
  if (finished_out) SMI_HIP(hipMemcpy(finished_out, L->finished, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (token_out) {
    std::vector<RowDesc> after((size_t)n);
    SMI_HIP(hipMemcpy(after.data(), L->rows, after.size() * sizeof(RowDesc), hipMemcpyDeviceToHost));
    for (int m = 0; m < n; ++m) token_out[m] = after[m].token;
  }
  return SMI_OK;
}

// Tests: the sampler alone on a caller's logits row (see sparkmi_debug.h).
int smi_llm_debug_sample(smi_llm* L, const float* logits_host, int n_rows, uint64_t seed, int use_bound, int32_t* tokens_out) {
  SMI_REQUIRE(L && tokens_out && n_rows >= 1 && n_rows <= kMaxRows, "smi_llm_debug_sample: bad argument");
  SMI_REQUIRE(L->do_sample, "smi_llm_debug_sample: smi_llm_set_sampling(do_sample = 1, ...) first");
  const int V = L->cfg.vocab_size;
  const int nblk = lm_blocks_for(L, n_rows);
  Alone run(L, kMaxRows, nullptr);   // (clean records: every row inherits the handle's settings)
  SMI_TRY(run.rc);
  // what the lm_head blocks would have left: one maximum per block; here block j holds the j-th contiguous share of the row
  if (logits_host) SMI_TRY(alone_rows(L, logits_host, 1, nblk, (V + nblk - 1) / nblk, kMaxRows));
  for (int m = 0; m < kMaxRows; ++m) L->hctl.seqid[m] = m;
  L->hctl.seed = seed;
  SMI_TRY(alone_commit(L, true));
  SMI_TRY(launch_sampler(L, n_rows, use_bound != 0, 0));
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(tokens_out, L->tok, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  return SMI_OK;
}

// Tests: the penalty kernel alone on caller rows (see sparkmi_debug.h).
int smi_llm_debug_penalize(smi_llm* L, const float* logits_host, int n_rows, const uint16_t* hist_host, const smi_penalty_params* pens,
                           const int32_t* emitted_host, float* logits_out, int32_t* argmax_out) {
  SMI_REQUIRE(L && logits_host && hist_host && pens && emitted_host && logits_out && argmax_out, "smi_llm_debug_penalize: null argument");
  SMI_REQUIRE(n_rows >= 1 && n_rows <= L->cfg.max_slots && n_rows <= kMaxRows, "smi_llm_debug_penalize: n_rows=%d outside 1..max_slots", n_rows);
  for (int m = 0; m < n_rows; ++m) SMI_TRY(validate_penalty(L, pens[m], m));
  const size_t V = (size_t)L->cfg.vocab_size;
  const int nblk = lm_blocks_for(L, n_rows);
  Alone run(L, n_rows, emitted_host);
  SMI_TRY(run.rc);
  SMI_TRY(alone_rows(L, logits_host, n_rows, nblk, 0));
  SMI_HIP(hipMemcpy(L->phist, hist_host, (size_t)n_rows * V * 2, hipMemcpyHostToDevice));
  for (int m = 0; m < n_rows; ++m) {
    L->hctl.samp[m].mode = SMI_SAMPLING_SAMPLE;   // (a sampling row: the kernel writes its processed logits back)
    PenRec& r = L->hctl.pen[m];
    r = pen_record(&pens[m]);
    if (!r.on) { r.rep = 1.f; r.prompt = pens[m].penalize_prompt; r.on = 1; }   // a neutral record runs too: as the identity
  }
  SMI_TRY(alone_commit(L, false));
  SMI_TRY(launch_penalize(L, n_rows, nullptr, 0));
  SMI_TRY(alone_fetch(L, n_rows, logits_out, nullptr, nullptr));
  std::vector<float> pv((size_t)n_rows * nblk);
  std::vector<int32_t> pi((size_t)n_rows * nblk);
  SMI_HIP(hipMemcpy(pv.data(), L->pval, pv.size() * 4, hipMemcpyDeviceToHost));
  SMI_HIP(hipMemcpy(pi.data(), L->pidx, pi.size() * 4, hipMemcpyDeviceToHost));
  for (int m = 0; m < n_rows; ++m) {   // k_finalize's reduction of the maxima
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = 0; j < nblk; ++j) {
      const float v = pv[(size_t)m * nblk + j];
      const int ix = pi[(size_t)m * nblk + j];
      if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    argmax_out[m] = bi;
  }
  return SMI_OK;
}

// Tests: the log-probability kernels alone on caller rows (see sparkmi_debug.h).
int smi_llm_debug_logprob(smi_llm* L, const float* logits_host, int n_rows, const float* temperature_host, const int32_t* tokens_host,
                          float* lp_out) {
  SMI_REQUIRE(L && logits_host && temperature_host && tokens_host && lp_out, "smi_llm_debug_logprob: null argument");
  SMI_REQUIRE(n_rows >= 1 && n_rows <= L->cfg.max_slots && n_rows <= kMaxRows, "smi_llm_debug_logprob: n_rows=%d outside 1..max_slots", n_rows);
  const int V = L->cfg.vocab_size;
  for (int m = 0; m < n_rows; ++m) {
    SMI_REQUIRE(std::isfinite(temperature_host[m]) && temperature_host[m] > 0.f, "smi_llm_debug_logprob: temperature[%d] must be finite and > 0", m);
    SMI_REQUIRE(tokens_host[m] >= 0 && tokens_host[m] < V, "smi_llm_debug_logprob: tokens[%d]=%d outside the vocabulary", m, tokens_host[m]);
  }
  SMI_REQUIRE(L->max_steps >= 1, "smi_llm_debug_logprob: no history");
  const int nblk = lm_blocks_for(L, n_rows);
  Alone run(L, n_rows, nullptr);
  SMI_TRY(run.rc);
  SMI_TRY(alone_rows(L, logits_host, n_rows, nblk, pen_set_ids(V, nblk)));
  SMI_HIP(hipMemcpy(L->tok, tokens_host, (size_t)n_rows * 4, hipMemcpyHostToDevice));
  for (int m = 0; m < n_rows; ++m) {   // (no tokens emitted: k_finalize writes lp[0][m])
    SampRec& r = L->hctl.samp[m];
    r = samp_neutral();              // a sampling row: its token is the caller's (L->tok) and its z is scaled by 1/T
    r.inv_temp = 1.0f / temperature_host[m];
    L->hctl.lp[m] = 1;
  }
  SMI_TRY(alone_commit(L, false));
  SMI_TRY(launch_logprob(L, n_rows, 0));
  FinP f = fin_params(L, n_rows);
  f.tok = L->tok;
  f.lp = L->lp; f.lp_part = L->lp_part; f.lp_rowc = L->lp_rowc;
  SMI_TRY(launch_finalize(f, 0));
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(lp_out, L->lp, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
  return SMI_OK;
}

// Tests: the bias stage and k_finalize's stop match alone on caller rows (see sparkmi_debug.h).
int smi_llm_debug_seqbias(smi_llm* L, const float* logits_host, int n_rows, const smi_seq_params* seq, const int64_t* ctx_host,
                          const int32_t* ctx_len_host, const int32_t* prompt_len_host, int ctx_cap, const int32_t* min_new_host,
                          float* logits_out, int32_t* token_out, int32_t* finished_out) {
  SMI_REQUIRE(L && logits_host && seq && ctx_host && ctx_len_host && prompt_len_host && logits_out && token_out && finished_out,
              "smi_llm_debug_seqbias: null argument");
  SMI_REQUIRE(n_rows >= 1 && n_rows <= L->cfg.max_slots && n_rows <= kMaxRows, "smi_llm_debug_seqbias: n_rows=%d outside 1..max_slots", n_rows);
  int32_t gen[kMaxRows];   // tokens emitted so far, per row
  for (int m = 0; m < n_rows; ++m) {
    SMI_TRY(validate_seq(L, seq[m], nullptr, nullptr, m));
    SMI_REQUIRE(!min_new_host || (min_new_host[m] >= 0 && min_new_host[m] <= L->cfg.max_positions), "smi_llm_debug_seqbias: min_new[%d] out of range", m);
    SMI_TRY(alone_ctx_check(L, "smi_llm_debug_seqbias", m, ctx_host, ctx_len_host, prompt_len_host, ctx_cap, false, &gen[m]));
  }
  const int nblk = lm_blocks_for(L, n_rows);
  Alone run(L, n_rows, gen);
  SMI_TRY(run.rc);
  SMI_TRY(alone_rows(L, logits_host, n_rows, nblk, pen_set_ids(L->cfg.vocab_size, nblk)));
  for (int m = 0; m < n_rows; ++m) {
    L->hctl.samp[m] = samp_neutral();
    if (min_new_host && min_new_host[m] > 0) {   // only min_new of a neutral penalty record: the stop match reads it
      L->hctl.pen[m].rep = 1.f; L->hctl.pen[m].min_new = min_new_host[m];
    }
    L->hseq[(size_t)m] = seq_record(&seq[m], ctx_host + (size_t)m * ctx_cap, prompt_len_host[m]);
    if (L->hseq[(size_t)m].plen == 0) L->hseq[(size_t)m].plen = prompt_len_host[m];
    L->seq_dirty[m] = 1;
  }
  SMI_TRY(alone_contexts(L, n_rows, ctx_host, ctx_len_host, prompt_len_host, ctx_cap, false));
  SMI_HIP(hipMemcpy(L->seq, L->hseq.data(), (size_t)n_rows * sizeof(SeqRec), hipMemcpyHostToDevice));
  SMI_TRY(alone_commit(L, false));
  SMI_TRY(launch_penalize(L, n_rows, L->seq, 0));
  FinP f = fin_params(L, n_rows);
  f.seq = L->seq;
  SMI_TRY(launch_finalize(f, 0));
  return alone_fetch(L, n_rows, logits_out, token_out, finished_out);
}

// Tests: the n-gram ban, k_penalize and k_finalize alone on caller rows (see sparkmi_debug.h).
int smi_llm_debug_ngram(smi_llm* L, const float* logits_host, int n_rows, const int32_t* ngram_host, const int64_t* ctx_host,
                        const int32_t* ctx_len_host, const int32_t* prompt_len_host, int ctx_cap, float* logits_out, int32_t* token_out) {
  SMI_REQUIRE(L && logits_host && ngram_host && ctx_host && ctx_len_host && prompt_len_host && logits_out && token_out,
              "smi_llm_debug_ngram: null argument");
  SMI_REQUIRE(n_rows >= 1 && n_rows <= L->cfg.max_slots && n_rows <= kMaxRows, "smi_llm_debug_ngram: n_rows=%d outside 1..max_slots", n_rows);
  int32_t gen[kMaxRows];   // tokens emitted so far, per row
  for (int m = 0; m < n_rows; ++m) {
    SMI_REQUIRE(ngram_host[m] >= 0 && ngram_host[m] <= SMI_MAX_NGRAM, "smi_llm_debug_ngram: ngram[%d]=%d outside 0..%d", m, ngram_host[m], SMI_MAX_NGRAM);
    SMI_TRY(alone_ctx_check(L, "smi_llm_debug_ngram", m, ctx_host, ctx_len_host, prompt_len_host, ctx_cap, true, &gen[m]));
  }
  const int nblk = lm_blocks_for(L, n_rows);
  Alone run(L, n_rows, gen);
  SMI_TRY(run.rc);
  SMI_TRY(alone_rows(L, logits_host, n_rows, nblk, pen_set_ids(L->cfg.vocab_size, nblk)));
  for (int m = 0; m < n_rows; ++m) {
    L->hctl.samp[m] = samp_neutral();
    L->hctl.ngram[m] = ngram_host[m]; L->hctl.ngplen[m] = prompt_len_host[m];
  }
  SMI_TRY(alone_contexts(L, n_rows, ctx_host, ctx_len_host, prompt_len_host, ctx_cap, true));
  SMI_TRY(alone_commit(L, false));
  SMI_TRY(launch_ngram_ban(L, n_rows, 0));
  SMI_TRY(launch_penalize(L, n_rows, nullptr, 0));
  SMI_TRY(launch_finalize(fin_params(L, n_rows), 0));
  return alone_fetch(L, n_rows, logits_out, token_out, nullptr);
}

// Tests: the head of a decode step alone on caller rows -- launch_one(KLM), then launch_one(KFIN) -- (see sparkmi_debug.h).
int smi_llm_debug_head(smi_llm* L, int M, smi_head_io* io) {
  SMI_REQUIRE(L && io && io->hidden, "smi_llm_debug_head: null argument");
  SMI_REQUIRE(M >= 1 && M <= L->cfg.max_slots && M <= kMaxRows, "smi_llm_debug_head: M=%d outside 1..max_slots", M);
  SMI_REQUIRE((io->flags & ~(SMI_HEAD_FIN | SMI_HEAD_POISON | SMI_HEAD_SCREEN)) == 0, "smi_llm_debug_head: flags=%d", io->flags);
  if ((io->flags & SMI_HEAD_SCREEN) && lm_screen_fits(L)) SMI_TRY(lm_screen_build(L));   // (outside any capture; nothing if it exists)
  struct ScrForce {   // the request holds for this call's launches only
    smi_llm* L;
    ScrForce(smi_llm* L_, int on) : L(L_) { L->scr_force = on; }
    ~ScrForce() { L->scr_force = 0; }
  } scr_force(L, (io->flags & SMI_HEAD_SCREEN) ? 1 : 0);
  const int V = L->cfg.vocab_size, nblk = lm_blocks_for(L, M);
  SMI_REQUIRE((!io->pval && !io->pidx) || (size_t)io->pcap >= (size_t)M * nblk, "smi_llm_debug_head: pval / pidx hold %d entries, %d rows x %d columns needed",
              io->pcap, M, nblk);
  if (io->allow)
    for (int m = 0; m < M; ++m) SMI_TRY(validate_allow(L, io->allow[m], nullptr, m));
  Alone run(L, M, nullptr);
  SMI_TRY(run.rc);
  graphs_flush(L);
  L->B = M; L->identity_slots = 1; L->session = 0; L->started = 0; L->attn_seg = 1;
  L->lm_restrict = io->allow != nullptr;
  for (int m = 0; m < M; ++m) {
    L->hctl.seqid[m] = m;
    if (io->reads && io->reads[m]) {   // a neutral sampling record; here the step's features see it too
      L->hctl.samp[m] = samp_neutral();
      L->slot_feat[m] |= F_SAMPLE;
    }
    if (io->allow) {
      L->hctl.allow[m] = allow_record(&io->allow[m], V);
      if (L->hctl.allow[m].n > 0) L->slot_feat[m] |= F_ALLOW;
    }
    L->lm_restrict &= (L->slot_feat[m] & F_ALLOW) != 0;   // live_set's rule
  }
  L->hctl.seed = 0;
  SMI_TRY(allow_tiles_upload(L, 0));
  SMI_TRY(alone_commit(L, true));
  if (io->flags & SMI_HEAD_POISON) SMI_HIP(hipMemset(L->logits, 0xff, (size_t)kMaxRows * V * 4));   // 0xffffffff: a quiet NaN
  if (run.dev.alloc((size_t)M * L->H * 4, "smi_llm_debug_head: hidden rows")) return SMI_EHIP;
  SMI_HIP(hipMemcpy(run.dev, io->hidden, (size_t)M * L->H * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_load_hidden, dim3((M + 3) / 4), dim3(256), 0, 0, run.dev, L->KTh, M, (const float*)sec(L, SMI_LLM_FINAL_NORM, 0), L->dec.h,
                     L->dec.xs_h, L->dec.ss, L->NTh * 4);
  SMI_LAUNCH_CHECK();
  L->lm_note_n = 0; L->lm_note_form[0] = 0; L->lm_note_grid[0] = L->lm_note_grid[1] = L->lm_note_block = 0;
  SMI_TRY(launch_one(L, KLM, 0, L->rows, M, nullptr, 0));
  SMI_TRY(alone_fetch(L, M, io->logits_lm, nullptr, nullptr));
  io->nblk = nblk; io->launches = L->lm_note_n; io->grid[0] = L->lm_note_grid[0]; io->grid[1] = L->lm_note_grid[1]; io->block = L->lm_note_block;
  memcpy(io->form, L->lm_note_form, sizeof(io->form));
  if (io->pval) SMI_HIP(hipMemcpy(io->pval, L->pval, (size_t)M * nblk * 4, hipMemcpyDeviceToHost));
  if (io->pidx) SMI_HIP(hipMemcpy(io->pidx, L->pidx, (size_t)M * nblk * 4, hipMemcpyDeviceToHost));
  if (io->flags & SMI_HEAD_FIN) {
    SMI_TRY(launch_one(L, KFIN, 0, L->rows, M, nullptr, 0));
    SMI_TRY(alone_fetch(L, M, io->logits_fin, io->tokens, nullptr));
  }
  return SMI_OK;
}

// Diagnostics: the screened lm_head's last list and the lengths of the last selections (see sparkmi_debug.h).
int smi_llm_debug_lm_screen(smi_llm* L, int32_t* tiles, int cap, int32_t* n_tiles, int32_t* counts, int ccap, int32_t* n_counts, int reset) {
  SMI_REQUIRE(L && n_tiles && n_counts && cap >= 0 && ccap >= 0 && (tiles || cap == 0) && (counts || ccap == 0), "smi_llm_debug_lm_screen: bad argument");
  SMI_REQUIRE(L->scr_ready && L->scr_log, "smi_llm_debug_lm_screen: this handle has no int8 copy of its lm_head");
  SMI_HIP(hipDeviceSynchronize());
  std::vector<int32_t> list((size_t)L->NTlm + 1), log(4097);
  SMI_HIP(hipMemcpy(list.data(), L->scr_list, list.size() * 4, hipMemcpyDeviceToHost));
  SMI_HIP(hipMemcpy(log.data(), L->scr_log, log.size() * 4, hipMemcpyDeviceToHost));
  const int nt = list[0] < 0 ? 0 : list[0] < L->NTlm ? list[0] : L->NTlm;
  *n_tiles = nt;
  for (int i = 0; i < nt && i < cap; ++i) tiles[i] = list[1 + i];
  const int total = log[0], kept = total < 4096 ? total : 4096;
  *n_counts = kept;
  for (int i = 0; i < kept && i < ccap; ++i) counts[i] = log[1 + ((total - kept + i) & 4095)];
  if (reset) SMI_HIP(hipMemset(L->scr_log, 0, 4));
  return SMI_OK;
}

// Diagnostics (SPARKMI_ENGINE_STAMPS=1): out[3][layers][16] microseconds since the first stamp of the last engine launch:
// CU 0 and the first head CU after the hand-offs A (h), B (q|k|v), C (attention), D (h_mid), E (act).
int smi_llm_engine_stamps(smi_llm* L, double* out, int cap) {
  SMI_REQUIRE(L && out && L->eng.enabled, "smi_llm_engine_stamps: engine not built");
  const int n = 3 * L->cfg.num_layers * 16;
  SMI_REQUIRE(cap >= n, "smi_llm_engine_stamps: out holds %d values, %d needed", cap, n);
  std::vector<unsigned long long> h((size_t)n);
  SMI_HIP(hipDeviceSynchronize());
  SMI_HIP(hipMemcpy(h.data(), L->eng.stamps, (size_t)n * 8, hipMemcpyDeviceToHost));
  unsigned long long t0 = ~0ull;
  for (int i = 0; i < n; ++i) if (h[i] && h[i] < t0) t0 = h[i];
  for (int i = 0; i < n; ++i) out[i] = h[i] ? (double)(h[i] - t0) * 0.01 : -1.0;
  return SMI_OK;
}
#endif   // SMI_DIAG

}  // extern "C"
