// Audio front / back end on the device (include/sparkmi.h, smi_rs_*): a polyphase resampler with scipy.signal.resample_poly's
// arithmetic, and the voice prompt's preparation -- resample, volume normalize, reference clip -- written straight into the
// buffers smi_enc_forward_rows reads.
//
//   k_rs_rows    grid (tiles of RS_TILE output samples, rows).  A block stages its row's taps and the input window of its tile
//                in LDS (coalesced reads of x), then every thread sums RS_TILE / RS_BLOCK output samples: ascending j, fp32, one
//                accumulator, product and sum rounded separately (-ffp-contract=off).  A sample's bits depend on its row's
//                samples and ratio alone: not on the tile size, the strides, the row's place or the other rows.
//   k_rs_prompt  one block per row: peak, exact rank selection (radix select on the bit patterns of |x|, three digits of
//                11 / 11 / 9 bits), a fixed-point sum of the selected range in 64-bit integers (every |x| > 0.01 is a multiple of
//                2^-30, so the sum is exact and its order does not matter), the combined gain in float64, the scaled samples and
//                the tiled reference clip.  Only integer LDS atomics: no floating-point atomic anywhere.
//   k_join_rows  the stream joiner (smi_join_*), grid as k_rs_rows: the overlapping chunks of streamed requests become one
//                contiguous stream per request, cross-faded in float64 and resampled with k_rs_rows' own sums (rs_tile_sums);
//                a block assembles its input window in LDS from the stream's history, the fade region and the chunk's body.
//                Tails and histories live in two sets a stream uses in turn, so one launch reads its state and writes the next.
//   k_trim_scan, k_trim_bounds   the speech bounds of rows (smi_trim_rows): window energies in float64, summed from LDS; no atomics.
//   k_concat_rows                trimmed rows into one waveform with gaps and faded edges (smi_concat_rows): one launch.
//   k_loud_seg, k_loud_carry, k_loud_energy, k_loud_gate   programme loudness of rows (smi_loud_rows; BS.1770 K-weighting and
//                gates) and the gain to a target: the serial filter is cut into segments of LD_SEG samples, one lane each, that
//                run from zero state; one wave per row carries the true states across; a second pass sums y^2.  No atomics.
//   k_gain_rows                  rows times their gain, read from the device (smi_gain_rows).
//   k_limit_win, k_limit_env, k_limit_apply, k_limit_stats   the look-ahead true-peak limiter of rows (smi_limit_rows), feed-forward
//                and float64: the envelope of the 4x oversampled span and the required gain from a tile staged in LDS; then, per
//                tile, the sliding minimum formed in LDS in place by doubling, the FIR smoothing of the reduction, the product and
//                the clamp; the window arrives as kernel arguments, the tiles' extremes are reduced one block a row.  No atomics.
//   k_tempo_search, k_tempo_ola  pitch-preserving time-scale change of rows (smi_tempo_rows; WSOLA): one block per row walks the
//                frames in order and, where a frame is searched, stages the quantised target and candidate samples in LDS as
//                int16 and sums exact squared differences in 64-bit integers; the overlap-add is then parallel.  No atomics.
//   k_pitch_ola                  the pitch shift of rows (smi_pitch_rows), behind k_tempo_search: a block computes the stretched
//                samples of its tile's window with tp_ola straight into LDS and resamples them with rs_tile_sums; the stretched
//                signal never reaches memory.  No atomics.
//   k_tempos_search, k_tempos_ola  the time-scale change for joined streams (smi_tempos_*): the frames a push makes final, walked over the
//                stream's history followed by its new chunk with the batch kernels' own device functions (tp_place, tp_ola);
//                histories and last places live in two sets a stream uses in turn, as the joiner's state does.
//   k_pitchs_ola                 the pitch shift of joined streams (smi_pitchs_*), behind k_tempos_search: k_pitch_ola's window of
//                stretched samples in LDS, filled from the stream's stored tail and with tp_ola over history and chunk, summed with
//                rs_tile_sums; the tail the next outputs still reach is the only stretched signal in memory.  No atomics.
//   k_louds_seg, k_louds_carry, k_louds_energy, k_louds_knots, k_louds_apply   loudness of joined streams (smi_louds_*): the
//                batch filter launches over a stream's held input followed by its new chunk, from the stream's carried state,
//                with the batch kernels' own device functions (ld_step, the block sums); one block per row then closes hops and
//                blocks and walks the row's new gain knots in order; the last launch writes the pieces and the next held input.
//                Everything a push is follows from the stream's length before it (ls_plan, host and device).  No atomics.
//   k_limits_env, k_limits_apply, k_limits_stats   the limiter of joined streams (smi_limits_*): the batch launches over a
//                stream's held input followed by its new chunk, with the batch kernels' own device functions (lm_env, lm_req,
//                lm_smooth, lm_out), for the samples that nothing still to come can change; the apply launch also writes the
//                next held input, the stats launch carries max e, min s and the count.  r is computed anew, never carried.
//                Everything a push is follows from the stream's length before it (lt_plan, host and device).  No atomics.
#include <limits.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "smi_common.h"

#define RS_MAX_ROWS 64          // rows of one call: their descriptors travel as kernel arguments
#define RS_TILE 1024            // output samples a block
#define RS_BLOCK 256
#define RS_LDS_FLOATS 16384     // taps + input window of one tile: 64 KiB of LDS
#define RS_POOL_FLOATS (1 << 18)
#define RS_MAX_SAMPLES (1 << 24)
#define JN_MAX_STREAMS 4096     // slots of one smi_join handle
#define PR_BLOCK 1024
#define PR_BINS 2048
#define TR_TILE 64              // windows a block of k_trim_scan
#define TR_BLOCK 256
#define TR_LDS_FLOATS (RS_LDS_FLOATS - 64)   // samples of one tile; the block's few words of static LDS fit beside them in 64 KiB
#define CC_TILE 1024            // output samples a block of k_concat_rows
#define LD_SEG 128              // samples one lane filters in a row (smi_loud_rows): a constant of the arithmetic, never of the call
#define LD_LANES 64             // segments a block of k_loud_seg / k_loud_energy: one wave
#define LD_TILE (LD_SEG * LD_LANES)
#define LD_PITCH (LD_SEG + 1)   // floats between two segments in LDS
#define LD_GATE 256             // threads of k_loud_gate
#define GN_TILE 1024            // samples a block of k_gain_rows
#define LM_TILE 1024            // samples a block of k_limit_env / k_limit_apply
#define LM_HALO 10              // H / phases: the samples the interpolator reaches on either side
#define LM_MAX_PHASES 8
#define LM_MAX_TAPS (2 * LM_HALO * LM_MAX_PHASES + 1)
#define LM_MAX_A 256            // the look-ahead
#define LM_MAX_R 2048           // the release
#define LM_WIN_PAD 2312         // float64 elements at the head of work_dev that hold the window (A + R + 1 <= 2305)
#define LM_WIN_ARG 384          // weights one k_limit_win launch carries as kernel arguments
#define LM_QPT ((LM_TILE + 2 * (LM_MAX_A + LM_MAX_R) + RS_BLOCK - 1) / RS_BLOCK)   // LDS entries a thread of k_limit_apply at most
#define TP_BLOCK 512           // threads of k_tempo_search: a candidate each, the usual 2 D + 1 = 481 in one round
#define TP_TILE 1024            // output samples a block of k_tempo_ola
#define TP_MAX_N 2048           // the frame
#define TP_MAX_D 1024           // the search radius
#define TP_MAX_OUT (1 << 26)    // 4 * RS_MAX_SAMPLES: the longest output row

namespace {

struct RsRow {
  int32_t n_in, n_out, up, down, tap_off, half;   // half = H: taps h[0 .. 2H]
};
struct RsArgs {
  RsRow r[RS_MAX_ROWS];
};
struct PrRow {
  int32_t n_out, ref_len;
};
struct PrArgs {
  PrRow r[RS_MAX_ROWS];
};

struct Filter {
  int up, down, half, tap_off;
};

// first and last input index of output sample k's sum (the last one before clamping to the row); kd = k * down < 2^31 and
// H < 2^14 (both checked on the host), so 32-bit unsigned arithmetic holds every intermediate
__device__ __forceinline__ int rs_jlo(int kd, int up, int half) {
  const int a = kd - half;
  return a <= 0 ? 0 : (int)(((uint32_t)a + (uint32_t)up - 1u) / (uint32_t)up);
}
__device__ __forceinline__ int rs_jhi(int kd, int up, int half) { return (int)(((uint32_t)kd + (uint32_t)half) / (uint32_t)up); }

// input samples a tile's window may span, for sizing the LDS
inline long long rs_window(int up, int down, int half) { return ((long long)(RS_TILE - 1) * down + 2LL * half) / up + 3; }

// The sums of one tile, shared by k_rs_rows and k_join_rows: output k_first + i goes to y[i], i < n_write; an output at or past
// n_out is a zero.  xw[0] is input sample j0 of the row (or of the joined stream), jmax the last input sample there is.
__device__ __forceinline__ void rs_tile_sums(const float* ht, const float* xw, int j0, int jmax, int k_first, int n_out, int up, int down,
                                             int half, float* __restrict__ y, int n_write) {
  for (int i = threadIdx.x; i < n_write; i += RS_BLOCK) {
    const int k = k_first + i;
    float acc = 0.f;
    if (k < n_out) {
      const int kd = k * down;
      const int jl = rs_jlo(kd, up, half);
      const int jh = min(rs_jhi(kd, up, half), jmax);
      int t = half + kd - jl * up;   // tap of the first term, in [0, 2H]
      const int w = jl - j0;
      const int n = jh - jl + 1;
      for (int m = 0; m < n; ++m, t -= up) acc = acc + xw[w + m] * ht[t];
    }
    y[i] = acc;
  }
}

__global__ __launch_bounds__(RS_BLOCK) void k_rs_rows(RsArgs a, const float* __restrict__ taps, const float* __restrict__ in,
                                                      long long in_stride, float* __restrict__ out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const RsRow r = a.r[blockIdx.y];
  const long long k0 = (long long)blockIdx.x * RS_TILE;
  if (k0 >= out_stride) return;
  const float* x = in + (size_t)blockIdx.y * in_stride;
  float* y = out + (size_t)blockIdx.y * out_stride;
  const int tid = threadIdx.x;
  if (k0 >= r.n_out) {   // padding past the row's length: zeros
    for (int i = tid; i < RS_TILE && k0 + i < out_stride; i += RS_BLOCK) y[k0 + i] = 0.f;
    return;
  }
  if (r.up == 1 && r.down == 1) {   // a copy
    for (int i = tid; i < RS_TILE && k0 + i < out_stride; i += RS_BLOCK) y[k0 + i] = k0 + i < r.n_out ? x[k0 + i] : 0.f;
    return;
  }
  const int ntaps = 2 * r.half + 1;
  float* ht = rs_lds;
  float* xw = rs_lds + ntaps;
  const int klast = (int)min(k0 + RS_TILE, (long long)r.n_out) - 1;
  const int j0 = rs_jlo((int)k0 * r.down, r.up, r.half);
  const int j1 = min(rs_jhi(klast * r.down, r.up, r.half), r.n_in - 1);
  const int nwin = j1 - j0 + 1;   // <= rs_window(): checked at registration
  const float* h = taps + r.tap_off;
  for (int i = tid; i < ntaps; i += RS_BLOCK) ht[i] = h[i];
  for (int i = tid; i < nwin; i += RS_BLOCK) xw[i] = x[j0 + i];
  __syncthreads();
  rs_tile_sums(ht, xw, j0, r.n_in - 1, (int)k0, r.n_out, r.up, r.down, r.half, y + k0, (int)min((long long)RS_TILE, out_stride - k0));
}

// ---- k_rs_prompt's block-wide helpers (PR_BLOCK threads)
__device__ __forceinline__ uint32_t pr_block_max(uint32_t v, uint32_t* s) {
  for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = 0;
  for (int i = 0; i < PR_BLOCK / 64; ++i) m = max(m, s[i]);
  return m;
}
__device__ __forceinline__ unsigned long long pr_block_sum(unsigned long long v, unsigned long long* s) {
  for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  for (int i = 0; i < PR_BLOCK / 64; ++i) t += s[i];
  return t;
}
// The bin of `hist[0 .. nbins)` that holds rank `rank` (0-based, rank < the histogram's total): res[0] = the bin, res[1] = the
// count below the bin, res[2] = the bin's own count.  nbins = PR_BLOCK or 2 * PR_BLOCK.
__device__ __forceinline__ void pr_find_bin(const uint32_t* hist, int nbins, uint32_t rank, uint32_t* wsum, uint32_t* res) {
  const int per = nbins / PR_BLOCK, tid = threadIdx.x;
  uint32_t c0 = hist[tid * per], c1 = per == 2 ? hist[tid * per + 1] : 0u;
  uint32_t inc = c0 + c1;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
    if ((tid & 63) >= o) inc += u;
  }
  __syncthreads();
  if ((tid & 63) == 63) wsum[tid >> 6] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < (tid >> 6); ++i) base += wsum[i];
  const uint32_t exc = base + inc - (c0 + c1);
  if (rank >= exc && rank < exc + c0 + c1) {   // exactly one thread
    const bool second = rank >= exc + c0;
    res[0] = (uint32_t)(tid * per + (second ? 1 : 0));
    res[1] = second ? exc + c0 : exc;
    res[2] = second ? c1 : c0;
  }
  __syncthreads();
}

// |x| > 0.01 as audio_volume_normalize tests it: on the sample's exact value
__device__ __forceinline__ bool pr_counts(uint32_t bits) { return (double)__uint_as_float(bits) > 0.01; }
// a counted sample as an integer multiple of 2^-30 (exact: the sample's ulp is at least 2^-30)
__device__ __forceinline__ unsigned long long pr_fixed(uint32_t bits) {
  return (unsigned long long)((double)__uint_as_float(bits) * 1073741824.0);
}

__global__ __launch_bounds__(PR_BLOCK) void k_rs_prompt(PrArgs a, int normalize, float* __restrict__ wav, long long wav_stride,
                                                        float* __restrict__ ref, long long ref_stride, double* __restrict__ gain_out) {
  __shared__ uint32_t hist[2][PR_BINS];
  __shared__ uint32_t s32[PR_BLOCK / 64];
  __shared__ unsigned long long s64[PR_BLOCK / 64];
  __shared__ uint32_t res[2][3];
  const PrRow r = a.r[blockIdx.x];
  const int n = r.n_out, tid = threadIdx.x;
  float* x = wav + (size_t)blockIdx.x * wav_stride;
  float* rf = ref + (size_t)blockIdx.x * ref_stride;
  double gain = 1.0;
  if (normalize) {
    // peak and the number of counted samples
    uint32_t pk = 0;
    unsigned long long cnt = 0;
    for (int i = tid; i < n; i += PR_BLOCK) {
      const uint32_t b = __float_as_uint(x[i]) & 0x7FFFFFFFu;
      pk = max(pk, b);
      cnt += pr_counts(b) ? 1u : 0u;
    }
    const double peak = (double)__uint_as_float(pr_block_max(pk, s32));
    const uint32_t nc = (uint32_t)pr_block_sum(cnt, s64);
    if (peak < 0.1) gain = 0.1 / fmax(peak, 1e-3);
    if (nc > 10) {
      const uint32_t lo = (uint32_t)(int)(0.9 * (double)nc), hi = (uint32_t)(int)(0.99 * (double)nc);
      // the patterns at sorted ranks lo and hi - 1, with the counts below them: positive floats order as their bit patterns
      const uint32_t rank[2] = {lo, hi - 1};
      uint32_t prefix[2] = {0, 0}, below[2] = {0, 0}, equal[2] = {0, 0};
      const int shift[3] = {20, 9, 0}, width[3] = {11, 11, 9};
      for (int p = 0; p < 3; ++p) {
        for (int i = tid; i < 2 * PR_BINS; i += PR_BLOCK) (&hist[0][0])[i] = 0;
        __syncthreads();
        const int top = shift[p] + width[p];   // bits at and above `top` are decided
        for (int i = tid; i < n; i += PR_BLOCK) {
          const uint32_t b = __float_as_uint(x[i]) & 0x7FFFFFFFu;
          if (!pr_counts(b)) continue;
          const uint32_t d = (b >> shift[p]) & ((1u << width[p]) - 1u);
          for (int q = 0; q < 2; ++q)
            if (top >= 31 || (b >> top) == (prefix[q] >> top)) atomicAdd(&hist[q][d], 1u);
        }
        __syncthreads();
        for (int q = 0; q < 2; ++q) {
          pr_find_bin(hist[q], 1 << width[p] > PR_BLOCK ? 2 * PR_BLOCK : PR_BLOCK, rank[q] - below[q], s32, res[q]);
          prefix[q] |= res[q][0] << shift[p];
          below[q] += res[q][1];
          equal[q] = res[q][2];
        }
      }
      // the sum of sorted[lo .. hi): everything strictly between the two patterns, plus the copies of each that lie in range
      unsigned long long sum = 0;
      if (prefix[0] == prefix[1]) {
        sum = (unsigned long long)(hi - lo) * pr_fixed(prefix[0]);
      } else {
        unsigned long long part = 0;
        for (int i = tid; i < n; i += PR_BLOCK) {
          const uint32_t b = __float_as_uint(x[i]) & 0x7FFFFFFFu;
          if (b > prefix[0] && b < prefix[1]) part += pr_fixed(b);
        }
        sum = pr_block_sum(part, s64) + (unsigned long long)(below[0] + equal[0] - lo) * pr_fixed(prefix[0]) +
              (unsigned long long)(hi - below[1]) * pr_fixed(prefix[1]);
      }
      const double volume = (double)sum / 1073741824.0 / (double)(hi - lo);
      gain = gain * fmin(fmax(0.2 / volume, 0.1), 10.0);
      const double peak2 = peak * gain;
      if (peak2 > 1.0) gain = gain / peak2;
    }
  }
  if (tid == 0 && gain_out) gain_out[blockIdx.x] = gain;
  // the reference clip first, from the samples as they came (read only), then the samples in place: both are fl32(x * gain)
  for (int i = tid; i < (int)ref_stride; i += PR_BLOCK) rf[i] = i < r.ref_len ? (float)((double)x[i % n] * gain) : 0.f;
  __syncthreads();
  if (normalize)
    for (int i = tid; i < n; i += PR_BLOCK) x[i] = (float)((double)x[i] * gain);
}

// ---- the stream joiner (smi_join_*)
struct JnRow {
  int32_t slot, set;        // the stream's slot; the state set this push reads (it writes the other one)
  int32_t len, n_fade;      // chunk samples; leading samples that are faded with the held tail (0 for a stream's first chunk)
  int32_t n_old, n_new;     // joined samples before / after this push
  int32_t k_old, k_new;     // outputs emitted before / after this push
  int32_t keep;             // 1: the chunk's last `overlap` samples become the held tail
};
struct JnArgs {
  JnRow r[RS_MAX_ROWS];
};
struct JnState {
  float* tail;              // [2][max_streams][overlap]
  float* hist;              // [2][max_streams][hs]: the last hs joined samples, hist[q] = x[N - hs + q]
  const double* fade_in;    // [overlap]
  const double* fade_out;   // [overlap]
  const float* taps;        // [2H + 1]
  int32_t max_streams, overlap, hs, up, down, half;
};

// sample j of the joined stream, n_old - hs <= j < n_new: from the history, the fade region or the chunk's body
__device__ __forceinline__ float jn_sample(int j, const JnRow& r, int hs, const float* __restrict__ c, const float* __restrict__ hist,
                                           const float* __restrict__ tail, const double* __restrict__ fi, const double* __restrict__ fo) {
  if (j < r.n_old) return hist[j - (r.n_old - hs)];
  const int q = j - r.n_old;
  const float a = c[q];
  if (q < r.n_fade) return (float)((double)a * fi[q] + (double)tail[q] * fo[q]);
  return a;
}

// grid (tiles of RS_TILE output samples, rows), as k_rs_rows.  Block (t, b) assembles the window of its tile from the stream's
// history, the fade region and the chunk's body in LDS and sums its outputs with k_rs_rows' loop; tile 0 of a row also writes
// the stream's next state -- tail and history -- into the state set this launch does not read.
__global__ __launch_bounds__(RS_BLOCK) void k_join_rows(JnArgs a, JnState s, const float* __restrict__ in, long long in_stride,
                                                        float* __restrict__ out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const JnRow r = a.r[blockIdx.y];
  const long long k0 = (long long)blockIdx.x * RS_TILE;   // of this push's piece
  if (k0 >= out_stride) return;
  const int tid = threadIdx.x;
  const float* c = in + (size_t)blockIdx.y * in_stride;
  float* y = out + (size_t)blockIdx.y * out_stride;
  const size_t per_t = (size_t)s.max_streams * s.overlap, per_h = (size_t)s.max_streams * s.hs;
  const float* tail = s.tail + r.set * per_t + (size_t)r.slot * s.overlap;
  const float* hist = s.hist + r.set * per_h + (size_t)r.slot * s.hs;
  if (blockIdx.x == 0) {   // the next state, from what this launch only reads
    float* tail2 = s.tail + (1 - r.set) * per_t + (size_t)r.slot * s.overlap;
    float* hist2 = s.hist + (1 - r.set) * per_h + (size_t)r.slot * s.hs;
    if (r.keep)
      for (int q = tid; q < s.overlap; q += RS_BLOCK) tail2[q] = c[r.len - s.overlap + q];
    for (int q = tid; q < s.hs; q += RS_BLOCK) {
      const int j = r.n_new - s.hs + q;
      hist2[q] = j < 0 ? 0.f : jn_sample(j, r, s.hs, c, hist, tail, s.fade_in, s.fade_out);
    }
  }
  const int n_piece = r.k_new - r.k_old;
  const int n_write = (int)min((long long)RS_TILE, out_stride - k0);
  if (k0 >= n_piece) {   // padding past the piece: zeros
    for (int i = tid; i < n_write; i += RS_BLOCK) y[k0 + i] = 0.f;
    return;
  }
  if (s.up == 1 && s.down == 1) {   // the join alone: k_old = n_old
    for (int i = tid; i < n_write; i += RS_BLOCK)
      y[k0 + i] = k0 + i < n_piece ? jn_sample(r.n_old + (int)k0 + i, r, s.hs, c, hist, tail, s.fade_in, s.fade_out) : 0.f;
    return;
  }
  const int ntaps = 2 * s.half + 1;
  float* ht = rs_lds;
  float* xw = rs_lds + ntaps;
  const int kf = r.k_old + (int)k0;                                  // of the stream
  const int klast = min(kf + RS_TILE, r.k_new) - 1;
  const int j0 = rs_jlo(kf * s.down, s.up, s.half);                 // >= n_old - hs: checked on the host
  const int j1 = min(rs_jhi(klast * s.down, s.up, s.half), r.n_new - 1);
  const int nwin = j1 - j0 + 1;   // <= rs_window(): checked at creation
  for (int i = tid; i < ntaps; i += RS_BLOCK) ht[i] = s.taps[i];
  for (int i = tid; i < nwin; i += RS_BLOCK) xw[i] = jn_sample(j0 + i, r, s.hs, c, hist, tail, s.fade_in, s.fade_out);
  __syncthreads();
  rs_tile_sums(ht, xw, j0, r.n_new - 1, kf, r.k_new, s.up, s.down, s.half, y + k0, n_write);
}

// ---- speech bounds of rows (smi_trim_*) and assembly of trimmed rows (smi_concat_*)
struct TrArgs {
  int32_t n[RS_MAX_ROWS];
};

// grid (tiles of TR_TILE windows, rows).  A block stages the samples its windows span in LDS once (coalesced), then each of its
// four waves sums whole windows from there: lane l adds the exact float64 squares of samples l, l + 64, ... of the window in
// ascending order, and the 64 partial sums meet in a fixed xor butterfly -- a window's sum depends on its samples alone.  The
// block writes the first and the last speech window of its tile (INT_MAX / -1: none) to work[row][tile]: no atomics, no state.
__global__ __launch_bounds__(TR_BLOCK) void k_trim_scan(TrArgs a, const float* __restrict__ in, long long in_stride, int W, int s,
                                                        double level, int tiles, int32_t* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  __shared__ int32_t wf[TR_BLOCK / 64], wl[TR_BLOCK / 64];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n[b];
  const int nwin = n >= W ? (n - W) / s + 1 : 0;
  const int i0 = t * TR_TILE;
  int first = INT_MAX, last = -1;
  if (i0 < nwin) {
    const int cnt = min(TR_TILE, nwin - i0);
    const float* x = in + (size_t)b * in_stride + (size_t)i0 * s;
    const int span = (cnt - 1) * s + W;   // i0 s + span <= n; span <= TR_LDS_FLOATS: checked on the host
    for (int i = tid; i < span; i += TR_BLOCK) rs_lds[i] = x[i];
    __syncthreads();
    for (int w = wave; w < cnt; w += TR_BLOCK / 64) {
      const float* p = rs_lds + w * s;
      double acc = 0.0;
      for (int q = lane; q < W; q += 64) {
        const double v = (double)p[q];
        acc = acc + v * v;
      }
      for (int o = 32; o; o >>= 1) acc = acc + __shfl_xor(acc, o);
      if (acc >= level) {   // (the same in every lane: the butterfly's sums are bitwise equal)
        first = min(first, i0 + w);
        last = i0 + w;
      }
    }
  }
  if (lane == 0) { wf[wave] = first; wl[wave] = last; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < TR_BLOCK / 64; ++i) { first = min(first, wf[i]); last = max(last, wl[i]); }
    work[2 * ((size_t)b * tiles + t)] = first;
    work[2 * ((size_t)b * tiles + t) + 1] = last;
  }
}

// one wave per row: the tiles' results become the row's bounds
__global__ __launch_bounds__(64) void k_trim_bounds(TrArgs a, int W, int s, int margin, int tiles, const int32_t* __restrict__ work,
                                                    int32_t* __restrict__ bounds) {
  const int b = blockIdx.x, n = a.n[b];
  int first = INT_MAX, last = -1;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    first = min(first, work[2 * ((size_t)b * tiles + t)]);
    last = max(last, work[2 * ((size_t)b * tiles + t) + 1]);
  }
  for (int o = 32; o; o >>= 1) {
    first = min(first, __shfl_xor(first, o));
    last = max(last, __shfl_xor(last, o));
  }
  if (threadIdx.x) return;
  int lo = 0, hi = 0;
  if (n < W) hi = n;
  else if (last >= 0) {
    lo = (int)max(0LL, (long long)first * s - margin);
    hi = (int)min((long long)n, (long long)last * s + margin);
  }
  bounds[2 * b] = lo;
  bounds[2 * b + 1] = hi;
}

struct CcRow {
  int32_t src, len, off, lead, fade;   // first sample of the piece in its row; its length; its place in `out`; zeros before it; f'
};
struct CcArgs {
  CcRow r[RS_MAX_ROWS];
};

// grid (tiles of CC_TILE samples, B + 1).  Row b < B writes piece b's span of `out`: its gap, then the piece, the first and the
// last f' samples weighted.  Row B writes the zeros from the total length to cap.
__global__ __launch_bounds__(RS_BLOCK) void k_concat_rows(CcArgs a, int B, const float* __restrict__ in, long long in_stride,
                                                          float* __restrict__ out, long long total, long long cap) {
  const int b = blockIdx.y;
  const long long k0 = (long long)blockIdx.x * CC_TILE;
  if (b == B) {
    for (long long k = total + k0 + threadIdx.x; k < min(cap, total + k0 + CC_TILE); k += RS_BLOCK) out[k] = 0.f;
    return;
  }
  const CcRow r = a.r[b];
  if (r.len == 0 || k0 >= (long long)r.lead + r.len) return;
  const float* p = in + (size_t)b * in_stride + r.src;
  float* y = out + ((long long)r.off - r.lead);
  const double den = (double)(r.fade + 1);
  const int end = (int)min((long long)r.lead + r.len, k0 + CC_TILE);
  for (int k = (int)k0 + threadIdx.x; k < end; k += RS_BLOCK) {
    float v = 0.f;
    if (k >= r.lead) {
      const int q = k - r.lead;
      const int e = min(q, r.len - 1 - q);   // distance to the nearer edge
      v = p[q];
      if (e < r.fade) v = (float)((double)v * ((double)(e + 1) / den));
    }
    y[k] = v;
  }
}

// ---- programme loudness of rows and the gain that brings them to a target (smi_loud_rows, smi_gain_rows)
struct LdRow {
  int32_t n, start, len;   // the row's samples; the span x[start .. start + len)
};
struct LdArgs {
  LdRow r[RS_MAX_ROWS];
};
struct LdCoef {
  double b[2][3], a1[2], a2[2];   // the two biquads of the K-weighting
  double T[4][4];                 // zero-input transition of the cascade's state over LD_SEG steps (ld_transition)
};
struct LdTargets {
  double t[RS_MAX_ROWS];
};
struct LdLayout {                 // float64 offsets into a row's part of work_dev
  long long row, e, s, pk, parts, hops;
  int32_t pps;                    // hop parts a segment can hold: (LD_SEG - 1) / hop + 2
};
// the cascade in direct form I: the last two inputs, the last two outputs of stage 1 and of stage 2
struct LdState {
  double x1, x2, p1, p2, q1, q2;
};

// One sample through both biquads: every product and sum rounded on its own, in this order.  The previous output enters last,
// so the chain from sample to sample is one product and one difference a stage.
__host__ __device__ __forceinline__ double ld_step(const LdCoef& c, LdState& s, double v) {
  const double w = ((c.b[0][0] * v + c.b[0][1] * s.x1) + c.b[0][2] * s.x2) - c.a2[0] * s.p2;
  const double y = w - c.a1[0] * s.p1;
  const double u = ((c.b[1][0] * y + c.b[1][1] * s.p1) + c.b[1][2] * s.p2) - c.a2[1] * s.q2;
  const double o = u - c.a1[1] * s.q1;
  s.x2 = s.x1; s.x1 = v;
  s.p2 = s.p1; s.p1 = y;
  s.q2 = s.q1; s.q1 = o;
  return o;
}

// T[.][i]: where unit state i stands after LD_SEG samples of silence (the input history is zero too)
inline void ld_transition(LdCoef& c) {
  for (int i = 0; i < 4; ++i) {
    LdState s = {0.0, 0.0, i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0, i == 3 ? 1.0 : 0.0};
    for (int t = 0; t < LD_SEG; ++t) ld_step(c, s, 0.0);
    c.T[0][i] = s.p1; c.T[1][i] = s.p2; c.T[2][i] = s.q1; c.T[3][i] = s.q2;
  }
}

// A block of one wave stages its tile -- LD_LANES segments of LD_SEG samples -- in LDS with coalesced reads; lane l then walks
// segment l at lds[l * LD_PITCH ..] (the odd pitch puts the 64 lanes on 64 banks).  Returns the samples of this lane's segment
// (0: none) and sets the input history from the two samples before it; the span's first segment starts from silence.
__device__ __forceinline__ int ld_stage(const LdRow& r, const float* __restrict__ x, float* lds, LdState& s) {
  const int t0 = blockIdx.x * LD_TILE, tid = threadIdx.x;
  const int cnt = min(LD_TILE, r.len - t0);
  for (int i = tid; i < cnt; i += LD_LANES) lds[(i / LD_SEG) * LD_PITCH + (i % LD_SEG)] = x[t0 + i];
  __syncthreads();
  const int i0 = t0 + tid * LD_SEG;
  s.x1 = i0 >= 1 && i0 < r.len ? (double)x[i0 - 1] : 0.0;
  s.x2 = i0 >= 2 && i0 < r.len ? (double)x[i0 - 2] : 0.0;
  return max(0, min(LD_SEG, r.len - i0));
}

// grid (tiles of LD_TILE samples, rows): every segment but the row's last from zero state; its end state goes to E[segment]
__global__ __launch_bounds__(LD_LANES) void k_loud_seg(LdArgs a, LdCoef c, const float* __restrict__ in, long long in_stride,
                                                       double* __restrict__ work, LdLayout lay) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const LdRow r = a.r[blockIdx.y];
  if ((long long)blockIdx.x * LD_TILE >= r.len) return;
  LdState s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ld_stage(r, in + (size_t)blockIdx.y * in_stride + r.start, rs_lds, s);
  const int k = blockIdx.x * LD_LANES + threadIdx.x;
  const int nseg = (r.len + LD_SEG - 1) / LD_SEG;
  if (k >= nseg - 1) return;   // (the last segment's end is nobody's start; every other segment is whole)
  const float* seg = rs_lds + threadIdx.x * LD_PITCH;
  for (int t = 0; t < LD_SEG; ++t) ld_step(c, s, (double)seg[t]);
  double* E = work + (size_t)blockIdx.y * lay.row + lay.e + 4 * (size_t)k;
  E[0] = s.p1; E[1] = s.p2; E[2] = s.q1; E[3] = s.q2;
}

// one wave per row: S[0] = 0, S[k + 1] = T S[k] + E[k].  The wave stages 64 end states in LDS at a time; every lane runs the
// same recurrence from there and lane t keeps S[k0 + t], so the stores are coalesced.
__global__ __launch_bounds__(64) void k_loud_carry(LdArgs a, LdCoef c, double* __restrict__ work, LdLayout lay) {
  __shared__ double e[64][4];
  const LdRow r = a.r[blockIdx.x];
  const int nseg = (r.len + LD_SEG - 1) / LD_SEG, lane = threadIdx.x;
  const double* E = work + (size_t)blockIdx.x * lay.row + lay.e;
  double* S = work + (size_t)blockIdx.x * lay.row + lay.s;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int k0 = 0; k0 < nseg; k0 += 64) {
    if (k0 + lane < nseg - 1)
      for (int i = 0; i < 4; ++i) e[lane][i] = E[4 * (size_t)(k0 + lane) + i];
    __syncthreads();
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    const int cnt = min(64, nseg - k0);
    for (int t = 0; t < cnt; ++t) {
      if (lane == t) { m0 = s0; m1 = s1; m2 = s2; m3 = s3; }
      if (k0 + t < nseg - 1) {
        const double n0 = (((c.T[0][0] * s0 + c.T[0][1] * s1) + c.T[0][2] * s2) + c.T[0][3] * s3) + e[t][0];
        const double n1 = (((c.T[1][0] * s0 + c.T[1][1] * s1) + c.T[1][2] * s2) + c.T[1][3] * s3) + e[t][1];
        const double n2 = (((c.T[2][0] * s0 + c.T[2][1] * s1) + c.T[2][2] * s2) + c.T[2][3] * s3) + e[t][2];
        const double n3 = (((c.T[3][0] * s0 + c.T[3][1] * s1) + c.T[3][2] * s2) + c.T[3][3] * s3) + e[t][3];
        s0 = n0; s1 = n1; s2 = n2; s3 = n3;
      }
    }
    if (lane < cnt) {
      double* d = S + 4 * (size_t)(k0 + lane);
      d[0] = m0; d[1] = m1; d[2] = m2; d[3] = m3;
    }
    __syncthreads();
  }
}

// grid as k_loud_seg: every segment again, from its true start state.  y^2 is summed in ascending sample order into one sum per
// hop part -- the piece of a hop that lies in this segment -- and written to P[segment][part]; max |x| of the segment to PK.
__global__ __launch_bounds__(LD_LANES) void k_loud_energy(LdArgs a, LdCoef c, int hop, const float* __restrict__ in, long long in_stride,
                                                          double* __restrict__ work, LdLayout lay) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const LdRow r = a.r[blockIdx.y];
  if ((long long)blockIdx.x * LD_TILE >= r.len) return;
  LdState s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int m = ld_stage(r, in + (size_t)blockIdx.y * in_stride + r.start, rs_lds, s);
  if (m == 0) return;
  const int k = blockIdx.x * LD_LANES + threadIdx.x;
  double* row = work + (size_t)blockIdx.y * lay.row;
  const double* S = row + lay.s + 4 * (size_t)k;
  s.p1 = S[0]; s.p2 = S[1]; s.q1 = S[2]; s.q2 = S[3];
  double* P = row + lay.parts + (size_t)k * lay.pps;
  const float* seg = rs_lds + threadIdx.x * LD_PITCH;
  int i = k * LD_SEG;                    // of the span
  int edge = (i / hop + 1) * hop;        // where the hop that holds sample i ends
  int p = 0, held = 0;
  double acc = 0.0;
  uint32_t pk = 0;
  for (int t = 0; t < m; ++t) {
    const float v = seg[t];
    pk = max(pk, __float_as_uint(v) & 0x7FFFFFFFu);
    const double o = ld_step(c, s, (double)v);
    acc = acc + o * o;
    held = 1;
    if (++i == edge) {
      P[p++] = acc;
      acc = 0.0;
      held = 0;
      edge += hop;
    }
  }
  if (held) P[p] = acc;
  row[lay.pk + k] = (double)__uint_as_float(pk);
}

// ---- k_loud_gate's block-wide sums (LD_GATE threads): a fixed tree, the same whatever the grid
__device__ __forceinline__ double ld_block_sum(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = LD_GATE / 2; o; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}
__device__ __forceinline__ double ld_block_max(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = LD_GATE / 2; o; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
    __syncthreads();
  }
  return s[0];
}
// mean square of block j (of the whole span where it is shorter than a block)
__device__ __forceinline__ double ld_z(const double* H, int j, int len, int block, int nh) {
  if (len >= block) return (((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / (double)block;
  double t = 0.0;
  for (int h = 0; h < nh; ++h) t = t + H[h];
  return t / (double)len;
}

// one block per row: hop parts into hops (ascending), hops into blocks, both gates, the loudness, the gain and its limits.
// Thread t sums the blocks j = t, t + LD_GATE, ... in ascending order, then the fixed tree: a sum depends on the row alone.
__global__ __launch_bounds__(LD_GATE) void k_loud_gate(LdArgs a, LdTargets tg, int block, double abs_gate, double max_gain_db, double ceiling,
                                                       double* __restrict__ work, LdLayout lay, double* __restrict__ stats) {
  __shared__ double red[LD_GATE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const LdRow r = a.r[b];
  const int len = r.len, hop = block / 4;
  double* row = work + (size_t)b * lay.row;
  double* H = row + lay.hops;
  const double* P = row + lay.parts;
  const int nh = (int)(((long long)len + hop - 1) / hop);
  const int nseg = (len + LD_SEG - 1) / LD_SEG;
  for (int h = tid; h < nh; h += LD_GATE) {
    const long long lo = (long long)h * hop, hi = min((long long)len, lo + hop) - 1;
    double t = 0.0;
    for (int k = (int)(lo / LD_SEG); k <= (int)(hi / LD_SEG); ++k) t = t + P[(size_t)k * lay.pps + (h - (int)(((long long)k * LD_SEG) / hop))];
    H[h] = t;
  }
  double pk = 0.0;
  for (int k = tid; k < nseg; k += LD_GATE) pk = fmax(pk, row[lay.pk + k]);
  const double peak = ld_block_max(pk, red);   // (its barriers also publish H to the block)
  const int nblk = len >= block ? (len - block) / hop + 1 : (len >= 1 ? 1 : 0);
  double sum = 0.0, cnt = 0.0;
  for (int j = tid; j < nblk; j += LD_GATE) {
    const double z = ld_z(H, j, len, block, nh);
    if (z > abs_gate) { sum = sum + z; cnt = cnt + 1.0; }
  }
  const double sum1 = ld_block_sum(sum, red), cnt1 = ld_block_sum(cnt, red);
  double sum2 = sum1, cnt2 = cnt1;
  if (len >= block && cnt1 > 0.0) {
    const double rel = 0.1 * (sum1 / cnt1);
    sum = 0.0; cnt = 0.0;
    for (int j = tid; j < nblk; j += LD_GATE) {
      const double z = ld_z(H, j, len, block, nh);
      if (z > abs_gate && z > rel) { sum = sum + z; cnt = cnt + 1.0; }
    }
    sum2 = ld_block_sum(sum, red);
    cnt2 = ld_block_sum(cnt, red);
  }
  if (tid) return;
  double loud = -INFINITY, g = 1.0, limit = 0.0;
  if (cnt2 > 0.0) {
    loud = -0.691 + 10.0 * log10(sum2 / cnt2);
    const double target = tg.t[b];
    if (target == target) {   // (a NaN target: measure only)
      g = pow(10.0, (target - loud) / 20.0);
      const double gmax = pow(10.0, max_gain_db / 20.0);
      if (g > gmax) { g = gmax; limit = 1.0; }
      if (g * peak > ceiling) { g = ceiling / peak; limit = 2.0; }
    }
  }
  double* st = stats + 4 * (size_t)b;
  st[0] = loud; st[1] = peak; st[2] = g; st[3] = limit;
}

// grid (tiles of GN_TILE samples, rows): the span times the row's gain, the rest of the row as it is, zeros from n to the stride
__global__ __launch_bounds__(RS_BLOCK) void k_gain_rows(LdArgs a, const double* __restrict__ stats, const float* in, long long in_stride,
                                                        float* out, long long out_stride) {
  const LdRow r = a.r[blockIdx.y];
  const double g = stats[4 * (size_t)blockIdx.y + 2];
  const float* x = in + (size_t)blockIdx.y * in_stride;
  float* y = out + (size_t)blockIdx.y * out_stride;
  const long long k0 = (long long)blockIdx.x * GN_TILE;
  const long long end = min(out_stride, k0 + GN_TILE);
  for (long long i = k0 + threadIdx.x; i < end; i += RS_BLOCK) {
    float v = 0.f;
    if (i < r.n) {
      v = x[i];
      if (i >= r.start && i < (long long)r.start + r.len) v = (float)((double)v * g);
    }
    y[i] = v;
  }
}

// ---- look-ahead true-peak limiter of rows (smi_limit_rows): feed-forward, float64, every product and sum rounded on its own
struct LmTaps {
  double h[LM_MAX_TAPS];   // the interpolator, h[0 .. 2H], H = LM_HALO * phases
  int32_t n, phases;       // n = 0: the sample-peak mode
};
struct LmWin {
  double w[LM_WIN_ARG];
};
struct LmLayout {          // float64 offsets into work_dev: the window, then a part per row (r, then three values a tile)
  long long rows, row, emax, smin, cnt;
};

// the smoothing window travels as kernel arguments, LM_WIN_ARG weights a launch: nothing is copied and nothing waits
__global__ __launch_bounds__(RS_BLOCK) void k_limit_win(LmWin w, int cnt, double* __restrict__ dst) {
  for (int i = threadIdx.x; i < cnt; i += RS_BLOCK) dst[i] = w.w[i];
}

// block-wide max / min / sum over RS_BLOCK threads; max and min are exact in any order, the sum is one of small integers
template <int OP>
__device__ __forceinline__ double lm_block_red(double v, double* s) {
  __syncthreads();
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = RS_BLOCK / 2; o; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double p = s[threadIdx.x], q = s[threadIdx.x + o];
      s[threadIdx.x] = OP == 0 ? fmax(p, q) : (OP == 1 ? fmin(p, q) : p + q);
    }
    __syncthreads();
  }
  return s[0];
}

// The per-sample arithmetic of the limiter, shared by the batch kernels and the stream kernels (k_limits_*), so that the two
// forms cannot differ in a bit.
// e of the sample xc points at, in a staged tile with LM_HALO samples on either side: the phases' sums in ascending d.  h is
// indexed like the taps (kernel arguments in the batch form, device memory in the stream form); tp false: the sample peak.
template <class Taps>
__device__ __forceinline__ double lm_env(const Taps& h, int P, bool tp, const float* xc) {
  double e = fabs((double)xc[0]);
  if (tp) {
    const int H = LM_HALO * P;
    for (int k = 1; k < P; ++k) {
      double u = 0.0;
      for (int d = -LM_HALO; d < LM_HALO; ++d) u = u + h[P * d + k + H] * (double)xc[-d];   // (every tap of phase k)
      e = fmax(e, fabs(u));
    }
  }
  return e;
}
// the required gain r of a sample with envelope e
__device__ __forceinline__ double lm_req(double g, double e, double ceiling) {
  const double v = g * e;
  return v > ceiling ? ceiling / v : 1.0;
}
// q[0 .. LM_TILE + 2 W), W = A + R, holds r over a tile's samples and W more on either side (1 where there is none).  The
// forward minimum over W + 1 entries is formed in place by doubling -- every thread reads its entries of a round into registers
// before any is written --, so F[i] = min r[i .. i + W] and m[j] = F[j - R]; the entries become the reductions 1 - m; a thread
// then sums its samples' windows in ascending k.  s[u] receives s of the tile's sample threadIdx.x + u RS_BLOCK.  Every thread
// of the block calls this.
__device__ __forceinline__ void lm_smooth(double* q, int A, int R, const double* __restrict__ win, double (&s)[LM_TILE / RS_BLOCK]) {
  const int W = A + R, nq = LM_TILE + 2 * W, tid = threadIdx.x;
  __syncthreads();
  double own[LM_TILE / RS_BLOCK];
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) own[u] = q[W + tid + u * RS_BLOCK];
  int cur = 1;
  while (cur < W + 1) {   // F over `cur` entries -> over min(2 cur, W + 1)
    const int off = 2 * cur <= W + 1 ? cur : W + 1 - cur;
    double t[LM_QPT];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < LM_QPT; ++u) {
      const int i = tid + u * RS_BLOCK;
      t[u] = i < nq ? (i + off < nq ? fmin(q[i], q[i + off]) : q[i]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < LM_QPT; ++u) {
      const int i = tid + u * RS_BLOCK;
      if (i < nq) q[i] = t[u];
    }
    cur += off;
  }
  __syncthreads();
  for (int i = tid; i < nq; i += RS_BLOCK) q[i] = 1.0 - q[i];
  __syncthreads();
  double acc[LM_TILE / RS_BLOCK];
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) acc[u] = 0.0;
  const double* qc = q + tid + A;   // m[j - k] of the tile's sample c lies at q[c + A - k]
  for (int k = -R; k <= A; ++k) {
    const double wk = win[k + R];
#pragma unroll
    for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) acc[u] = acc[u] + wk * qc[u * RS_BLOCK - k];
  }
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) s[u] = fmin(1.0 - acc[u], own[u]);
}
// the product and the clamp
__device__ __forceinline__ float lm_out(float x, double g, double s, float c32) {
  const float v = (float)(((double)x * g) * s);
  return v > c32 ? c32 : (v < -c32 ? -c32 : v);
}

// grid (tiles of LM_TILE samples of the span, rows).  The tile and LM_HALO samples on either side go to LDS with coalesced
// reads (zeros outside the span, which is never read); a thread then takes every RS_BLOCK-th sample: the phases' sums in
// ascending d, the envelope e, and the required gain r to the row's part of work.  The tile's max e goes beside it.
__global__ __launch_bounds__(RS_BLOCK) void k_limit_env(LdArgs a, LmTaps tp, const double* __restrict__ gain, int gain_stride, double ceiling,
                                                        const float* __restrict__ in, long long in_stride, double* __restrict__ work,
                                                        LmLayout lay) {
  __shared__ float xs[LM_TILE + 2 * LM_HALO];
  __shared__ double red[RS_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const LdRow r = a.r[b];
  const int t0 = blockIdx.x * LM_TILE;
  if (t0 >= r.len) return;
  const float* x = in + (size_t)b * in_stride + r.start;
  for (int i = tid; i < LM_TILE + 2 * LM_HALO; i += RS_BLOCK) {
    const int j = t0 - LM_HALO + i;
    xs[i] = j >= 0 && j < r.len ? x[j] : 0.f;
  }
  __syncthreads();
  const double g = gain ? gain[(size_t)b * gain_stride] : 1.0;
  double* row = work + lay.rows + (size_t)b * lay.row;
  const int cnt = min(LM_TILE, r.len - t0);
  double emax = 0.0;
  for (int i = tid; i < cnt; i += RS_BLOCK) {
    const double e = lm_env(tp.h, tp.phases, tp.n != 0, xs + LM_HALO + i);
    row[t0 + i] = lm_req(g, e, ceiling);
    emax = fmax(emax, e);
  }
  emax = lm_block_red<0>(emax, red);
  if (!tid) row[lay.emax + blockIdx.x] = emax;
}

// grid (tiles of LM_TILE samples of the row up to out_stride, rows).  A tile that meets the span stages r over its samples and
// A + R more on either side (1 outside the span) in LDS and smooths them there (lm_smooth).  The
// tile's min s and its count of s < 1 go to work.  in and out may be one buffer: a block reads the samples it writes, no others.
__global__ __launch_bounds__(RS_BLOCK) void k_limit_apply(LdArgs a, int A, int R, const double* __restrict__ gain, int gain_stride, float c32,
                                                          const double* __restrict__ win, const float* in, long long in_stride,
                                                          const double* __restrict__ rq, double* __restrict__ tiles, LmLayout lay,
                                                          float* out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  __shared__ double red[RS_BLOCK];
  double* q = (double*)rs_lds;
  const int b = blockIdx.y, tid = threadIdx.x;
  const LdRow r = a.r[b];
  const float* x = in + (size_t)b * in_stride;
  float* y = out + (size_t)b * out_stride;
  const long long k0 = (long long)blockIdx.x * LM_TILE;
  const bool hit = r.len > 0 && k0 < (long long)r.start + r.len && k0 + LM_TILE > r.start;
  double s[LM_TILE / RS_BLOCK];
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) s[u] = 1.0;
  if (hit) {
    const int W = A + R, nq = LM_TILE + 2 * W;
    const double* rr = rq + (size_t)b * lay.row;
    const long long j0 = k0 - r.start - W;   // the span's index of q[0]
    for (int i = tid; i < nq; i += RS_BLOCK) {
      const long long j = j0 + i;
      q[i] = j >= 0 && j < r.len ? rr[j] : 1.0;
    }
    lm_smooth(q, A, R, win, s);
  }
  const double g = gain ? gain[(size_t)b * gain_stride] : 1.0;
  double smin = 1.0, cnt = 0.0;
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) {
    const long long i = k0 + tid + u * RS_BLOCK;
    if (i >= out_stride) continue;
    float v = 0.f;
    if (i < r.n) {
      v = x[i];
      if (i >= r.start && i < (long long)r.start + r.len) {
        v = lm_out(v, g, s[u], c32);
        smin = fmin(smin, s[u]);
        if (s[u] < 1.0) cnt = cnt + 1.0;
      }
    }
    y[i] = v;
  }
  if (!hit) return;
  smin = lm_block_red<1>(smin, red);
  cnt = lm_block_red<2>(cnt, red);
  if (!tid) {
    double* row = tiles + (size_t)b * lay.row;
    row[lay.smin + blockIdx.x] = smin;
    row[lay.cnt + blockIdx.x] = cnt;
  }
}

// one block per row: the tiles' values into the row's four stats.  max, min and a sum of whole numbers: exact in any order.
__global__ __launch_bounds__(RS_BLOCK) void k_limit_stats(LdArgs a, const double* __restrict__ gain, int gain_stride,
                                                          const double* __restrict__ work, LmLayout lay, double* __restrict__ stats) {
  __shared__ double red[RS_BLOCK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const LdRow r = a.r[b];
  const double* row = work + lay.rows + (size_t)b * lay.row;
  double emax = 0.0, smin = 1.0, cnt = 0.0;
  if (r.len > 0) {
    const int te = (r.len + LM_TILE - 1) / LM_TILE;
    for (int t = tid; t < te; t += RS_BLOCK) emax = fmax(emax, row[lay.emax + t]);
    const int t_lo = r.start / LM_TILE, t_hi = (r.start + r.len - 1) / LM_TILE;
    for (int t = t_lo + tid; t <= t_hi; t += RS_BLOCK) {
      smin = fmin(smin, row[lay.smin + t]);
      cnt = cnt + row[lay.cnt + t];
    }
  }
  emax = lm_block_red<0>(emax, red);
  smin = lm_block_red<1>(smin, red);
  cnt = lm_block_red<2>(cnt, red);
  if (tid) return;
  const double g = gain ? gain[(size_t)b * gain_stride] : 1.0;
  double* st = stats + 4 * (size_t)b;
  st[0] = g * emax; st[1] = g; st[2] = smin; st[3] = cnt;
}

// ---- time-scale change of rows (smi_tempo_rows)
struct TpRow {
  int32_t start, len, p, q, m, frames;   // the span x[start .. start + len); tempo p / q; M output samples in K frames
};
struct TpArgs {
  TpRow r[RS_MAX_ROWS];
};

// Where the tempo kernels read samples: get(i, v) fetches sample i into v where the sequence has one and returns false where it
// has none (such a place reads as 0 and is never fetched).  TpSpan is a row's span (smi_tempo_rows); TsSeq is a stream's history
// followed by its new chunk (smi_tempos_push_rows).
struct TpSpan {
  const float* __restrict__ x;
  int len;
  __device__ __forceinline__ bool get(long long i, float& v) const {
    if (i < 0 || i >= len) return false;
    v = x[i];
    return true;
  }
};

// sample i, quantised for the search: clamp(rint(fl64(x) * 32767), +-32767); 0 where there is no sample and for a NaN
template <class Src>
__device__ __forceinline__ int tp_quant(const Src& x, long long i) {
  float f;
  if (!x.get(i, f)) return 0;
  const double v = (double)f * 32767.0;   // exact: 24 x 15 bits
  if (!(v == v)) return 0;
  return (int)fmin(fmax(rint(v), -32767.0), 32767.0);
}

// the smaller of two (distance, tie key) pairs: the key holds |a + delta - t| above delta + D, so it orders ties as the header does
__device__ __forceinline__ void tp_min(unsigned long long& d, unsigned long long& key, unsigned long long d2, unsigned long long key2) {
  if (d2 < d || (d2 == d && key2 < key)) { d = d2; key = key2; }
}

// s_k of frame k >= 1 from s_{k-1}, by the whole block (TP_BLOCK threads, every one returns it).  A frame whose natural
// continuation lies within D of its nominal place keeps it (what the search would return: distance 0, nothing closer to t_k).
// Any other frame is searched: the block stages qx[t .. t + N) and qx[a - D .. a + D + N) in LDS as int16, thread c < 2 D + 1
// (then c + TP_BLOCK, ...) sums (target - candidate)^2 over the N samples in a 64-bit integer -- each term below 2^32, the sum
// below 2^43: exact, whatever the order -- and the block takes the minimum of (distance, |a + delta - t|, delta): a wave
// butterfly, then the waves' results from LDS.  Lanes of a wave read the same target samples (a broadcast) and consecutive
// candidate samples.  tq [TP_MAX_N], cq [TP_MAX_N + 2 TP_MAX_D] and red are the block's LDS, free again on return.
template <class Src>
__device__ __forceinline__ long long tp_place(const Src& x, long long k, long long s_prev, int N, int D, int p, int q, int16_t* tq,
                                              int16_t* cq, unsigned long long (*red)[TP_BLOCK / 64]) {
  const int tid = threadIdx.x, H = N / 2, ncand = 2 * D + 1;
  const long long ak = (k * H * p) / q;   // k H p < 2^32 * 2^15
  const long long tk = s_prev + H;
  const long long off = tk - ak;
  if (off >= -D && off <= D) return tk;
  for (int i = tid; i < N; i += TP_BLOCK) tq[i] = (int16_t)tp_quant(x, tk + i);
  for (int i = tid; i < N + 2 * D; i += TP_BLOCK) cq[i] = (int16_t)tp_quant(x, ak - D + i);
  __syncthreads();
  unsigned long long best = ~0ull, bkey = ~0ull;
  for (int c = tid; c < ncand; c += TP_BLOCK) {
    const int16_t* cw = cq + c;
    unsigned long long acc = 0;
    for (int i = 0; i < N; i += 2) {
      const uint32_t tt = *(const uint32_t*)(tq + i);   // two target samples, the same in every lane
      const uint32_t d0 = (uint32_t)((int)(int16_t)(tt & 0xFFFFu) - (int)cw[i]);
      const uint32_t d1 = (uint32_t)(((int)tt >> 16) - (int)cw[i + 1]);
      acc += (unsigned long long)(d0 * d0) + (unsigned long long)(d1 * d1);   // |d| <= 65534: d^2 < 2^32, as the unsigned product gives it
    }
    const long long dist_t = ak + (c - D) - tk;
    tp_min(best, bkey, acc, ((unsigned long long)(dist_t < 0 ? -dist_t : dist_t) << 32) | (unsigned long long)c);
  }
  for (int o = 32; o; o >>= 1) {
    const unsigned long long d2 = (unsigned long long)__shfl_xor((long long)best, o);
    const unsigned long long k2 = (unsigned long long)__shfl_xor((long long)bkey, o);
    tp_min(best, bkey, d2, k2);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = best; red[1][tid >> 6] = bkey; }
  __syncthreads();
  best = red[0][0]; bkey = red[1][0];
  for (int w = 1; w < TP_BLOCK / 64; ++w) tp_min(best, bkey, red[0][w], red[1][w]);
  __syncthreads();   // (red, tq and cq are free for the next searched frame)
  return ak + ((long long)(bkey & 0xFFFFFFFFull) - D);
}

// One block per row; the frames in order, since t_k hangs on s_{k-1} (tp_place).
__global__ __launch_bounds__(TP_BLOCK) void k_tempo_search(TpArgs a, int N, int D, const float* __restrict__ in, long long in_stride,
                                                           int32_t* __restrict__ pos, long long pos_stride) {
  __shared__ __attribute__((aligned(16))) int16_t tq[TP_MAX_N];
  __shared__ __attribute__((aligned(16))) int16_t cq[TP_MAX_N + 2 * TP_MAX_D];
  __shared__ unsigned long long red[2][TP_BLOCK / 64];
  const TpRow r = a.r[blockIdx.x];
  const TpSpan x = {in + (size_t)blockIdx.x * in_stride + r.start, r.len};
  int32_t* ps = pos + (size_t)blockIdx.x * pos_stride;
  const int tid = threadIdx.x;
  for (long long k = r.frames + tid; k < pos_stride; k += TP_BLOCK) ps[k] = 0;   // past the row's frames: zeros
  long long s = 0;
  for (int k = 0; k < r.frames; ++k) {
    if (k) s = tp_place(x, k, s, N, D, r.p, r.q, tq, cq, red);
    if (tid == 0) ps[k] = (int32_t)s;
  }
}

// sample i as float64; 0 where there is none
template <class Src>
__device__ __forceinline__ double tp_sample(const Src& x, long long i) {
  float f;
  return x.get(i, f) ? (double)f : 0.0;
}

// output sample j of frame k >= 1, whose place is sk and whose predecessor's sk1:
// fl32(fl64(x[s_k + j]) w[j] + fl64(x[s_{k-1} + j + H]) w[j + H]), each product and the sum rounded on their own
template <class Src>
__device__ __forceinline__ float tp_ola(const Src& x, int j, int H, long long sk, long long sk1, const double* __restrict__ win) {
  const double u0 = tp_sample(x, sk + j) * win[j];
  const double u1 = tp_sample(x, sk1 + j + H) * win[j + H];
  return (float)(u0 + u1);
}

// grid (tiles of TP_TILE output samples, rows): tp_ola for every sample; frame 0 is the span's own first H samples; zeros from M
// to the stride
__global__ __launch_bounds__(RS_BLOCK) void k_tempo_ola(TpArgs a, int N, const float* __restrict__ in, long long in_stride,
                                                        const double* __restrict__ win, const int32_t* __restrict__ pos,
                                                        long long pos_stride, float* __restrict__ out, long long out_stride) {
  const TpRow r = a.r[blockIdx.y];
  const TpSpan x = {in + (size_t)blockIdx.y * in_stride + r.start, r.len};
  const int32_t* ps = pos + (size_t)blockIdx.y * pos_stride;
  float* y = out + (size_t)blockIdx.y * out_stride;
  const int H = N / 2;
  const long long m0 = (long long)blockIdx.x * TP_TILE;
  const long long end = min(out_stride, m0 + TP_TILE);
  for (long long m = m0 + threadIdx.x; m < end; m += RS_BLOCK) {
    float v = 0.f;
    if (m < r.m) {
      const int k = (int)(m / H), j = (int)(m - (long long)k * H);
      if (k == 0) (void)x.get(m, v);
      else v = tp_ola(x, j, H, ps[k], ps[k - 1], win);
    }
    y[m] = v;
  }
}

// ---- pitch shift of rows (smi_pitch_rows): the stretch above at P / Q, resampled by up / down and cut to n_out
struct PtRow {
  int32_t n_out, up, down, half, tap_off;   // half = H >= 1: taps h[0 .. 2H]; up == down == 1: no pitch ratio (half and tap_off are then 0 and unused)
};
struct PtArgs {
  PtRow r[RS_MAX_ROWS];
};

// sample m < M of the stretched span: k_tempo_ola's value
template <class Src>
__device__ __forceinline__ float pt_stretched(const Src& x, long long m, int H, const int32_t* __restrict__ ps, const double* __restrict__ win) {
  const int k = (int)(m / H), j = (int)(m - (long long)k * H);
  float v = 0.f;
  if (k == 0) (void)x.get(m, v);
  else v = tp_ola(x, j, H, ps[k], ps[k - 1], win);
  return v;
}

// grid (tiles of RS_TILE final output samples, rows).  A block stages its row's taps, computes the stretched samples its tile's
// sums reach -- at most rs_window() of them, each with tp_ola from the places and the input -- straight into LDS, and after one
// barrier sums its outputs with k_rs_rows' loop (rs_tile_sums) against the stretched length M.  The stretched signal is never
// written to memory.  A row without a pitch ratio writes the overlap-add itself, as k_tempo_ola does.  Zeros from n_out to the
// stride.
__global__ __launch_bounds__(RS_BLOCK) void k_pitch_ola(TpArgs a, PtArgs f, int N, const float* __restrict__ in, long long in_stride,
                                                        const double* __restrict__ win, const float* __restrict__ taps,
                                                        const int32_t* __restrict__ pos, long long pos_stride, float* __restrict__ out,
                                                        long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const TpRow r = a.r[blockIdx.y];
  const PtRow g = f.r[blockIdx.y];
  const long long k0 = (long long)blockIdx.x * RS_TILE;
  if (k0 >= out_stride) return;
  const TpSpan x = {in + (size_t)blockIdx.y * in_stride + r.start, r.len};
  const int32_t* ps = pos + (size_t)blockIdx.y * pos_stride;
  float* y = out + (size_t)blockIdx.y * out_stride;
  const int tid = threadIdx.x, H = N / 2;
  if (k0 >= g.n_out) {   // padding past the row's length: zeros
    for (int i = tid; i < RS_TILE && k0 + i < out_stride; i += RS_BLOCK) y[k0 + i] = 0.f;
    return;
  }
  if (g.up == 1 && g.down == 1) {   // no pitch ratio: n_out == M, the stretched samples are the row
    for (int i = tid; i < RS_TILE && k0 + i < out_stride; i += RS_BLOCK) y[k0 + i] = k0 + i < g.n_out ? pt_stretched(x, k0 + i, H, ps, win) : 0.f;
    return;
  }
  const int ntaps = 2 * g.half + 1;
  float* ht = rs_lds;
  float* zw = rs_lds + ntaps;
  const int klast = (int)min(k0 + RS_TILE, (long long)g.n_out) - 1;
  const int j0 = rs_jlo((int)k0 * g.down, g.up, g.half);
  const int j1 = min(rs_jhi(klast * g.down, g.up, g.half), r.m - 1);
  const int nwin = j1 - j0 + 1;   // <= rs_window(): checked on the host
  const float* h = taps + g.tap_off;
  for (int i = tid; i < ntaps; i += RS_BLOCK) ht[i] = h[i];
  for (int i = tid; i < nwin; i += RS_BLOCK) zw[i] = pt_stretched(x, (long long)j0 + i, H, ps, win);
  __syncthreads();
  rs_tile_sums(ht, zw, j0, r.m - 1, (int)k0, g.n_out, g.up, g.down, g.half, y + k0, (int)min((long long)RS_TILE, out_stride - k0));
}

// ---- time-scale change of joined streams (smi_tempos_*)
struct TsRow {
  int32_t slot, set;        // the stream's slot; the state set this push reads (it writes the other one)
  int32_t len, p, q;        // chunk samples; tempo p / q (p == q: a copy)
  int32_t n_old, n_new;     // input samples before / after this push
  int32_t f_old, f_new;     // frames emitted before / after this push
  int32_t m_new;            // outputs emitted after this push (before it: H f_old, or n_old at p == q)
  int32_t h0_old, h0_new;   // first input sample the read set's history holds / the written set's will hold (-1: none is written)
};
struct TsArgs {
  TsRow r[RS_MAX_ROWS];
};
struct TsState {
  const double* win;        // [N]
  float* hist;              // [2][max_streams][hcap]: hist[i] = x[h0 + i], i < n - h0
  int32_t* spos;            // [2][max_streams]: s_{k-1} of the last emitted frame
  int32_t* work;            // [RS_MAX_ROWS][fmax + 1]: s_{f_old - 1}, then the places of this push's frames
  int32_t max_streams, hcap, fmax;
};

// a stream's input from h0_old to n_new: the history, then the chunk.  Nothing before h0_old is ever needed (the host's
// arithmetic, smi_tempos_piece_len); it and everything from n_new on read as 0, as the batch reads what lies beyond L.
struct TsSeq {
  const float* __restrict__ hist;
  const float* __restrict__ chunk;
  int h0, n_old, n_new;
  __device__ __forceinline__ bool get(long long i, float& v) const {
    if (i < h0 || i >= n_new) return false;
    v = i < n_old ? hist[i - h0] : chunk[i - n_old];
    return true;
  }
};

__device__ __forceinline__ TsSeq ts_seq(const TsRow& r, const TsState& s, const float* chunk) {
  return {s.hist + ((size_t)r.set * s.max_streams + r.slot) * s.hcap, chunk, r.h0_old, r.n_old, r.n_new};
}

// One block per row walks the row's newly final frames in order with the batch kernel's tp_place, from the s_{k-1} the stream's
// read set holds; the places go to the row's part of `work` (behind s_{f_old - 1}, for k_tempos_ola) and to pos (may be null),
// and the last one into the set this launch does not read.
__global__ __launch_bounds__(TP_BLOCK) void k_tempos_search(TsArgs a, TsState s, int N, int D, const float* __restrict__ in,
                                                            long long in_stride, int32_t* __restrict__ pos, long long pos_stride) {
  __shared__ __attribute__((aligned(16))) int16_t tq[TP_MAX_N];
  __shared__ __attribute__((aligned(16))) int16_t cq[TP_MAX_N + 2 * TP_MAX_D];
  __shared__ unsigned long long red[2][TP_BLOCK / 64];
  const TsRow r = a.r[blockIdx.x];
  const TsSeq x = ts_seq(r, s, in + (size_t)blockIdx.x * in_stride);
  int32_t* wk = s.work + (size_t)blockIdx.x * (s.fmax + 1);
  int32_t* ps = pos ? pos + (size_t)blockIdx.x * pos_stride : nullptr;
  const int tid = threadIdx.x, nf = r.f_new - r.f_old;   // nf <= fmax: checked on the host
  if (ps)
    for (long long k = nf + tid; k < pos_stride; k += TP_BLOCK) ps[k] = 0;
  long long sp = r.f_old ? s.spos[(size_t)r.set * s.max_streams + r.slot] : 0;
  if (tid == 0) wk[0] = (int32_t)sp;
  for (int i = 0; i < nf; ++i) {
    const long long k = (long long)r.f_old + i;
    if (k) sp = tp_place(x, k, sp, N, D, r.p, r.q, tq, cq, red);
    if (tid == 0) {
      wk[i + 1] = (int32_t)sp;
      if (ps) ps[i] = (int32_t)sp;
    }
  }
  if (tid == 0) s.spos[(size_t)(1 - r.set) * s.max_streams + r.slot] = (int32_t)sp;
}

// grid (tiles of TP_TILE samples of the pieces, rows): the batch kernel's tp_ola for every sample of the row's piece, zeros from
// there to the stride; a stream at p == q copies its chunk.  Tile 0 of a row also writes the stream's next history into the set
// this launch does not read.
__global__ __launch_bounds__(RS_BLOCK) void k_tempos_ola(TsArgs a, TsState s, int N, const float* __restrict__ in, long long in_stride,
                                                         float* __restrict__ out, long long out_stride) {
  const TsRow r = a.r[blockIdx.y];
  const float* c = in + (size_t)blockIdx.y * in_stride;
  const TsSeq x = ts_seq(r, s, c);
  const int32_t* wk = s.work + (size_t)blockIdx.y * (s.fmax + 1);
  float* y = out + (size_t)blockIdx.y * out_stride;
  const int H = N / 2, tid = threadIdx.x;
  const bool copy = r.p == r.q;
  if (blockIdx.x == 0 && r.h0_new >= 0) {
    float* hist2 = s.hist + ((size_t)(1 - r.set) * s.max_streams + r.slot) * s.hcap;
    const int nh = r.n_new - r.h0_new;   // <= hcap: checked on the host
    for (int i = tid; i < nh; i += RS_BLOCK) {
      float v = 0.f;
      (void)x.get((long long)r.h0_new + i, v);
      hist2[i] = v;
    }
  }
  const long long m_old = copy ? (long long)r.n_old : (long long)H * r.f_old;
  const long long i0 = (long long)blockIdx.x * TP_TILE;
  const long long end = min(out_stride, i0 + TP_TILE);
  for (long long i = i0 + tid; i < end; i += RS_BLOCK) {
    const long long m = m_old + i;
    float v = 0.f;
    if (m < r.m_new) {
      if (copy) v = c[i];   // m_new = n_new: i < len
      else {
        const long long k = m / H;
        const int j = (int)(m - k * H), f = (int)(k - r.f_old);   // 0 <= f < f_new - f_old
        if (k == 0) (void)x.get(m, v);
        else v = tp_ola(x, j, H, wk[f + 1], wk[f], s.win);
      }
    }
    y[i] = v;
  }
}

// ---- pitch shift of joined streams (smi_pitchs_*): smi_tempos' stream at P / Q, resampled by up / down as it arrives
struct PsRow {
  int32_t k_old, k_new;     // final outputs emitted before / after this push
};
struct PsArgs {
  PsRow r[RS_MAX_ROWS];
};
struct PsState {
  float* taps;              // [max_streams][tslot]: a slot's up, down, G and a zero as int32, then its taps h[0 .. 2G] (written at open)
  float* tail;              // [2][max_streams][tcap]: tail[i] = z[t0 + i], i < E - t0, t0 = rs_jlo(K down)
  int32_t tslot, tcap;
};

// sample m of the stretched stream, E before this push <= m < E after it (TsRow::m_new; M on the last push): k_tempos_ola's value
__device__ __forceinline__ float ps_stretched(const TsSeq& x, const TsRow& r, const int32_t* __restrict__ wk, long long m, int H,
                                              const double* __restrict__ win) {
  float v = 0.f;
  if (r.p == r.q) {   // the stretch is a copy
    (void)x.get(m, v);
    return v;
  }
  const long long k = m / H;
  const int j = (int)(m - k * H), f = (int)(k - r.f_old);   // 0 <= f < f_new - f_old
  if (k == 0) (void)x.get(m, v);
  else v = tp_ola(x, j, H, wk[f + 1], wk[f], win);
  return v;
}

// grid (tiles of RS_TILE final outputs of the pieces, rows), behind k_tempos_search.  A block stages its row's taps, fills the
// window of stretched samples its sums reach straight into LDS -- those below E before this push from the read set's tail, the
// others with tp_ola over history and chunk from the places in `work` -- and after one barrier sums its outputs with
// rs_tile_sums against the stretched samples there are (M on the last push).  A row at up = down = 1 writes the stretched
// samples themselves, as k_tempos_ola does.  Zeros from the piece's end to the stride.  Tile 0 of a row also writes the
// stream's next input history and next stretched tail into the set this launch does not read.
__global__ __launch_bounds__(RS_BLOCK) void k_pitchs_ola(TsArgs a, PsArgs f, TsState s, PsState ps, int N, const float* __restrict__ in,
                                                         long long in_stride, float* __restrict__ out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const TsRow r = a.r[blockIdx.y];
  const PsRow g = f.r[blockIdx.y];
  const TsSeq x = ts_seq(r, s, in + (size_t)blockIdx.y * in_stride);
  const int32_t* wk = s.work + (size_t)blockIdx.y * (s.fmax + 1);
  float* y = out + (size_t)blockIdx.y * out_stride;
  const int H = N / 2, tid = threadIdx.x;
  const int32_t* hd = (const int32_t*)(ps.taps + (size_t)r.slot * ps.tslot);
  const int up = hd[0], down = hd[1], half = hd[2];
  const bool plain = up == 1 && down == 1;
  const long long e_old = r.p == r.q ? (long long)r.n_old : (long long)H * r.f_old;
  const float* tail = ps.tail + ((size_t)r.set * s.max_streams + r.slot) * ps.tcap;
  const int t0_old = plain ? 0 : rs_jlo(g.k_old * down, up, half);
  if (blockIdx.x == 0 && r.h0_new >= 0) {   // (not the stream's last push)
    float* hist2 = s.hist + ((size_t)(1 - r.set) * s.max_streams + r.slot) * s.hcap;
    const int nh = r.n_new - r.h0_new;   // <= hcap: checked on the host
    for (int i = tid; i < nh; i += RS_BLOCK) {
      float v = 0.f;
      (void)x.get((long long)r.h0_new + i, v);
      hist2[i] = v;
    }
    if (!plain) {
      float* tail2 = ps.tail + ((size_t)(1 - r.set) * s.max_streams + r.slot) * ps.tcap;
      const int t0_new = rs_jlo(g.k_new * down, up, half);   // >= t0_old
      const int nt = r.m_new - t0_new;   // <= tcap: checked on the host
      for (int i = tid; i < nt; i += RS_BLOCK) {
        const int m = t0_new + i;
        tail2[i] = m < e_old ? tail[m - t0_old] : ps_stretched(x, r, wk, m, H, s.win);
      }
    }
  }
  const long long i0 = (long long)blockIdx.x * RS_TILE;
  if (i0 >= out_stride) return;
  const int n_write = (int)min((long long)RS_TILE, out_stride - i0);
  const long long k0 = g.k_old + i0;
  if (k0 >= g.k_new) {   // past the piece: zeros
    for (int i = tid; i < n_write; i += RS_BLOCK) y[i0 + i] = 0.f;
    return;
  }
  if (plain) {   // no pitch ratio: K = E, the stretched samples are the piece
    for (int i = tid; i < n_write; i += RS_BLOCK) y[i0 + i] = k0 + i < g.k_new ? ps_stretched(x, r, wk, k0 + i, H, s.win) : 0.f;
    return;
  }
  const int ntaps = 2 * half + 1;
  float* ht = rs_lds;
  float* zw = rs_lds + ntaps;
  const int klast = (int)min(k0 + RS_TILE, (long long)g.k_new) - 1;
  const int j0 = rs_jlo((int)k0 * down, up, half);   // >= t0_old
  const int j1 = min(rs_jhi(klast * down, up, half), r.m_new - 1);
  const int nwin = j1 - j0 + 1;   // <= rs_window(): checked at open
  const float* h = ps.taps + (size_t)r.slot * ps.tslot + 4;
  for (int i = tid; i < ntaps; i += RS_BLOCK) ht[i] = h[i];
  for (int i = tid; i < nwin; i += RS_BLOCK) {
    const int m = j0 + i;
    zw[i] = m < e_old ? tail[m - t0_old] : ps_stretched(x, r, wk, m, H, s.win);
  }
  __syncthreads();
  rs_tile_sums(ht, zw, j0, r.m_new - 1, (int)k0, g.k_new, up, down, half, y + i0, n_write);
}

// ---- loudness of joined streams (smi_louds_*)
#define LS_STATE 12             // float64 of one stream's state in one set: s[4], open hop, three closed hops, G, I, flags, peak
struct LsRow {
  int32_t slot, set;        // the stream's slot; the state set this push reads (it writes the other one)
  int32_t n_old, len;       // samples before this push; chunk samples, with bit 30 set on the stream's last push
};
struct LsArgs {
  LsRow r[RS_MAX_ROWS];
};
struct LsParam {
  double target, max_gain_db, ceiling, s_up, s_dn;
};
struct LsParams {
  LsParam r[RS_MAX_ROWS];
};
struct LsState {
  LdCoef c;
  double* st;               // [2][max_streams][LS_STATE]
  double* z;                // [max_streams][max_blocks]: the block mean squares so far (written once each: one set)
  float* hist;              // [2][max_streams][hcap]: hist[i] = x[h0 + i], i < n - h0
  double* work;             // [RS_MAX_ROWS][wrow]
  long long wrow, w_s, w_parts, w_hops, w_gain;   // a row's scratch and where its parts lie (end states at 0)
  int32_t max_streams, max_blocks, hcap, pps, block;
};

// everything a push is, from the stream's length before it, the chunk's length and `last`: the host's checks and the kernels
// both call this, so they cannot disagree
struct LsPlan {
  int n_old, n_new, last;
  int h0_old, h0_new;       // first sample the read set's history holds / the written set's will hold
  int seg0, nwhole, nseg;   // first segment this push filters; the whole segments; those and the tail short of one
  int e_old, e_new;         // samples emitted before / after
  int k_old, k_new;         // knots made before / after
  int z_old, z_new;         // whole blocks before / after
};
__host__ __device__ __forceinline__ int ls_emitted(int n, int hop) { return n / hop > 4 ? (n / hop - 4) * hop : 0; }
__host__ __device__ __forceinline__ int ls_blocks(int n, int hop) { return n / hop > 3 ? n / hop - 3 : 0; }
__host__ __device__ __forceinline__ int ls_hist_start(int n, int hop) {
  const int e = ls_emitted(n, hop), f = n / LD_SEG * LD_SEG;
  const int a = (e < f ? e : f) - 2;   // (the two samples before the first unfiltered segment are its input history)
  return a > 0 ? a : 0;
}
__host__ __device__ __forceinline__ LsPlan ls_plan(int n_old, int len, int last, int hop) {
  LsPlan p;
  p.n_old = n_old; p.n_new = n_old + len; p.last = last;
  p.h0_old = ls_hist_start(n_old, hop); p.h0_new = ls_hist_start(p.n_new, hop);
  p.seg0 = n_old / LD_SEG;
  p.nwhole = p.n_new / LD_SEG - p.seg0;
  p.nseg = p.nwhole + (p.n_new % LD_SEG ? 1 : 0);
  p.e_old = ls_emitted(n_old, hop); p.e_new = last ? p.n_new : ls_emitted(p.n_new, hop);
  p.z_old = ls_blocks(n_old, hop); p.z_new = ls_blocks(p.n_new, hop);
  p.k_old = p.z_old; p.k_new = last ? (p.n_new ? (p.n_new - 1) / hop + 2 : 0) : p.z_new;
  return p;
}
__device__ __forceinline__ LsPlan ls_plan(const LsRow& r, int hop) { return ls_plan(r.n_old, r.len & 0x3FFFFFFF, (r.len >> 30) & 1, hop); }

// a stream's input from h0_old to n_new: the history, then the chunk
struct LsSeq {
  const float* __restrict__ hist;
  const float* __restrict__ chunk;
  int h0, n_old;
  __device__ __forceinline__ float at(int i) const { return i < n_old ? hist[i - h0] : chunk[i - n_old]; }
};
__device__ __forceinline__ LsSeq ls_seq(const LsRow& r, const LsPlan& p, const LsState& s, const float* chunk) {
  return {s.hist + ((size_t)r.set * s.max_streams + r.slot) * s.hcap, chunk, p.h0_old, p.n_old};
}

// ld_stage over a stream: tile blockIdx.x of the segments this push filters, lane l on segment seg0 + 64 blockIdx.x + l
__device__ __forceinline__ int ls_stage(const LsPlan& p, const LsSeq& x, float* lds, LdState& s) {
  const int a0 = (p.seg0 + blockIdx.x * LD_LANES) * LD_SEG, tid = threadIdx.x;   // of the stream
  const int cnt = min(LD_TILE, p.n_new - a0);
  for (int i = tid; i < cnt; i += LD_LANES) lds[(i / LD_SEG) * LD_PITCH + (i % LD_SEG)] = x.at(a0 + i);
  __syncthreads();
  const int i0 = a0 + tid * LD_SEG;
  s.x1 = i0 >= 1 && i0 < p.n_new ? (double)x.at(i0 - 1) : 0.0;
  s.x2 = i0 >= 2 && i0 < p.n_new ? (double)x.at(i0 - 2) : 0.0;
  return max(0, min(LD_SEG, p.n_new - i0));
}

// grid (tiles of LD_TILE samples of the push's segments, rows): k_loud_seg for every whole segment of the push
__global__ __launch_bounds__(LD_LANES) void k_louds_seg(LsArgs a, LsState s, const float* __restrict__ in, long long in_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const LsRow r = a.r[blockIdx.y];
  const LsPlan p = ls_plan(r, s.block / 4);
  if ((int)blockIdx.x * LD_LANES >= p.nwhole) return;
  LdState t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ls_stage(p, ls_seq(r, p, s, in + (size_t)blockIdx.y * in_stride), rs_lds, t);
  const int g = blockIdx.x * LD_LANES + threadIdx.x;
  if (g >= p.nwhole) return;
  const float* seg = rs_lds + threadIdx.x * LD_PITCH;
  for (int i = 0; i < LD_SEG; ++i) ld_step(s.c, t, (double)seg[i]);
  double* E = s.work + (size_t)blockIdx.y * s.wrow + 4 * (size_t)g;
  E[0] = t.p1; E[1] = t.p2; E[2] = t.q1; E[3] = t.q2;
}

// one wave per row: k_loud_carry's recurrence from the stream's state; the state behind the last whole segment goes to the set
// this launch does not read
__global__ __launch_bounds__(64) void k_louds_carry(LsArgs a, LsState s) {
  __shared__ double e[64][4];
  const LsRow r = a.r[blockIdx.x];
  const LsPlan p = ls_plan(r, s.block / 4);
  const int lane = threadIdx.x, ns = p.nwhole + 1;
  const double* E = s.work + (size_t)blockIdx.x * s.wrow;
  double* S = s.work + (size_t)blockIdx.x * s.wrow + s.w_s;
  const double* rd = s.st + ((size_t)r.set * s.max_streams + r.slot) * LS_STATE;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (p.seg0) { s0 = rd[0]; s1 = rd[1]; s2 = rd[2]; s3 = rd[3]; }
  const LdCoef& c = s.c;
  for (int k0 = 0; k0 < ns; k0 += 64) {
    if (k0 + lane < p.nwhole)
      for (int i = 0; i < 4; ++i) e[lane][i] = E[4 * (size_t)(k0 + lane) + i];
    __syncthreads();
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    const int cnt = min(64, ns - k0);
    for (int t = 0; t < cnt; ++t) {
      if (lane == t) { m0 = s0; m1 = s1; m2 = s2; m3 = s3; }
      if (k0 + t < p.nwhole) {
        const double n0 = (((c.T[0][0] * s0 + c.T[0][1] * s1) + c.T[0][2] * s2) + c.T[0][3] * s3) + e[t][0];
        const double n1 = (((c.T[1][0] * s0 + c.T[1][1] * s1) + c.T[1][2] * s2) + c.T[1][3] * s3) + e[t][1];
        const double n2 = (((c.T[2][0] * s0 + c.T[2][1] * s1) + c.T[2][2] * s2) + c.T[2][3] * s3) + e[t][2];
        const double n3 = (((c.T[3][0] * s0 + c.T[3][1] * s1) + c.T[3][2] * s2) + c.T[3][3] * s3) + e[t][3];
        s0 = n0; s1 = n1; s2 = n2; s3 = n3;
      }
    }
    if (lane < cnt) {
      double* d = S + 4 * (size_t)(k0 + lane);
      d[0] = m0; d[1] = m1; d[2] = m2; d[3] = m3;
    }
    __syncthreads();
  }
  if (lane == 0) {   // (every lane holds the state behind the last whole segment)
    double* wr = s.st + ((size_t)(1 - r.set) * s.max_streams + r.slot) * LS_STATE;
    wr[0] = s0; wr[1] = s1; wr[2] = s2; wr[3] = s3;
  }
}

// grid as k_louds_seg: k_loud_energy for every segment of the push, the tail short of one included (it is filtered again, from
// the same state, by the push that completes it: the hops that close inside it have the sums they will have then)
__global__ __launch_bounds__(LD_LANES) void k_louds_energy(LsArgs a, LsState s, const float* __restrict__ in, long long in_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  const LsRow r = a.r[blockIdx.y];
  const int hop = s.block / 4;
  const LsPlan p = ls_plan(r, hop);
  if ((int)blockIdx.x * LD_LANES >= p.nseg) return;
  LdState t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int m = ls_stage(p, ls_seq(r, p, s, in + (size_t)blockIdx.y * in_stride), rs_lds, t);
  if (m == 0) return;
  const int g = blockIdx.x * LD_LANES + threadIdx.x;
  double* row = s.work + (size_t)blockIdx.y * s.wrow;
  const double* S = row + s.w_s + 4 * (size_t)g;
  t.p1 = S[0]; t.p2 = S[1]; t.q1 = S[2]; t.q2 = S[3];
  double* P = row + s.w_parts + (size_t)g * s.pps;
  const float* seg = rs_lds + threadIdx.x * LD_PITCH;
  int i = (p.seg0 + g) * LD_SEG;         // of the stream
  int edge = (i / hop + 1) * hop;        // where the hop that holds sample i ends
  int q = 0, held = 0;
  double acc = 0.0;
  for (int u = 0; u < m; ++u) {
    const double o = ld_step(s.c, t, (double)seg[u]);
    acc = acc + o * o;
    held = 1;
    if (++i == edge) {
      P[q++] = acc;
      acc = 0.0;
      held = 0;
      edge += hop;
    }
  }
  if (held) P[q] = acc;
}

// the parts of hop h in the segments k0 .. k1 of this push, added in ascending order to t (ls_plan's seg0 is segment 0 of P)
__device__ __forceinline__ double ls_hop_sum(double t, const double* P, int pps, int seg0, int hop, int h, int k0, int k1) {
  for (int k = k0; k <= k1; ++k) t = t + P[(size_t)(k - seg0) * pps + (h - (k * LD_SEG) / hop)];
  return t;
}

// The gated loudness over z[0 .. j] with k_loud_gate's sums: sum1 / cnt1 are this thread's running sums of the blocks
// t, t + 256, ... <= j that pass the absolute gate.  Returns false where no block passes.
__device__ __forceinline__ bool ls_gated(const double* z, int j, double abs_gate, double sum1, double cnt1, double* red, double& loud) {
  const double S1 = ld_block_sum(sum1, red), C1 = ld_block_sum(cnt1, red);
  loud = -INFINITY;
  if (!(C1 > 0.0)) return false;
  const double rel = 0.1 * (S1 / C1);
  double sum = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i <= j; i += LD_GATE) {
    const double v = z[i];
    if (v > abs_gate && v > rel) { sum = sum + v; cnt = cnt + 1.0; }
  }
  const double S2 = ld_block_sum(sum, red), C2 = ld_block_sum(cnt, red);
  if (!(C2 > 0.0)) return false;
  loud = -0.691 + 10.0 * log10(S2 / C2);
  return true;
}

// max |x| over [lo, hi) of the stream, by the block
__device__ __forceinline__ double ls_peak(const LsSeq& x, int lo, int hi, double* red) {
  uint32_t pk = 0;
  for (int i = lo + (int)threadIdx.x; i < hi; i += LD_GATE) pk = max(pk, __float_as_uint(x.at(i)) & 0x7FFFFFFFu);
  return ld_block_max((double)__uint_as_float(pk), red);
}

// one knot: the target gain `A` (have: from a loudness; else a held gain), the slew step for j > 0, the peak step
__device__ __forceinline__ double ls_knot(const LsParam& q, int j, double A, int flags, double g_prev, double gmax, bool clamp_max,
                                          double pk, int& flags_out) {
  if (!(q.target == q.target)) { flags_out = 0; return 1.0; }
  if (clamp_max && A > gmax) { A = gmax; flags |= 1; }
  if (j > 0) {
    const double lo = g_prev * q.s_dn, hi = g_prev * q.s_up;
    if (A < lo) { A = lo; flags |= 4; }
    else if (A > hi) { A = hi; flags |= 4; }
  }
  double g = A;
  if (A * pk > q.ceiling) { g = q.ceiling / pk; flags |= 2; }
  flags_out = flags;
  return g;
}

// One block per row: closes the hops and blocks the push completes, then walks the row's new knots in order (include/sparkmi.h).
// Every thread carries the same scalars (the block-wide sums return one value to all); thread 0 writes.
__global__ __launch_bounds__(LD_GATE) void k_louds_knots(LsArgs a, LsParams pr, LsState s, double abs_gate, const float* __restrict__ in,
                                                         long long in_stride, double* __restrict__ gain, long long gain_stride,
                                                         double* __restrict__ stats) {
  __shared__ double red[LD_GATE];
  const int b = blockIdx.x, tid = threadIdx.x, block = s.block, hop = block / 4;
  const LsRow r = a.r[b];
  const LsParam q = pr.r[b];
  const LsPlan p = ls_plan(r, hop);
  const LsSeq x = ls_seq(r, p, s, in + (size_t)b * in_stride);
  const double* rd = s.st + ((size_t)r.set * s.max_streams + r.slot) * LS_STATE;
  double* wr = s.st + ((size_t)(1 - r.set) * s.max_streams + r.slot) * LS_STATE;
  double* row = s.work + (size_t)b * s.wrow;
  const double* P = row + s.w_parts;
  double* Hw = row + s.w_hops;       // Hw[3 + h - hF]: the sum of hop h; Hw[0 .. 3): the three hops before hF
  double* gw = row + s.w_gain;       // gw[1 + j - k_old]: G_j; gw[0]: the last knot before this push
  double* Z = s.z + (size_t)r.slot * s.max_blocks;
  double* gr = gain ? gain + (size_t)b * gain_stride : nullptr;
  const int nk = p.k_new - p.k_old;
  if (gr)
    for (long long i = 2LL * nk + tid; i < gain_stride; i += LD_GATE) gr[i] = 0.0;
  // 1. hop sums, from the first hop that is open at the first segment this push filters
  const int F_old = p.seg0 * LD_SEG, hF = F_old / hop;
  const double open_old = F_old % hop ? rd[4] : 0.0;
  const int nh_end = (p.n_new + hop - 1) / hop;
  if (tid < 3) Hw[tid] = rd[5 + tid];
  for (int h = hF + tid; h < nh_end; h += LD_GATE) {
    const int lo = h * hop, hi = min(p.n_new, lo + hop) - 1;
    Hw[3 + h - hF] = ls_hop_sum(h == hF ? open_old : 0.0, P, s.pps, p.seg0, hop, h, max(lo / LD_SEG, p.seg0), hi / LD_SEG);
  }
  __syncthreads();
  // 2. the blocks this push completes
  for (int j = p.z_old + tid; j < p.z_new; j += LD_GATE) {
    const double* H = Hw + 3 + (j - hF);
    Z[j] = (((H[0] + H[1]) + H[2]) + H[3]) / (double)block;
  }
  const double pk_chunk = ls_peak(x, p.n_old, p.n_new, red);   // (its barriers also publish Hw and Z to the block)
  const double peak = p.n_old ? fmax(rd[11], pk_chunk) : pk_chunk;
  // 3. the knots, in order
  double g_prev = p.k_old ? rd[8] : 1.0, loud = p.n_old ? rd[9] : -INFINITY;
  int flags_or = p.n_old ? (int)rd[10] : 0;
  const double gmax = pow(10.0, q.max_gain_db / 20.0);
  if (tid == 0) gw[0] = g_prev;
  double sum1 = 0.0, cnt1 = 0.0;
  for (int j = tid; j < p.k_old; j += LD_GATE) {
    const double v = Z[j];
    if (v > abs_gate) { sum1 = sum1 + v; cnt1 = cnt1 + 1.0; }
  }
  const int k_norm = min(p.k_new, p.z_new);
  for (int j = p.k_old; j < k_norm; ++j) {
    if (j % LD_GATE == tid) {
      const double v = Z[j];
      if (v > abs_gate) { sum1 = sum1 + v; cnt1 = cnt1 + 1.0; }
    }
    double I;
    const bool have = ls_gated(Z, j, abs_gate, sum1, cnt1, red, I);
    loud = I;
    const double pk = ls_peak(x, max(0, (j - 1) * hop), min(p.n_new, (j + 1) * hop), red);
    int fl;
    const double A = have ? pow(10.0, (q.target - I) / 20.0) : g_prev;   // (g_prev is 1 at knot 0)
    const double g = ls_knot(q, j, A, have ? 0 : 8, g_prev, gmax, have, pk, fl);
    if (tid == 0) {
      gw[1 + j - p.k_old] = g;
      if (gr) { gr[2 * (j - p.k_old)] = g; gr[2 * (j - p.k_old) + 1] = (double)fl; }
    }
    g_prev = g;
    flags_or |= fl;
  }
  if (p.k_new > k_norm) {   // the stream's end: the knots behind the last whole block hold one target gain
    double A = g_prev;
    int f0 = 8;
    bool clamp = false;
    if (p.z_new == 0) {     // shorter than a block: one block, the whole stream, the absolute gate alone
      const int nh = (p.n_new + hop - 1) / hop;
      double t = 0.0;
      for (int h = 0; h < nh; ++h) t = t + Hw[3 + h - hF];
      const double zz = t / (double)p.n_new;
      A = 1.0;
      loud = -INFINITY;
      if (zz > abs_gate) {
        loud = -0.691 + 10.0 * log10(zz);
        A = pow(10.0, (q.target - loud) / 20.0);
        f0 = 0;
        clamp = true;
      }
    }
    for (int j = max(p.k_old, k_norm); j < p.k_new; ++j) {
      const double pk = ls_peak(x, max(0, (j - 1) * hop), min(p.n_new, (j + 1) * hop), red);
      int fl;
      const double g = ls_knot(q, j, A, f0, g_prev, gmax, clamp, pk, fl);
      if (tid == 0) {
        gw[1 + j - p.k_old] = g;
        if (gr) { gr[2 * (j - p.k_old)] = g; gr[2 * (j - p.k_old) + 1] = (double)fl; }
      }
      g_prev = g;
      flags_or |= fl;
    }
  }
  if (tid) return;
  // the next state: the hop that is open behind the last whole segment, and the three before it
  const int F_new = (p.seg0 + p.nwhole) * LD_SEG, hN = F_new / hop;
  double open_new = 0.0;
  if (F_new % hop) {
    const int lo = hN * hop;
    open_new = ls_hop_sum(hN == hF ? open_old : 0.0, P, s.pps, p.seg0, hop, hN, max(lo / LD_SEG, p.seg0), p.seg0 + p.nwhole - 1);
  }
  const double h0 = Hw[hN - hF], h1 = Hw[hN - hF + 1], h2 = Hw[hN - hF + 2];
  wr[4] = open_new; wr[5] = h0; wr[6] = h1; wr[7] = h2;
  wr[8] = g_prev; wr[9] = loud; wr[10] = (double)flags_or; wr[11] = peak;
  if (stats) {
    double* st = stats + 4 * (size_t)b;
    st[0] = loud; st[1] = peak; st[2] = g_prev; st[3] = (double)flags_or;
  }
}

// grid (tiles of GN_TILE samples of the pieces, rows): every sample of the row's piece times the gain between its two knots,
// zeros from there to the stride.  Tile 0 of a row also writes the stream's next history into the set this launch does not read.
__global__ __launch_bounds__(RS_BLOCK) void k_louds_apply(LsArgs a, LsState s, const float* __restrict__ in, long long in_stride,
                                                          float* __restrict__ out, long long out_stride) {
  const LsRow r = a.r[blockIdx.y];
  const int hop = s.block / 4, tid = threadIdx.x;
  const LsPlan p = ls_plan(r, hop);
  const LsSeq x = ls_seq(r, p, s, in + (size_t)blockIdx.y * in_stride);
  const double* gw = s.work + (size_t)blockIdx.y * s.wrow + s.w_gain;
  float* y = out + (size_t)blockIdx.y * out_stride;
  if (blockIdx.x == 0 && !p.last) {
    float* hist2 = s.hist + ((size_t)(1 - r.set) * s.max_streams + r.slot) * s.hcap;
    for (int i = p.h0_new + tid; i < p.n_new; i += RS_BLOCK) hist2[i - p.h0_new] = x.at(i);   // n_new - h0_new <= hcap: the host's check
  }
  const long long i0 = (long long)blockIdx.x * GN_TILE;
  const long long end = min(out_stride, i0 + GN_TILE);
  const int piece = p.e_new - p.e_old;
  for (long long i = i0 + tid; i < end; i += RS_BLOCK) {
    float v = 0.f;
    if (i < piece) {
      const int m = p.e_old + (int)i, j = m / hop;
      const double g0 = gw[1 + j - p.k_old], g1 = gw[2 + j - p.k_old];
      const double fr = (double)(m - j * hop) / (double)hop;
      const double d = (g1 - g0) * fr;
      v = (float)((double)x.at(m) * (g0 + d));
    }
    y[i] = v;
  }
}

// ---- limiter of joined streams (smi_limits_*)
#define LT_STATE 4              // float64 of one stream's state in one set: max e, min s, the count of s < 1 (and one unused)
struct LtRow {
  int32_t slot, set;        // the stream's slot; the state set this push reads (it writes the other one)
  int32_t n_old, len;       // samples before this push; chunk samples, with bit 30 set on the stream's last push
  int32_t tp;               // 1: the true-peak mode; 0: the sample peak
  float c32;                // the largest float32 <= ceiling
  double ceiling;
};
struct LtArgs {
  LtRow r[RS_MAX_ROWS];
};
struct LtState {
  const double* win;        // [A + R + 1]
  const double* taps;       // [LM_MAX_TAPS]
  double* st;               // [2][max_streams][LT_STATE]
  float* hist;              // [2][max_streams][hcap]: hist[i] = x[h0 + i], i < n - h0
  double* work;             // [rows of a call][wrow]: r over [r_lo, r_hi), then three values a tile
  long long wrow, w_emax, w_smin, w_cnt;
  int32_t max_streams, hcap, A, R, phases;
};

// everything a push is, from the stream's length before it, the chunk's length and `last`: the host's checks and the kernels
// both call this, so they cannot disagree.  W = A + R.
struct LtPlan {
  int n_old, n_new, last;
  int e_old, e_new;         // samples emitted before / after
  int h0_old, h0_new;       // first sample the read set's history holds / the written set's will hold
  int r_lo, r_hi;           // the samples whose r this push computes: what the piece's sums can read, inside the stream
};
__host__ __device__ __forceinline__ int lt_emitted(int n, int W) { return n > W + LM_HALO ? n - (W + LM_HALO) : 0; }
__host__ __device__ __forceinline__ int lt_hist_start(int n, int W) {
  const int a = lt_emitted(n, W) - W - (LM_HALO - 1);
  return a > 0 ? a : 0;
}
__host__ __device__ __forceinline__ LtPlan lt_plan(int n_old, int len, int last, int W) {
  LtPlan p;
  p.n_old = n_old; p.n_new = n_old + len; p.last = last;
  p.e_old = lt_emitted(n_old, W); p.e_new = last ? p.n_new : lt_emitted(p.n_new, W);
  p.h0_old = lt_hist_start(n_old, W); p.h0_new = lt_hist_start(p.n_new, W);
  p.r_lo = p.e_old > W ? p.e_old - W : 0;
  p.r_hi = p.e_new > p.e_old ? (p.e_new + W < p.n_new ? p.e_new + W : p.n_new) : p.r_lo;
  return p;
}
__device__ __forceinline__ LtPlan lt_plan(const LtRow& r, int W) { return lt_plan(r.n_old, r.len & 0x3FFFFFFF, (r.len >> 30) & 1, W); }

// a stream's input: the history from h0_old, then the chunk; zero before the stream, behind its end, and before h0_old (which
// no sum of this push reads)
struct LtSeq {
  const float* __restrict__ hist;
  const float* __restrict__ chunk;
  int h0, n_old, n_new;
  __device__ __forceinline__ float at(int i) const { return i < h0 || i >= n_new ? 0.f : (i < n_old ? hist[i - h0] : chunk[i - n_old]); }
};
__device__ __forceinline__ LtSeq lt_seq(const LtRow& r, const LtPlan& p, const LtState& s, const float* chunk) {
  return {s.hist + ((size_t)r.set * s.max_streams + r.slot) * s.hcap, chunk, p.h0_old, p.n_old, p.n_new};
}

// grid (tiles of LM_TILE samples of [r_lo, r_hi), rows): k_limit_env over the virtual sequence of history followed by the chunk,
// at g = 1; the tile's max e counts the samples this push emits alone
__global__ __launch_bounds__(RS_BLOCK) void k_limits_env(LtArgs a, LtState s, const float* __restrict__ in, long long in_stride) {
  __shared__ float xs[LM_TILE + 2 * LM_HALO];
  __shared__ double red[RS_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const LtRow r = a.r[b];
  const LtPlan p = lt_plan(r, s.A + s.R);
  const int t0 = p.r_lo + blockIdx.x * LM_TILE;   // of the stream
  if (t0 >= p.r_hi) return;
  const LtSeq x = lt_seq(r, p, s, in + (size_t)b * in_stride);
  for (int i = tid; i < LM_TILE + 2 * LM_HALO; i += RS_BLOCK) xs[i] = x.at(t0 - LM_HALO + i);
  __syncthreads();
  double* row = s.work + (size_t)b * s.wrow;
  const int cnt = min(LM_TILE, p.r_hi - t0);
  double emax = 0.0;
  for (int i = tid; i < cnt; i += RS_BLOCK) {
    const double e = lm_env(s.taps, s.phases, r.tp != 0, xs + LM_HALO + i);
    row[t0 - p.r_lo + i] = lm_req(1.0, e, r.ceiling);
    if (t0 + i >= p.e_old && t0 + i < p.e_new) emax = fmax(emax, e);
  }
  emax = lm_block_red<0>(emax, red);
  if (!tid) row[s.w_emax + blockIdx.x] = emax;
}

// grid (tiles of LM_TILE samples of the pieces up to out_stride, rows): k_limit_apply over the piece -- r from the row's work,
// 1 outside [r_lo, r_hi) --, zeros from the piece's end to the stride.  Tile 0 of a row also writes the stream's next history
// into the set this launch does not read.
__global__ __launch_bounds__(RS_BLOCK) void k_limits_apply(LtArgs a, LtState s, const float* __restrict__ in, long long in_stride,
                                                           float* __restrict__ out, long long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  __shared__ double red[RS_BLOCK];
  double* q = (double*)rs_lds;
  const int b = blockIdx.y, tid = threadIdx.x;
  const LtRow r = a.r[b];
  const int W = s.A + s.R;
  const LtPlan p = lt_plan(r, W);
  const LtSeq x = lt_seq(r, p, s, in + (size_t)b * in_stride);
  float* y = out + (size_t)b * out_stride;
  double* row = s.work + (size_t)b * s.wrow;
  if (blockIdx.x == 0 && !p.last) {
    float* hist2 = s.hist + ((size_t)(1 - r.set) * s.max_streams + r.slot) * s.hcap;
    for (int i = p.h0_new + tid; i < p.n_new; i += RS_BLOCK) hist2[i - p.h0_new] = x.at(i);   // n_new - h0_new <= hcap: the host's check
  }
  const long long k0 = (long long)blockIdx.x * LM_TILE;   // of the piece
  const int piece = p.e_new - p.e_old;
  const bool hit = k0 < piece;
  double sv[LM_TILE / RS_BLOCK];
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) sv[u] = 1.0;
  if (hit) {
    const int nq = LM_TILE + 2 * W;
    const int j0 = p.e_old + (int)k0 - W;   // the stream's index of q[0]
    for (int i = tid; i < nq; i += RS_BLOCK) {
      const int j = j0 + i;
      q[i] = j >= p.r_lo && j < p.r_hi ? row[j - p.r_lo] : 1.0;
    }
    lm_smooth(q, s.A, s.R, s.win, sv);
  }
  double smin = 1.0, cnt = 0.0;
#pragma unroll
  for (int u = 0; u < LM_TILE / RS_BLOCK; ++u) {
    const long long i = k0 + tid + u * RS_BLOCK;
    if (i >= out_stride) continue;
    float v = 0.f;
    if (i < piece) {
      v = lm_out(x.at(p.e_old + (int)i), 1.0, sv[u], r.c32);
      smin = fmin(smin, sv[u]);
      if (sv[u] < 1.0) cnt = cnt + 1.0;
    }
    y[i] = v;
  }
  if (!hit) return;
  smin = lm_block_red<1>(smin, red);
  cnt = lm_block_red<2>(cnt, red);
  if (!tid) {
    row[s.w_smin + blockIdx.x] = smin;
    row[s.w_cnt + blockIdx.x] = cnt;
  }
}

// one block per row: the tiles' values and the stream's stats so far into the set this launch does not read and, where asked
// for, into the row's four stats.  max, min and a sum of whole numbers: exact in any order.
__global__ __launch_bounds__(RS_BLOCK) void k_limits_stats(LtArgs a, LtState s, double* __restrict__ stats) {
  __shared__ double red[RS_BLOCK];
  const int b = blockIdx.x, tid = threadIdx.x;
  const LtRow r = a.r[b];
  const LtPlan p = lt_plan(r, s.A + s.R);
  const double* row = s.work + (size_t)b * s.wrow;
  double emax = 0.0, smin = 1.0, cnt = 0.0;
  const int te = (p.r_hi - p.r_lo + LM_TILE - 1) / LM_TILE, ta = (p.e_new - p.e_old + LM_TILE - 1) / LM_TILE;
  for (int t = tid; t < te; t += RS_BLOCK) emax = fmax(emax, row[s.w_emax + t]);
  for (int t = tid; t < ta; t += RS_BLOCK) {
    smin = fmin(smin, row[s.w_smin + t]);
    cnt = cnt + row[s.w_cnt + t];
  }
  emax = lm_block_red<0>(emax, red);
  smin = lm_block_red<1>(smin, red);
  cnt = lm_block_red<2>(cnt, red);
  if (tid) return;
  if (p.n_old > 0) {   // (a first push reads no state)
    const double* so = s.st + ((size_t)r.set * s.max_streams + r.slot) * LT_STATE;
    emax = fmax(emax, so[0]); smin = fmin(smin, so[1]); cnt = cnt + so[2];
  }
  double* sn = s.st + ((size_t)(1 - r.set) * s.max_streams + r.slot) * LT_STATE;
  sn[0] = emax; sn[1] = smin; sn[2] = cnt;
  if (stats) {
    double* st = stats + 4 * (size_t)b;
    st[0] = emax; st[1] = 1.0; st[2] = smin; st[3] = cnt;
  }
}

}  // namespace

struct smi_rs {
  int max_rows, max_in, max_out;
  DevBuf<float> pool;
  int pool_used;
  std::vector<Filter> filters;
};

// a stream's counters live on the host: a push's piece length is known before its launch
struct JnStream {
  int open = 0, set = 0;
  long long chunks = 0, n = 0, k = 0;   // chunks pushed, joined samples N, outputs emitted K
};
struct smi_join {
  JnState s;
  int max_chunk, n_taps;
  size_t lds;
  DevBuf<char> pool;
  std::vector<JnStream> streams;
};

static const Filter* rs_find(const smi_rs* h, int up, int down) {
  for (const Filter& f : h->filters)
    if (f.up == up && f.down == down) return &f;
  return nullptr;
}

static long long rs_out_len(long long n, int up, int down) { return (n * up + down - 1) / down; }

// every check of a rows call, then its descriptors; nothing reaches the device before all rows pass
static int rs_rows_args(const smi_rs* h, const char* who, const int32_t* n_in, const int32_t* up, const int32_t* down, int B,
                        long long in_stride, long long out_stride, RsArgs& A, int& tiles, size_t& lds) {
  SMI_REQUIRE(B >= 1 && B <= h->max_rows, "%s: B=%d outside 1..%d (the handle's max_rows)", who, B, h->max_rows);
  long long need = 0;
  lds = 0;
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(n_in[b] >= 1 && n_in[b] <= h->max_in, "%s: n_in[%d]=%d outside 1..%d (the handle's max_in)", who, b, n_in[b], h->max_in);
    SMI_REQUIRE(up[b] >= 1 && down[b] >= 1, "%s: up[%d]=%d, down[%d]=%d: both must be positive", who, b, up[b], b, down[b]);
    SMI_REQUIRE((long long)n_in[b] * up[b] < (1LL << 31), "%s: n_in[%d] * up = %lld reaches 2^31", who, b, (long long)n_in[b] * up[b]);
    const long long no = rs_out_len(n_in[b], up[b], down[b]);
    SMI_REQUIRE(no <= h->max_out, "%s: row %d gives n_out=%lld > %d (the handle's max_out)", who, b, no, h->max_out);
    SMI_REQUIRE(no * down[b] < (1LL << 31), "%s: n_out * down = %lld of row %d reaches 2^31", who, no * down[b], b);
    RsRow& r = A.r[b];
    r.n_in = n_in[b]; r.n_out = (int32_t)no; r.up = up[b]; r.down = down[b]; r.tap_off = 0; r.half = 0;
    if (!(up[b] == 1 && down[b] == 1)) {
      const Filter* f = rs_find(h, up[b], down[b]);
      SMI_REQUIRE(f, "%s: ratio up/down = %d/%d of row %d is not registered (smi_rs_register)", who, up[b], down[b], b);
      r.tap_off = f->tap_off; r.half = f->half;
      const size_t fl = (size_t)(2 * f->half + 1) + (size_t)rs_window(f->up, f->down, f->half);
      if (fl > lds) lds = fl;
    }
    if (no > need) need = no;
  }
  SMI_REQUIRE(in_stride >= 1 && out_stride >= need, "%s: out_stride=%lld below the longest output row (%lld)", who, out_stride, need);
  for (int b = 0; b < B; ++b)
    SMI_REQUIRE(n_in[b] <= in_stride, "%s: n_in[%d]=%d exceeds in_stride=%lld", who, b, n_in[b], in_stride);
  SMI_REQUIRE(out_stride <= RS_MAX_SAMPLES, "%s: out_stride=%lld above %d", who, out_stride, RS_MAX_SAMPLES);
  tiles = (int)((out_stride + RS_TILE - 1) / RS_TILE);
  lds *= sizeof(float);
  return SMI_OK;
}

extern "C" {

int smi_rs_create(int max_rows, int max_in, int max_out, smi_rs** out) {
  SMI_REQUIRE(out, "smi_rs_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_rows >= 1 && max_rows <= RS_MAX_ROWS, "smi_rs_create: max_rows=%d outside 1..%d", max_rows, RS_MAX_ROWS);
  SMI_REQUIRE(max_in >= 1 && max_in <= RS_MAX_SAMPLES, "smi_rs_create: max_in=%d outside 1..%d", max_in, RS_MAX_SAMPLES);
  SMI_REQUIRE(max_out >= 1 && max_out <= RS_MAX_SAMPLES, "smi_rs_create: max_out=%d outside 1..%d", max_out, RS_MAX_SAMPLES);
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_rs* h = new smi_rs();
  h->max_rows = max_rows; h->max_in = max_in; h->max_out = max_out;
  if (h->pool.alloc((size_t)RS_POOL_FLOATS * sizeof(float), "smi_rs_create: tap pool")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  *out = h;
  return SMI_OK;
}

int smi_rs_destroy(smi_rs* h) {
  delete h;
  return SMI_OK;
}

int smi_rs_register(smi_rs* h, int up, int down, const double* taps_host, int n_taps) {
  SMI_REQUIRE(h && taps_host, "smi_rs_register: null argument");
  SMI_REQUIRE(up >= 1 && down >= 1 && !(up == 1 && down == 1), "smi_rs_register: up=%d, down=%d: positive and not 1/1 (a copy needs no filter)", up, down);
  SMI_REQUIRE(n_taps >= 1 && (n_taps & 1), "smi_rs_register: n_taps=%d must be odd (taps h[0 .. 2H])", n_taps);
  SMI_REQUIRE(!rs_find(h, up, down), "smi_rs_register: ratio up/down = %d/%d is registered already", up, down);
  const int half = n_taps / 2;
  const long long fl = (long long)n_taps + rs_window(up, down, half);
  SMI_REQUIRE(fl <= RS_LDS_FLOATS, "smi_rs_register: n_taps=%d with up/down = %d/%d needs %lld floats of LDS a tile, above %d", n_taps, up,
              down, fl, RS_LDS_FLOATS);
  SMI_REQUIRE(h->pool_used + n_taps <= RS_POOL_FLOATS, "smi_rs_register: n_taps=%d does not fit the handle's tap pool (%d of %d floats used)",
              n_taps, h->pool_used, RS_POOL_FLOATS);
  std::vector<float> t((size_t)n_taps);
  for (int i = 0; i < n_taps; ++i) t[i] = (float)taps_host[i];
  SMI_HIP(hipMemcpy(h->pool + h->pool_used, t.data(), (size_t)n_taps * sizeof(float), hipMemcpyHostToDevice));
  h->filters.push_back(Filter{up, down, half, h->pool_used});
  h->pool_used += n_taps;
  return SMI_OK;
}

long long smi_rs_out_len(long long n, int up, int down) {
  if (n < 0 || up < 1 || down < 1) return -1;
  return rs_out_len(n, up, down);
}

int smi_rs_resample_rows(smi_rs* h, const float* in_dev, long long in_stride, const int32_t* n_in_host, const int32_t* up_host,
                         const int32_t* down_host, int B, float* out_dev, long long out_stride, void* stream) {
  SMI_REQUIRE(h && in_dev && n_in_host && up_host && down_host && out_dev, "smi_rs_resample_rows: null argument");
  RsArgs A;
  int tiles = 0;
  size_t lds = 0;
  const int rc = rs_rows_args(h, "smi_rs_resample_rows", n_in_host, up_host, down_host, B, in_stride, out_stride, A, tiles, lds);
  if (rc) return rc;
  hipLaunchKernelGGL(k_rs_rows, dim3(tiles, B), dim3(RS_BLOCK), lds, (hipStream_t)stream, A, h->pool, in_dev, in_stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

int smi_rs_prompt_rows(smi_rs* h, const float* in_dev, long long in_stride, const int32_t* n_in_host, const int32_t* up_host,
                       const int32_t* down_host, int B, int normalize, float* wav_dev, long long wav_stride,
                       const int32_t* ref_len_host, float* ref_dev, long long ref_stride, double* gain_out_dev,
                       int32_t* n_out_host, void* stream) {
  SMI_REQUIRE(h && in_dev && n_in_host && up_host && down_host && wav_dev && ref_len_host && ref_dev, "smi_rs_prompt_rows: null argument");
  SMI_REQUIRE(normalize == 0 || normalize == 1, "smi_rs_prompt_rows: normalize=%d is neither 0 nor 1", normalize);
  RsArgs A;
  int tiles = 0;
  size_t lds = 0;
  const int rc = rs_rows_args(h, "smi_rs_prompt_rows", n_in_host, up_host, down_host, B, in_stride, wav_stride, A, tiles, lds);
  if (rc) return rc;
  PrArgs P;
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(ref_len_host[b] >= 1 && ref_len_host[b] <= ref_stride, "smi_rs_prompt_rows: ref_len[%d]=%d outside 1..%lld (ref_stride)", b,
                ref_len_host[b], ref_stride);
    P.r[b].n_out = A.r[b].n_out;
    P.r[b].ref_len = ref_len_host[b];
  }
  SMI_REQUIRE(ref_stride <= RS_MAX_SAMPLES, "smi_rs_prompt_rows: ref_stride=%lld above %d", ref_stride, RS_MAX_SAMPLES);
  hipLaunchKernelGGL(k_rs_rows, dim3(tiles, B), dim3(RS_BLOCK), lds, (hipStream_t)stream, A, h->pool, in_dev, in_stride, wav_dev, wav_stride);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rs_prompt, dim3(B), dim3(PR_BLOCK), 0, (hipStream_t)stream, P, normalize, wav_dev, wav_stride, ref_dev, ref_stride,
                     gain_out_dev);
  SMI_LAUNCH_CHECK();
  if (n_out_host)
    for (int b = 0; b < B; ++b) n_out_host[b] = A.r[b].n_out;
  return SMI_OK;
}

long long smi_join_piece_len(int overlap, int up, int down, int n_taps, int first, long long n_before, long long k_before, long long len,
                             int last, long long* n_after, long long* k_after) {
  if (overlap < 0 || up < 1 || down < 1 || n_taps < 1 || !(n_taps & 1) || n_before < 0 || k_before < 0 || len < 0) return -1;
  if (!last && len < 2LL * overlap) return -1;
  if (last && !first && len < overlap) return -1;
  const long long n = n_before + len - (last ? 0 : overlap);
  long long k = n;
  if (!(up == 1 && down == 1)) {
    const long long half = n_taps / 2;
    if (last) k = rs_out_len(n, up, down);
    else k = n * up <= half ? 0 : (n * up - half + down - 1) / down;
  }
  if (k < k_before) return -1;
  if (n_after) *n_after = n;
  if (k_after) *k_after = k;
  return k - k_before;
}

int smi_join_create(int max_streams, int max_chunk, int overlap, const double* fade_in_host, const double* fade_out_host, int up, int down,
                    const double* taps_host, int n_taps, smi_join** out) {
  SMI_REQUIRE(out, "smi_join_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_streams >= 1 && max_streams <= JN_MAX_STREAMS, "smi_join_create: max_streams=%d outside 1..%d", max_streams, JN_MAX_STREAMS);
  SMI_REQUIRE(max_chunk >= 1 && max_chunk <= RS_MAX_SAMPLES, "smi_join_create: max_chunk=%d outside 1..%d", max_chunk, RS_MAX_SAMPLES);
  SMI_REQUIRE(overlap >= 0 && 2LL * overlap <= max_chunk, "smi_join_create: overlap=%d outside 0..max_chunk/2 (max_chunk=%d)", overlap, max_chunk);
  SMI_REQUIRE(overlap == 0 || (fade_in_host && fade_out_host), "smi_join_create: null fade table with overlap=%d", overlap);
  SMI_REQUIRE(up >= 1 && down >= 1, "smi_join_create: up=%d, down=%d: both must be positive", up, down);
  const bool copy = up == 1 && down == 1;
  int half = 0;
  if (!copy) {
    SMI_REQUIRE(taps_host, "smi_join_create: null taps_host with up/down = %d/%d", up, down);
    SMI_REQUIRE(n_taps >= 1 && (n_taps & 1), "smi_join_create: n_taps=%d must be odd (taps h[0 .. 2H])", n_taps);
    half = n_taps / 2;
    const long long fl = (long long)n_taps + rs_window(up, down, half);
    SMI_REQUIRE(fl <= RS_LDS_FLOATS, "smi_join_create: n_taps=%d with up/down = %d/%d needs %lld floats of LDS a tile, above %d", n_taps, up,
                down, fl, RS_LDS_FLOATS);
  }
  const long long outs = rs_out_len(max_chunk, up, down) + 1;
  SMI_REQUIRE(outs <= RS_MAX_SAMPLES, "smi_join_create: max_chunk=%d at up/down = %d/%d gives pieces of %lld samples, above %d", max_chunk, up,
              down, outs, RS_MAX_SAMPLES);
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_join* h = new smi_join();
  h->max_chunk = max_chunk; h->n_taps = copy ? 1 : n_taps;
  JnState& s = h->s;
  s.max_streams = max_streams; s.overlap = overlap; s.up = up; s.down = down; s.half = half;
  s.hs = copy ? 0 : (int)((2LL * half + down + up - 1) / up) + 1;
  h->lds = copy ? 0 : ((size_t)n_taps + (size_t)rs_window(up, down, half)) * sizeof(float);
  // one allocation: the two fade tables (float64), then the taps, the two tail sets and the two history sets (fp32)
  const size_t n_tail = 2 * (size_t)max_streams * overlap, n_hist = 2 * (size_t)max_streams * s.hs;
  const size_t f64 = 2 * (size_t)overlap * sizeof(double);
  const size_t bytes = f64 + ((size_t)h->n_taps + n_tail + n_hist) * sizeof(float);
  if (h->pool.alloc(bytes, "smi_join_create: stream state")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  double* fd = (double*)h->pool.get();
  float* ff = (float*)(h->pool + f64);
  s.fade_in = fd; s.fade_out = fd + overlap;
  s.taps = ff; s.tail = ff + h->n_taps; s.hist = s.tail + n_tail;
  std::vector<float> t((size_t)h->n_taps, 0.f);
  if (!copy)
    for (int i = 0; i < n_taps; ++i) t[i] = (float)taps_host[i];
  hipError_t e = hipMemset(h->pool, 0, bytes);
  if (e == hipSuccess && overlap) e = hipMemcpy(fd, fade_in_host, (size_t)overlap * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && overlap) e = hipMemcpy(fd + overlap, fade_out_host, (size_t)overlap * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ff, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    smi_set_error("smi_join_create: upload of the fade tables and taps: %s", hipGetErrorString(e));
    delete h;
    return SMI_EHIP;
  }
  h->streams.assign((size_t)max_streams, JnStream{});
  *out = h;
  return SMI_OK;
}

int smi_join_destroy(smi_join* h) {
  delete h;
  return SMI_OK;
}

int smi_join_open(smi_join* h, int stream) {
  SMI_REQUIRE(h, "smi_join_open: null handle");
  SMI_REQUIRE(stream >= 0 && stream < h->s.max_streams, "smi_join_open: stream=%d outside 0..%d", stream, h->s.max_streams - 1);
  JnStream& st = h->streams[(size_t)stream];
  st.open = 1; st.chunks = 0; st.n = 0; st.k = 0;   // (st.set goes on alternating: a first chunk reads no state)
  return SMI_OK;
}

int smi_join_push_rows(smi_join* h, const float* chunks_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                       const int32_t* last_host, int B, float* out_dev, long long out_stride, int32_t* n_out_host, void* stream) {
  SMI_REQUIRE(h && chunks_dev && stream_host && len_host && last_host && out_dev, "smi_join_push_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_join_push_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(stride >= 1, "smi_join_push_rows: stride=%lld must be positive", stride);
  const JnState& s = h->s;
  JnArgs A;
  long long n_new[RS_MAX_ROWS], k_new[RS_MAX_ROWS], need = 1;
  for (int b = 0; b < B; ++b) {
    const int id = stream_host[b];
    SMI_REQUIRE(id >= 0 && id < s.max_streams, "smi_join_push_rows: stream[%d]=%d outside 0..%d", b, id, s.max_streams - 1);
    for (int c = 0; c < b; ++c)
      SMI_REQUIRE(stream_host[c] != id, "smi_join_push_rows: stream[%d]=%d is row %d's stream too (one chunk of a stream a call)", b, id, c);
    const JnStream& st = h->streams[(size_t)id];
    SMI_REQUIRE(st.open, "smi_join_push_rows: stream[%d]=%d is not open (smi_join_open; a stream closes with its last chunk)", b, id);
    const int len = len_host[b], last = last_host[b];
    SMI_REQUIRE(last == 0 || last == 1, "smi_join_push_rows: last[%d]=%d is neither 0 nor 1", b, last);
    SMI_REQUIRE(len >= 0 && len <= h->max_chunk && len <= stride, "smi_join_push_rows: len[%d]=%d outside 0..min(max_chunk=%d, stride=%lld)", b,
                len, h->max_chunk, stride);
    SMI_REQUIRE(last || len >= 2LL * s.overlap, "smi_join_push_rows: len[%d]=%d of a chunk that is not the last is below 2 * overlap = %d", b,
                len, 2 * s.overlap);
    SMI_REQUIRE(!last || st.chunks == 0 || len >= s.overlap, "smi_join_push_rows: len[%d]=%d of a last chunk is below overlap = %d", b, len,
                s.overlap);
    const long long piece = smi_join_piece_len(s.overlap, s.up, s.down, 2 * s.half + 1, st.chunks == 0, st.n, st.k, len, last, &n_new[b], &k_new[b]);
    SMI_REQUIRE(piece >= 0, "smi_join_push_rows: len[%d]=%d gives no valid piece", b, len);
    SMI_REQUIRE(n_new[b] * s.up < (1LL << 31) && (k_new[b] + 1) * s.down < (1LL << 31),
                "smi_join_push_rows: stream[%d]=%d would reach N * up = %lld, K * down = %lld: 2^31 is the limit of a stream", b, id,
                n_new[b] * s.up, k_new[b] * s.down);
    if (piece > 0 && s.hs > 0) {   // the first output's window starts inside the history
      const long long a0 = st.k * s.down - s.half;
      const long long jlo = a0 <= 0 ? 0 : (a0 + s.up - 1) / s.up;
      SMI_REQUIRE(jlo >= st.n - s.hs, "smi_join_push_rows: stream[%d]=%d needs %lld samples of history, the handle keeps %d", b, id,
                  st.n - jlo, s.hs);
    }
    JnRow& r = A.r[b];
    r.slot = id; r.set = st.set; r.len = len; r.n_fade = st.chunks ? s.overlap : 0;
    r.n_old = (int32_t)st.n; r.n_new = (int32_t)n_new[b]; r.k_old = (int32_t)st.k; r.k_new = (int32_t)k_new[b];
    r.keep = last ? 0 : 1;
    if (piece > need) need = piece;
  }
  SMI_REQUIRE(out_stride >= need && out_stride <= RS_MAX_SAMPLES, "smi_join_push_rows: out_stride=%lld outside %lld (the longest piece)..%d",
              out_stride, need, RS_MAX_SAMPLES);
  for (int b = 0; b < B; ++b) {
    JnStream& st = h->streams[(size_t)stream_host[b]];
    if (n_out_host) n_out_host[b] = (int32_t)(k_new[b] - st.k);
    st.n = n_new[b]; st.k = k_new[b]; st.chunks += 1; st.set ^= 1;
    if (last_host[b]) st.open = 0;
  }
  const int tiles = (int)((out_stride + RS_TILE - 1) / RS_TILE);
  hipLaunchKernelGGL(k_join_rows, dim3(tiles, B), dim3(RS_BLOCK), h->lds, (hipStream_t)stream, A, h->s, chunks_dev, stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

long long smi_trim_work_len(long long n_max, int window, int step, int B) {
  if (n_max < 0 || n_max > RS_MAX_SAMPLES || window < 1 || step < 1 || B < 1 || B > RS_MAX_ROWS) return -1;
  const long long nwin = n_max >= window ? (n_max - window) / step + 1 : 0;
  const long long tiles = nwin ? (nwin + TR_TILE - 1) / TR_TILE : 1;
  return 2 * tiles * B;
}

int smi_trim_rows(const float* in_dev, long long in_stride, const int32_t* n_host, int B, int window, int step, double threshold,
                  int margin, int32_t* work_dev, long long work_len, int32_t* bounds_dev, void* stream) {
  SMI_REQUIRE(in_dev && n_host && work_dev && bounds_dev, "smi_trim_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_trim_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(window >= 1 && window <= RS_MAX_SAMPLES, "smi_trim_rows: window=%d outside 1..%d", window, RS_MAX_SAMPLES);
  SMI_REQUIRE(step >= 1 && step <= RS_MAX_SAMPLES, "smi_trim_rows: step=%d outside 1..%d", step, RS_MAX_SAMPLES);
  SMI_REQUIRE((long long)(TR_TILE - 1) * step + window <= TR_LDS_FLOATS,
              "smi_trim_rows: window=%d with step=%d: %d windows span %lld samples, above %d (the kernel stages them in 64 KiB of LDS)", window,
              step, TR_TILE, (long long)(TR_TILE - 1) * step + window, TR_LDS_FLOATS);
  SMI_REQUIRE(threshold >= 0.0 && threshold <= 1e150, "smi_trim_rows: threshold=%g outside 0..1e150", threshold);   // (NaN fails too)
  SMI_REQUIRE(margin >= 0 && margin <= RS_MAX_SAMPLES, "smi_trim_rows: margin=%d outside 0..%d", margin, RS_MAX_SAMPLES);
  SMI_REQUIRE(in_stride >= 1, "smi_trim_rows: in_stride=%lld must be positive", in_stride);
  TrArgs A;
  int n_max = 0;
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(n_host[b] >= 0 && n_host[b] <= RS_MAX_SAMPLES && n_host[b] <= in_stride, "smi_trim_rows: n[%d]=%d outside 0..min(%d, in_stride=%lld)",
                b, n_host[b], RS_MAX_SAMPLES, in_stride);
    A.n[b] = n_host[b];
    if (n_host[b] > n_max) n_max = n_host[b];
  }
  const long long need = smi_trim_work_len(n_max, window, step, B);
  SMI_REQUIRE(work_len >= need, "smi_trim_rows: work_len=%lld below %lld (smi_trim_work_len)", work_len, need);
  const int tiles = (int)(need / (2 * B));
  const size_t lds = ((size_t)(TR_TILE - 1) * step + window) * sizeof(float);
  hipLaunchKernelGGL(k_trim_scan, dim3(tiles, B), dim3(TR_BLOCK), lds, (hipStream_t)stream, A, in_dev, in_stride, window, step,
                     threshold * threshold * (double)window, tiles, work_dev);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_trim_bounds, dim3(B), dim3(64), 0, (hipStream_t)stream, A, window, step, margin, tiles, work_dev, bounds_dev);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

long long smi_concat_layout(const int32_t* start_host, const int32_t* end_host, const int32_t* gap_host, int B, long long* offset_host) {
  if (!start_host || !end_host || !gap_host || B < 1 || B > RS_MAX_ROWS) return -1;
  long long total = 0;
  for (int b = 0; b < B; ++b) {
    if (start_host[b] < 0 || end_host[b] < start_host[b] || gap_host[b] < 0) return -1;
    if (end_host[b] > start_host[b]) total += gap_host[b];
    if (offset_host) offset_host[b] = total;
    total += end_host[b] - start_host[b];
  }
  return total;
}

int smi_concat_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host,
                    const int32_t* gap_host, int B, int fade, float* out_dev, long long cap, long long* offset_host, long long* total_host,
                    void* stream) {
  SMI_REQUIRE(in_dev && n_host && start_host && end_host && gap_host && out_dev, "smi_concat_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_concat_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(fade >= 0 && fade <= RS_MAX_SAMPLES, "smi_concat_rows: fade=%d outside 0..%d", fade, RS_MAX_SAMPLES);
  SMI_REQUIRE(in_stride >= 1, "smi_concat_rows: in_stride=%lld must be positive", in_stride);
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(n_host[b] >= 0 && n_host[b] <= RS_MAX_SAMPLES && n_host[b] <= in_stride,
                "smi_concat_rows: n[%d]=%d outside 0..min(%d, in_stride=%lld)", b, n_host[b], RS_MAX_SAMPLES, in_stride);
    SMI_REQUIRE(start_host[b] >= 0, "smi_concat_rows: start[%d]=%d is negative", b, start_host[b]);
    SMI_REQUIRE(end_host[b] >= start_host[b], "smi_concat_rows: end[%d]=%d below start[%d]=%d", b, end_host[b], b, start_host[b]);
    SMI_REQUIRE(end_host[b] <= n_host[b], "smi_concat_rows: end[%d]=%d above n[%d]=%d", b, end_host[b], b, n_host[b]);
    SMI_REQUIRE(gap_host[b] >= 0 && gap_host[b] <= RS_MAX_SAMPLES, "smi_concat_rows: gap[%d]=%d outside 0..%d", b, gap_host[b], RS_MAX_SAMPLES);
  }
  long long off[RS_MAX_ROWS];
  const long long total = smi_concat_layout(start_host, end_host, gap_host, B, off);
  SMI_REQUIRE(cap >= 1 && cap >= total && cap < (1LL << 31), "smi_concat_rows: cap=%lld outside max(1, the total length %lld)..2^31 - 1", cap, total);
  CcArgs A;
  long long longest = cap - total;
  for (int b = 0; b < B; ++b) {
    CcRow& r = A.r[b];
    r.src = start_host[b]; r.len = end_host[b] - start_host[b]; r.off = (int32_t)off[b];
    r.lead = r.len ? gap_host[b] : 0;
    r.fade = fade < r.len / 2 ? fade : r.len / 2;
    if ((long long)r.lead + r.len > longest) longest = (long long)r.lead + r.len;
    if (offset_host) offset_host[b] = off[b];
  }
  if (total_host) *total_host = total;
  const int tiles = longest ? (int)((longest + CC_TILE - 1) / CC_TILE) : 1;
  hipLaunchKernelGGL(k_concat_rows, dim3(tiles, B + 1), dim3(RS_BLOCK), 0, (hipStream_t)stream, A, B, in_dev, in_stride, out_dev, total, cap);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// where the parts of one row's scratch lie; the total is smi_loud_work_len
static LdLayout ld_layout(long long n_max, int block) {
  const int hop = block / 4;
  const long long nseg = n_max ? (n_max + LD_SEG - 1) / LD_SEG : 1, nhop = n_max ? (n_max + hop - 1) / hop : 1;
  LdLayout l;
  l.pps = (LD_SEG - 1) / hop + 2;
  l.e = 0;
  l.s = l.e + 4 * nseg;
  l.pk = l.s + 4 * nseg;
  l.parts = l.pk + nseg;
  l.hops = l.parts + nseg * l.pps;
  l.row = l.hops + nhop;
  return l;
}

// the rows of a loudness / gain call: every check, then the descriptors
static int ld_rows_args(const char* who, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B, long long in_stride,
                        LdArgs& A, int& n_max, int& len_max) {
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "%s: B=%d outside 1..%d", who, B, RS_MAX_ROWS);
  SMI_REQUIRE((start_host == nullptr) == (end_host == nullptr), "%s: start_host and end_host must both be given or both be null", who);
  SMI_REQUIRE(in_stride >= 1, "%s: in_stride=%lld must be positive", who, in_stride);
  n_max = 0; len_max = 0;
  for (int b = 0; b < B; ++b) {
    const int n = n_host[b];
    SMI_REQUIRE(n >= 0 && n <= RS_MAX_SAMPLES && n <= in_stride, "%s: n[%d]=%d outside 0..min(%d, in_stride=%lld)", who, b, n, RS_MAX_SAMPLES,
                in_stride);
    const int st = start_host ? start_host[b] : 0, en = end_host ? end_host[b] : n;
    SMI_REQUIRE(st >= 0, "%s: start[%d]=%d is negative", who, b, st);
    SMI_REQUIRE(en >= st, "%s: end[%d]=%d below start[%d]=%d", who, b, en, b, st);
    SMI_REQUIRE(en <= n, "%s: end[%d]=%d above n[%d]=%d", who, b, en, b, n);
    A.r[b].n = n; A.r[b].start = st; A.r[b].len = en - st;
    if (n > n_max) n_max = n;
    if (en - st > len_max) len_max = en - st;
  }
  return SMI_OK;
}

extern "C" {

long long smi_loud_work_len(long long n_max, int block, int B) {
  if (n_max < 0 || n_max > RS_MAX_SAMPLES || block < 4 || block > RS_MAX_SAMPLES || (block & 3) || B < 1 || B > RS_MAX_ROWS) return -1;
  return ld_layout(n_max, block).row * B;
}

int smi_loud_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                  const double* coef_host, int block, const double* target_host, double max_gain_db, double ceiling, double* work_dev,
                  long long work_len, double* stats_dev, void* stream) {
  SMI_REQUIRE(in_dev && n_host && coef_host && target_host && work_dev && stats_dev, "smi_loud_rows: null argument");
  SMI_REQUIRE(block >= 4 && block <= RS_MAX_SAMPLES && !(block & 3), "smi_loud_rows: block=%d must be a multiple of 4 in 4..%d", block,
              RS_MAX_SAMPLES);
  for (int i = 0; i < 10; ++i)
    SMI_REQUIRE(std::isfinite(coef_host[i]), "smi_loud_rows: coef[%d]=%g is not finite", i, coef_host[i]);
  SMI_REQUIRE(std::isfinite(max_gain_db) && max_gain_db >= 0.0, "smi_loud_rows: max_gain_db=%g must be finite and >= 0", max_gain_db);
  SMI_REQUIRE(std::isfinite(ceiling) && ceiling > 0.0, "smi_loud_rows: ceiling=%g must be finite and > 0", ceiling);
  LdArgs A;
  int n_max = 0, len_max = 0;
  const int rc = ld_rows_args("smi_loud_rows", n_host, start_host, end_host, B, in_stride, A, n_max, len_max);
  if (rc) return rc;
  LdTargets T;
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(!std::isinf(target_host[b]), "smi_loud_rows: target[%d]=%g must be finite, or NaN to measure only", b, target_host[b]);
    T.t[b] = target_host[b];
  }
  const long long need = smi_loud_work_len(n_max, block, B);
  SMI_REQUIRE(work_len >= need, "smi_loud_rows: work_len=%lld below %lld (smi_loud_work_len)", work_len, need);
  const LdLayout lay = ld_layout(n_max, block);
  LdCoef c;
  for (int st = 0; st < 2; ++st) {
    for (int i = 0; i < 3; ++i) c.b[st][i] = coef_host[5 * st + i];
    c.a1[st] = coef_host[5 * st + 3];
    c.a2[st] = coef_host[5 * st + 4];
  }
  ld_transition(c);
  const double abs_gate = pow(10.0, (-70.0 + 0.691) / 10.0);
  const int tiles = len_max ? (len_max + LD_TILE - 1) / LD_TILE : 1;
  const size_t lds = (size_t)LD_LANES * LD_PITCH * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_loud_seg, dim3(tiles, B), dim3(LD_LANES), lds, s, A, c, in_dev, in_stride, work_dev, lay);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loud_carry, dim3(B), dim3(64), 0, s, A, c, work_dev, lay);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loud_energy, dim3(tiles, B), dim3(LD_LANES), lds, s, A, c, block / 4, in_dev, in_stride, work_dev, lay);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loud_gate, dim3(B), dim3(LD_GATE), 0, s, A, T, block, abs_gate, max_gain_db, ceiling, work_dev, lay, stats_dev);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

int smi_gain_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                  const double* stats_dev, float* out_dev, long long out_stride, void* stream) {
  SMI_REQUIRE(in_dev && n_host && stats_dev && out_dev, "smi_gain_rows: null argument");
  LdArgs A;
  int n_max = 0, len_max = 0;
  const int rc = ld_rows_args("smi_gain_rows", n_host, start_host, end_host, B, in_stride, A, n_max, len_max);
  if (rc) return rc;
  SMI_REQUIRE(out_stride >= 1 && out_stride >= n_max && out_stride <= RS_MAX_SAMPLES, "smi_gain_rows: out_stride=%lld outside max(1, the longest row %d)..%d",
              out_stride, n_max, RS_MAX_SAMPLES);
  if (!(out_dev == in_dev && out_stride == in_stride)) {   // in place, row on row, or apart
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + ((size_t)(B - 1) * in_stride + n_max) * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_gain_rows: out_dev overlaps in_dev (only out_dev == in_dev with equal strides is allowed)");
  }
  const int tiles = (int)((out_stride + GN_TILE - 1) / GN_TILE);
  hipLaunchKernelGGL(k_gain_rows, dim3(tiles, B), dim3(RS_BLOCK), 0, (hipStream_t)stream, A, stats_dev, in_dev, in_stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// where the parts of the limiter's scratch lie: the window, then per row r [n_max] and three values a tile
static LmLayout lm_layout(long long n_max) {
  const long long tiles = n_max ? (n_max + LM_TILE - 1) / LM_TILE : 1;
  LmLayout l;
  l.rows = LM_WIN_PAD;
  l.emax = (n_max + 7) / 8 * 8;
  l.smin = l.emax + tiles;
  l.cnt = l.smin + tiles;
  l.row = (l.cnt + tiles + 7) / 8 * 8;
  return l;
}

extern "C" {

long long smi_limit_work_len(long long n_max, int B) {
  if (n_max < 0 || n_max > RS_MAX_SAMPLES || B < 1 || B > RS_MAX_ROWS) return -1;
  const LmLayout l = lm_layout(n_max);
  return l.rows + l.row * B;
}

int smi_limit_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const double* gain_dev, int gain_stride, double ceiling, const double* taps_host, int n_taps, int phases, int lookahead,
                   int release, const double* win_host, double* work_dev, long long work_len, float* out_dev, long long out_stride,
                   double* stats_dev, void* stream) {
  SMI_REQUIRE(in_dev && n_host && win_host && work_dev && out_dev && stats_dev, "smi_limit_rows: null argument");
  SMI_REQUIRE(std::isfinite(ceiling) && ceiling > 0.0, "smi_limit_rows: ceiling=%g must be finite and > 0", ceiling);
  SMI_REQUIRE(phases >= 1 && phases <= LM_MAX_PHASES, "smi_limit_rows: phases=%d outside 1..%d", phases, LM_MAX_PHASES);
  SMI_REQUIRE(n_taps == 0 || n_taps == 2 * LM_HALO * phases + 1,
              "smi_limit_rows: n_taps=%d is neither 0 (the sample peak) nor %d = 2 * 10 * phases + 1 for phases=%d", n_taps,
              2 * LM_HALO * phases + 1, phases);
  SMI_REQUIRE(n_taps == 0 || taps_host, "smi_limit_rows: null taps_host with n_taps=%d", n_taps);
  for (int i = 0; i < n_taps; ++i) SMI_REQUIRE(std::isfinite(taps_host[i]), "smi_limit_rows: taps[%d]=%g is not finite", i, taps_host[i]);
  SMI_REQUIRE(lookahead >= 0 && lookahead <= LM_MAX_A, "smi_limit_rows: lookahead=%d outside 0..%d", lookahead, LM_MAX_A);
  SMI_REQUIRE(release >= 0 && release <= LM_MAX_R, "smi_limit_rows: release=%d outside 0..%d", release, LM_MAX_R);
  const int nw = lookahead + release + 1;
  double wsum = 0.0;
  for (int i = 0; i < nw; ++i) {
    SMI_REQUIRE(std::isfinite(win_host[i]) && win_host[i] >= 0.0, "smi_limit_rows: win[%d]=%g must be finite and >= 0", i, win_host[i]);
    wsum = wsum + win_host[i];
  }
  SMI_REQUIRE(std::fabs(wsum - 1.0) <= 1e-12, "smi_limit_rows: win sums to 1%+.3g over its %d weights, not to 1 within 1e-12", wsum - 1.0, nw);
  SMI_REQUIRE(gain_stride >= 0, "smi_limit_rows: gain_stride=%d is negative", gain_stride);
  LdArgs A;
  int n_max = 0, len_max = 0;
  const int rc = ld_rows_args("smi_limit_rows", n_host, start_host, end_host, B, in_stride, A, n_max, len_max);
  if (rc) return rc;
  SMI_REQUIRE(out_stride >= 1 && out_stride >= n_max && out_stride <= RS_MAX_SAMPLES,
              "smi_limit_rows: out_stride=%lld outside max(1, the longest row %d)..%d", out_stride, n_max, RS_MAX_SAMPLES);
  if (!(out_dev == in_dev && out_stride == in_stride)) {   // in place, row on row, or apart
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + ((size_t)(B - 1) * in_stride + n_max) * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_limit_rows: out_dev overlaps in_dev (only out_dev == in_dev with equal strides is allowed)");
  }
  if (gain_dev) {
    const double* g1 = gain_dev + (size_t)(B - 1) * gain_stride + 1;
    SMI_REQUIRE(g1 <= stats_dev || stats_dev + 4 * (size_t)B <= gain_dev, "smi_limit_rows: stats_dev overlaps gain_dev");
  }
  const long long need = smi_limit_work_len(n_max, B);
  SMI_REQUIRE(work_len >= need, "smi_limit_rows: work_len=%lld below %lld (smi_limit_work_len)", work_len, need);
  const LmLayout lay = lm_layout(n_max);
  LmTaps tp;
  for (int i = 0; i < LM_MAX_TAPS; ++i) tp.h[i] = i < n_taps ? taps_host[i] : 0.0;
  tp.n = n_taps; tp.phases = phases;
  float c32 = (float)ceiling;   // the largest float32 <= ceiling
  if ((double)c32 > ceiling) c32 = nextafterf(c32, 0.f);
  hipStream_t s = (hipStream_t)stream;
  for (int o = 0; o < nw; o += LM_WIN_ARG) {
    LmWin w;
    const int cnt = nw - o < LM_WIN_ARG ? nw - o : LM_WIN_ARG;
    for (int i = 0; i < LM_WIN_ARG; ++i) w.w[i] = i < cnt ? win_host[o + i] : 0.0;
    hipLaunchKernelGGL(k_limit_win, dim3(1), dim3(RS_BLOCK), 0, s, w, cnt, work_dev + o);
    SMI_LAUNCH_CHECK();
  }
  const int etiles = len_max ? (len_max + LM_TILE - 1) / LM_TILE : 1;
  hipLaunchKernelGGL(k_limit_env, dim3(etiles, B), dim3(RS_BLOCK), 0, s, A, tp, gain_dev, gain_stride, ceiling, in_dev, in_stride, work_dev, lay);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + LM_TILE - 1) / LM_TILE);
  const size_t lds = (size_t)(LM_TILE + 2 * (lookahead + release)) * sizeof(double);
  hipLaunchKernelGGL(k_limit_apply, dim3(tiles, B), dim3(RS_BLOCK), lds, s, A, lookahead, release, gain_dev, gain_stride, c32,
                     (const double*)work_dev, in_dev, in_stride, (const double*)(work_dev + lay.rows), work_dev + lay.rows, lay, out_dev,
                     out_stride);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_limit_stats, dim3(B), dim3(RS_BLOCK), 0, s, A, gain_dev, gain_stride, (const double*)work_dev, lay, stats_dev);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// the lengths of a time-scaled span: M = ceil(L q / p) samples in K frames of N / 2; false for a bad argument
static bool tp_layout(long long L, int p, int q, int N, long long& M, long long& K) {
  if (L < 0 || L > RS_MAX_SAMPLES || p < 1 || p > 32767 || q < 1 || q > 32767 || p > 4 * q || q > 4 * p) return false;
  if (N < 16 || N > TP_MAX_N || (N & 1)) return false;
  M = (L * q + p - 1) / p;
  K = M ? (M - 1) / (N / 2) + 1 : 0;
  return true;
}

extern "C" {

long long smi_tempo_layout(long long L, int p, int q, int N, long long* K_out) {
  long long M = 0, K = 0;
  if (!tp_layout(L, p, q, N, M, K)) return -1;
  if (K_out) *K_out = K;
  return M;
}

int smi_tempo_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const int32_t* p_host, const int32_t* q_host, int N, int D, const double* win_dev, int32_t* pos_dev, long long pos_stride,
                   float* out_dev, long long out_stride, int32_t* m_host, void* stream) {
  SMI_REQUIRE(N >= 16 && N <= TP_MAX_N && !(N & 1), "smi_tempo_rows: N=%d must be even in 16..%d", N, TP_MAX_N);
  SMI_REQUIRE(D >= 0 && D <= TP_MAX_D, "smi_tempo_rows: D=%d outside 0..%d", D, TP_MAX_D);
  SMI_REQUIRE(in_dev && n_host && p_host && q_host && win_dev && pos_dev && out_dev, "smi_tempo_rows: null argument");
  LdArgs S;
  int n_max = 0, len_max = 0;
  const int rc = ld_rows_args("smi_tempo_rows", n_host, start_host, end_host, B, in_stride, S, n_max, len_max);
  if (rc) return rc;
  TpArgs A;
  long long m_max = 0, k_max = 0;
  for (int b = 0; b < B; ++b) {
    const int p = p_host[b], q = q_host[b];
    SMI_REQUIRE(p >= 1 && p <= 32767, "smi_tempo_rows: p[%d]=%d outside 1..32767", b, p);
    SMI_REQUIRE(q >= 1 && q <= 32767, "smi_tempo_rows: q[%d]=%d outside 1..32767", b, q);
    SMI_REQUIRE(p <= 4 * q && q <= 4 * p, "smi_tempo_rows: p[%d]/q[%d] = %d/%d outside 1/4..4", b, b, p, q);
    long long M = 0, K = 0;
    SMI_REQUIRE(tp_layout(S.r[b].len, p, q, N, M, K), "smi_tempo_rows: row %d has no layout (smi_tempo_layout)", b);
    TpRow& r = A.r[b];
    r.start = S.r[b].start; r.len = S.r[b].len; r.p = p; r.q = q; r.m = (int32_t)M; r.frames = (int32_t)K;
    if (M > m_max) m_max = M;
    if (K > k_max) k_max = K;
  }
  SMI_REQUIRE(out_stride >= 1 && out_stride >= m_max && out_stride <= TP_MAX_OUT,
              "smi_tempo_rows: out_stride=%lld outside max(1, the longest output row %lld)..%d", out_stride, m_max, TP_MAX_OUT);
  SMI_REQUIRE(pos_stride >= 1 && pos_stride >= k_max && pos_stride <= TP_MAX_OUT,
              "smi_tempo_rows: pos_stride=%lld outside max(1, the most frames of a row %lld)..%d", pos_stride, k_max, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + ((size_t)(B - 1) * in_stride + n_max) * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_tempo_rows: out_dev overlaps in_dev");
  }
  if (m_host)
    for (int b = 0; b < B; ++b) m_host[b] = A.r[b].m;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tempo_search, dim3(B), dim3(TP_BLOCK), 0, s, A, N, D, in_dev, in_stride, pos_dev, pos_stride);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + TP_TILE - 1) / TP_TILE);
  hipLaunchKernelGGL(k_tempo_ola, dim3(tiles, B), dim3(RS_BLOCK), 0, s, A, N, in_dev, in_stride, win_dev, pos_dev, pos_stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// ---- pitch shift of rows (smi_pitch_*)
struct PtPlan {
  int P, Q, up, down;
  long long M, K, n_out;
};

static long long pt_gcd(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}

// the plan of a span of L samples at tempo tp / tq and pitch ratio rp / rq: the stretch P / Q = (tp rq) / (tq rp) in lowest
// terms with its M and K, the resampling up / down = rq / rp in lowest terms, and n_out = ceil(L tq / tp); false for a bad argument
static bool pt_plan(long long L, int tp, int tq, int rp, int rq, int N, PtPlan& pl) {
  if (tp < 1 || tp > 32767 || tq < 1 || tq > 32767 || rp < 1 || rp > 32767 || rq < 1 || rq > 32767) return false;
  const long long a = (long long)tp * rq, b = (long long)tq * rp, g = pt_gcd(a, b), gr = pt_gcd(rp, rq);
  if (a / g > 32767 || b / g > 32767) return false;
  pl.P = (int)(a / g); pl.Q = (int)(b / g);
  pl.up = (int)(rq / gr); pl.down = (int)(rp / gr);
  if (!tp_layout(L, pl.P, pl.Q, N, pl.M, pl.K)) return false;
  pl.n_out = (L * tq + tp - 1) / tp;
  return true;
}

extern "C" {

long long smi_pitch_layout(long long L, int tp, int tq, int rp, int rq, int N, int* P_out, int* Q_out, long long* M_out, long long* K_out,
                           int* up_out, int* down_out) {
  PtPlan pl;
  if (!pt_plan(L, tp, tq, rp, rq, N, pl)) return -1;
  if (P_out) *P_out = pl.P;
  if (Q_out) *Q_out = pl.Q;
  if (M_out) *M_out = pl.M;
  if (K_out) *K_out = pl.K;
  if (up_out) *up_out = pl.up;
  if (down_out) *down_out = pl.down;
  return pl.n_out;
}

int smi_pitch_rows(const float* in_dev, long long in_stride, const int32_t* n_host, const int32_t* start_host, const int32_t* end_host, int B,
                   const int32_t* tp_host, const int32_t* tq_host, const int32_t* rp_host, const int32_t* rq_host, int N, int D,
                   const double* win_dev, const float* taps_dev, long long taps_len, const int32_t* tap_off_host, const int32_t* n_taps_host,
                   int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride, int32_t* m_host, void* stream) {
  SMI_REQUIRE(N >= 16 && N <= TP_MAX_N && !(N & 1), "smi_pitch_rows: N=%d must be even in 16..%d", N, TP_MAX_N);
  SMI_REQUIRE(D >= 0 && D <= TP_MAX_D, "smi_pitch_rows: D=%d outside 0..%d", D, TP_MAX_D);
  SMI_REQUIRE(in_dev && n_host && tp_host && tq_host && rp_host && rq_host && win_dev && tap_off_host && n_taps_host && pos_dev && out_dev,
              "smi_pitch_rows: null argument");
  SMI_REQUIRE(taps_len >= 0 && (taps_dev || !taps_len), "smi_pitch_rows: taps_len=%lld needs a pool (taps_dev is null)", taps_len);
  LdArgs S;
  int n_max = 0, len_max = 0;
  const int rc = ld_rows_args("smi_pitch_rows", n_host, start_host, end_host, B, in_stride, S, n_max, len_max);
  if (rc) return rc;
  TpArgs A;
  PtArgs F;
  long long m_max = 0, k_max = 0;
  size_t lds = 0;
  for (int b = 0; b < B; ++b) {
    const int tp = tp_host[b], tq = tq_host[b], rp = rp_host[b], rq = rq_host[b];
    SMI_REQUIRE(tp >= 1 && tp <= 32767, "smi_pitch_rows: tp[%d]=%d outside 1..32767", b, tp);
    SMI_REQUIRE(tq >= 1 && tq <= 32767, "smi_pitch_rows: tq[%d]=%d outside 1..32767", b, tq);
    SMI_REQUIRE(rp >= 1 && rp <= 32767, "smi_pitch_rows: rp[%d]=%d outside 1..32767", b, rp);
    SMI_REQUIRE(rq >= 1 && rq <= 32767, "smi_pitch_rows: rq[%d]=%d outside 1..32767", b, rq);
    PtPlan pl;
    SMI_REQUIRE(pt_plan(S.r[b].len, tp, tq, rp, rq, N, pl),
                "smi_pitch_rows: row %d has no layout (smi_pitch_layout): the stretch (tp[%d] rq[%d]) / (tq[%d] rp[%d]) = (%d * %d) / (%d * %d) "
                "must lie in 1/4..4 with terms up to 32767", b, b, b, b, b, tp, rq, tq, rp);
    TpRow& r = A.r[b];
    r.start = S.r[b].start; r.len = S.r[b].len; r.p = pl.P; r.q = pl.Q; r.m = (int32_t)pl.M; r.frames = (int32_t)pl.K;
    PtRow& g = F.r[b];
    g.n_out = (int32_t)pl.n_out; g.up = pl.up; g.down = pl.down; g.half = 0; g.tap_off = 0;
    const int nt = n_taps_host[b], off = tap_off_host[b];
    if (pl.up == 1 && pl.down == 1) {
      SMI_REQUIRE(nt == 0, "smi_pitch_rows: n_taps[%d]=%d must be 0 for a row whose pitch ratio is 1/1", b, nt);
    } else {
      SMI_REQUIRE(nt >= 3 && (nt & 1), "smi_pitch_rows: n_taps[%d]=%d must be odd and at least 3 (taps h[0 .. 2H], H >= 1) for a row at rp/rq = %d/%d",
                  b, nt, rp, rq);
      SMI_REQUIRE(off >= 0 && (long long)off + nt <= taps_len, "smi_pitch_rows: tap_off[%d]=%d with n_taps[%d]=%d leaves the pool of taps_len=%lld",
                  b, off, b, nt, taps_len);
      const long long fl = (long long)nt + rs_window(pl.up, pl.down, nt / 2);
      SMI_REQUIRE(fl <= RS_LDS_FLOATS, "smi_pitch_rows: n_taps[%d]=%d with up/down = %d/%d needs %lld floats of LDS a tile, above %d", b, nt,
                  pl.up, pl.down, fl, RS_LDS_FLOATS);
      SMI_REQUIRE(pl.M * pl.up < (1LL << 31), "smi_pitch_rows: M * up = %lld of row %d reaches 2^31", pl.M * pl.up, b);
      SMI_REQUIRE(pl.n_out * pl.down < (1LL << 31), "smi_pitch_rows: n_out * down = %lld of row %d reaches 2^31", pl.n_out * pl.down, b);
      SMI_REQUIRE(rs_out_len(pl.M, pl.up, pl.down) >= pl.n_out, "smi_pitch_rows: row %d: the stretched span resamples to %lld samples, below n_out=%lld",
                  b, rs_out_len(pl.M, pl.up, pl.down), pl.n_out);
      g.half = nt / 2; g.tap_off = off;
      if ((size_t)fl > lds) lds = (size_t)fl;
    }
    if (pl.n_out > m_max) m_max = pl.n_out;
    if (pl.K > k_max) k_max = pl.K;
  }
  SMI_REQUIRE(out_stride >= 1 && out_stride >= m_max && out_stride <= TP_MAX_OUT,
              "smi_pitch_rows: out_stride=%lld outside max(1, the longest output row %lld)..%d", out_stride, m_max, TP_MAX_OUT);
  SMI_REQUIRE(pos_stride >= 1 && pos_stride >= k_max && pos_stride <= TP_MAX_OUT,
              "smi_pitch_rows: pos_stride=%lld outside max(1, the most frames of a row %lld)..%d", pos_stride, k_max, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + ((size_t)(B - 1) * in_stride + n_max) * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_pitch_rows: out_dev overlaps in_dev");
    const char* t0 = (const char*)taps_dev;
    const char* t1 = t0 + (size_t)taps_len * sizeof(float);
    SMI_REQUIRE(!taps_len || t1 <= o0 || o1 <= t0, "smi_pitch_rows: out_dev overlaps taps_dev");
  }
  if (m_host)
    for (int b = 0; b < B; ++b) m_host[b] = F.r[b].n_out;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tempo_search, dim3(B), dim3(TP_BLOCK), 0, s, A, N, D, in_dev, in_stride, pos_dev, pos_stride);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + RS_TILE - 1) / RS_TILE);
  hipLaunchKernelGGL(k_pitch_ola, dim3(tiles, B), dim3(RS_BLOCK), lds * sizeof(float), s, A, F, N, in_dev, in_stride, win_dev, taps_dev, pos_dev,
                     pos_stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// ---- tempo of joined streams (smi_tempos_*): the host arithmetic of include/sparkmi.h's "when a frame is final"
#define TS_MAX_N (1LL << 28)   // input samples of one stream: M <= 2^30 and every place stay inside int32

static bool ts_args(int p, int q, int N, int D) {
  return p >= 1 && p <= 32767 && q >= 1 && q <= 32767 && p <= 4 * q && q <= 4 * p && N >= 16 && N <= TP_MAX_N && !(N & 1) && D >= 0 &&
         D <= TP_MAX_D;
}

static long long ts_nominal(long long k, int p, int q, int H) { return (k * H * p) / q; }

// R_k: the input samples a stream must hold before frame k is final
static long long ts_ready(long long k, int p, int q, int H, int D) {
  if (k == 0) return H;
  const long long a = ts_nominal(k, p, q, H), b = ts_nominal(k - 1, p, q, H) + H;
  return (a > b ? a : b) + D + 2LL * H;
}

// the first input sample frame k can still read: where the history of a stream that has emitted k frames begins
static long long ts_hist_start(long long k, int p, int q, int H, int D) {
  if (k == 0) return 0;
  const long long a = ts_nominal(k, p, q, H), b = ts_nominal(k - 1, p, q, H) + H;
  const long long lo = (a < b ? a : b) - D;
  return lo > 0 ? lo : 0;
}

// the samples of history a stream can hold between two pushes, whatever p / q in 1/4 .. 4 (include/sparkmi.h derives it)
static int ts_hist_cap(int N, int D) {
  const int H = N / 2, a = 7 * H + D, b = 5 * H + 2 * D;
  return a > b ? a : b;
}

struct TsStream {
  int open = 0, set = 0, p = 1, q = 1;
  long long n = 0, f = 0;   // input samples so far, frames emitted
};
struct smi_tempos {
  TsState s;
  int max_chunk, N, D;
  DevBuf<char> pool;
  std::vector<TsStream> streams;
};

extern "C" {

long long smi_tempos_piece_len(int p, int q, int N, int D, long long n_before, long long frames_before, long long len, int last,
                               long long* n_after, long long* frames_after) {
  if (!ts_args(p, q, N, D) || n_before < 0 || frames_before < 0 || len < 0 || n_before > TS_MAX_N || len > TS_MAX_N) return -1;
  if (last != 0 && last != 1) return -1;
  const int H = N / 2;
  const long long n = n_before + len;
  const long long M = (n * q + p - 1) / p;
  long long f, piece;
  if (p == q) {   // a copy: everything at once
    f = last ? (M ? (M - 1) / H + 1 : 0) : n / H;
    piece = len;
  } else if (last) {
    f = M ? (M - 1) / H + 1 : 0;
    piece = M - frames_before * H;
  } else {
    f = frames_before;
    while ((f + 1) * H <= M && n >= ts_ready(f, p, q, H, D)) ++f;
    piece = (f - frames_before) * H;
  }
  if (piece < 0 || f < frames_before) return -1;
  if (n_after) *n_after = n;
  if (frames_after) *frames_after = f;
  return piece;
}

int smi_tempos_create(int max_streams, int max_chunk, int N, int D, const double* win_host, smi_tempos** out) {
  SMI_REQUIRE(out, "smi_tempos_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_streams >= 1 && max_streams <= JN_MAX_STREAMS, "smi_tempos_create: max_streams=%d outside 1..%d", max_streams, JN_MAX_STREAMS);
  SMI_REQUIRE(max_chunk >= 1 && max_chunk <= RS_MAX_SAMPLES, "smi_tempos_create: max_chunk=%d outside 1..%d", max_chunk, RS_MAX_SAMPLES);
  SMI_REQUIRE(N >= 16 && N <= TP_MAX_N && !(N & 1), "smi_tempos_create: N=%d must be even in 16..%d", N, TP_MAX_N);
  SMI_REQUIRE(D >= 0 && D <= TP_MAX_D, "smi_tempos_create: D=%d outside 0..%d", D, TP_MAX_D);
  SMI_REQUIRE(win_host, "smi_tempos_create: null win_host");
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_tempos* h = new smi_tempos();
  h->max_chunk = max_chunk; h->N = N; h->D = D;
  TsState& s = h->s;
  s.max_streams = max_streams;
  s.hcap = ts_hist_cap(N, D);
  s.fmax = (int)(4LL * ((long long)max_chunk + s.hcap) / (N / 2) + 4);   // frames one push can emit
  // one allocation: the window (float64), then the two history sets (fp32), the two sets of places and the frames' work (int32)
  const size_t f64 = (size_t)N * sizeof(double);
  const size_t n_hist = 2 * (size_t)max_streams * s.hcap, n_pos = 2 * (size_t)max_streams, n_work = (size_t)RS_MAX_ROWS * (s.fmax + 1);
  const size_t bytes = f64 + n_hist * sizeof(float) + (n_pos + n_work) * sizeof(int32_t);
  if (h->pool.alloc(bytes, "smi_tempos_create: stream state")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  s.win = (const double*)h->pool.get();
  s.hist = (float*)(h->pool + f64);
  s.spos = (int32_t*)(s.hist + n_hist);
  s.work = s.spos + n_pos;
  hipError_t e = hipMemset(h->pool, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->pool, win_host, f64, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    smi_set_error("smi_tempos_create: upload of the window: %s", hipGetErrorString(e));
    delete h;
    return SMI_EHIP;
  }
  h->streams.assign((size_t)max_streams, TsStream{});
  *out = h;
  return SMI_OK;
}

int smi_tempos_destroy(smi_tempos* h) {
  delete h;
  return SMI_OK;
}

int smi_tempos_open(smi_tempos* h, int stream, int p, int q) {
  SMI_REQUIRE(h, "smi_tempos_open: null handle");
  SMI_REQUIRE(stream >= 0 && stream < h->s.max_streams, "smi_tempos_open: stream=%d outside 0..%d", stream, h->s.max_streams - 1);
  SMI_REQUIRE(p >= 1 && p <= 32767, "smi_tempos_open: p=%d outside 1..32767", p);
  SMI_REQUIRE(q >= 1 && q <= 32767, "smi_tempos_open: q=%d outside 1..32767", q);
  SMI_REQUIRE(p <= 4 * q && q <= 4 * p, "smi_tempos_open: p/q = %d/%d outside 1/4..4", p, q);
  TsStream& st = h->streams[(size_t)stream];
  st.open = 1; st.p = p; st.q = q; st.n = 0; st.f = 0;   // (st.set goes on alternating: a first push reads no state)
  return SMI_OK;
}

int smi_tempos_push_rows(smi_tempos* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride,
                         int32_t* n_out_host, void* stream) {
  SMI_REQUIRE(h && in_dev && stream_host && len_host && last_host && out_dev, "smi_tempos_push_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_tempos_push_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(stride >= 1, "smi_tempos_push_rows: stride=%lld must be positive", stride);
  const TsState& s = h->s;
  const int H = h->N / 2;
  TsArgs A;
  long long n_new[RS_MAX_ROWS], f_new[RS_MAX_ROWS], piece[RS_MAX_ROWS], need = 1, need_pos = 1;
  for (int b = 0; b < B; ++b) {
    const int id = stream_host[b];
    SMI_REQUIRE(id >= 0 && id < s.max_streams, "smi_tempos_push_rows: stream[%d]=%d outside 0..%d", b, id, s.max_streams - 1);
    for (int c = 0; c < b; ++c)
      SMI_REQUIRE(stream_host[c] != id, "smi_tempos_push_rows: stream[%d]=%d is row %d's stream too (one chunk of a stream a call)", b, id, c);
    const TsStream& st = h->streams[(size_t)id];
    SMI_REQUIRE(st.open, "smi_tempos_push_rows: stream[%d]=%d is not open (smi_tempos_open; a stream closes with its last chunk)", b, id);
    const int len = len_host[b], last = last_host[b];
    SMI_REQUIRE(last == 0 || last == 1, "smi_tempos_push_rows: last[%d]=%d is neither 0 nor 1", b, last);
    SMI_REQUIRE(len >= 0 && len <= h->max_chunk && len <= stride, "smi_tempos_push_rows: len[%d]=%d outside 0..min(max_chunk=%d, stride=%lld)", b,
                len, h->max_chunk, stride);
    SMI_REQUIRE(st.n + len <= TS_MAX_N, "smi_tempos_push_rows: stream[%d]=%d would reach %lld samples: 2^28 is the limit of a stream", b, id,
                st.n + len);
    piece[b] = smi_tempos_piece_len(st.p, st.q, h->N, h->D, st.n, st.f, len, last, &n_new[b], &f_new[b]);
    SMI_REQUIRE(piece[b] >= 0, "smi_tempos_push_rows: len[%d]=%d gives no valid piece", b, len);
    const bool copy = st.p == st.q;
    const long long h0_old = copy ? st.n : ts_hist_start(st.f, st.p, st.q, H, h->D);
    const long long h0_new = last ? -1 : copy ? n_new[b] : ts_hist_start(f_new[b], st.p, st.q, H, h->D);
    SMI_REQUIRE(f_new[b] - st.f <= s.fmax, "smi_tempos_push_rows: len[%d]=%d makes %lld frames final, the handle holds %d a push", b, len,
                f_new[b] - st.f, s.fmax);
    SMI_REQUIRE(last || (h0_new >= h0_old && n_new[b] - h0_new <= s.hcap),
                "smi_tempos_push_rows: stream[%d]=%d needs %lld samples of history, the handle keeps %d", b, id, n_new[b] - h0_new, s.hcap);
    TsRow& r = A.r[b];
    r.slot = id; r.set = st.set; r.len = len; r.p = st.p; r.q = st.q;
    r.n_old = (int32_t)st.n; r.n_new = (int32_t)n_new[b]; r.f_old = (int32_t)st.f; r.f_new = (int32_t)f_new[b];
    r.m_new = (int32_t)((copy ? st.n : st.f * H) + piece[b]);
    r.h0_old = (int32_t)h0_old; r.h0_new = (int32_t)h0_new;
    if (piece[b] > need) need = piece[b];
    if (f_new[b] - st.f > need_pos) need_pos = f_new[b] - st.f;
  }
  SMI_REQUIRE(out_stride >= need && out_stride <= TP_MAX_OUT, "smi_tempos_push_rows: out_stride=%lld outside %lld (the longest piece)..%d",
              out_stride, need, TP_MAX_OUT);
  SMI_REQUIRE(!pos_dev || (pos_stride >= need_pos && pos_stride <= TP_MAX_OUT),
              "smi_tempos_push_rows: pos_stride=%lld outside %lld (the most frames of a piece)..%d", pos_stride, need_pos, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + (size_t)B * stride * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_tempos_push_rows: out_dev overlaps in_dev");
  }
  for (int b = 0; b < B; ++b) {
    TsStream& st = h->streams[(size_t)stream_host[b]];
    if (n_out_host) n_out_host[b] = (int32_t)piece[b];
    st.n = n_new[b]; st.f = f_new[b]; st.set ^= 1;
    if (last_host[b]) st.open = 0;
  }
  hipStream_t hs = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tempos_search, dim3(B), dim3(TP_BLOCK), 0, hs, A, s, h->N, h->D, in_dev, stride, pos_dev, pos_stride);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + TP_TILE - 1) / TP_TILE);
  hipLaunchKernelGGL(k_tempos_ola, dim3(tiles, B), dim3(RS_BLOCK), 0, hs, A, s, h->N, in_dev, stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// ---- pitch shift of joined streams (smi_pitchs_*): the host arithmetic of include/sparkmi.h's "When an output is final"
struct PsPlan {
  int P, Q, up, down, half;
};

// the plan of a stream at tempo tp / tq and pitch ratio rp / rq with n_taps taps; false for a bad argument
static bool ps_plan(int tp, int tq, int rp, int rq, int N, int D, int n_taps, PsPlan& pl) {
  PtPlan bp;
  if (!pt_plan(0, tp, tq, rp, rq, N, bp) || !ts_args(bp.P, bp.Q, N, D)) return false;
  pl.P = bp.P; pl.Q = bp.Q; pl.up = bp.up; pl.down = bp.down; pl.half = n_taps / 2;
  if (bp.up == 1 && bp.down == 1) return n_taps == 0;
  return n_taps >= 3 && (n_taps & 1) && n_taps < (1 << 15) && pl.half >= pl.up;
}

// K: the final outputs of a stream that goes on and has emitted E stretched samples
static long long ps_final(long long E, const PsPlan& pl) {
  const long long a = E * pl.up - pl.half;
  return a <= 0 ? 0 : (a + pl.down - 1) / pl.down;
}

// the first stretched sample that output K and those behind it reach (rs_jlo on the host)
static long long ps_tail_start(long long K, const PsPlan& pl) {
  const long long a = K * pl.down - pl.half;
  return a <= 0 ? 0 : (a + pl.up - 1) / pl.up;
}

struct PsStream {
  int open = 0, set = 0, tp = 1, tq = 1, rp = 1, rq = 1, n_taps = 0;
  PsPlan pl = {1, 1, 1, 1, 0};
  long long n = 0, f = 0, k = 0;   // input samples so far, frames emitted, final outputs emitted
};
struct smi_pitchs {
  TsState s;
  PsState ps;
  int max_chunk, N, D, max_taps;
  DevBuf<char> pool;
  std::vector<PsStream> streams;
  std::vector<float> stage;   // [max_streams][tslot]: what open copies to the device, kept until the slot is opened again
};

extern "C" {

long long smi_pitchs_piece_len(int tp, int tq, int rp, int rq, int N, int D, int n_taps, long long n_before, long long frames_before,
                               long long k_before, long long len, int last, long long* n_after, long long* frames_after,
                               long long* k_after) {
  PsPlan pl;
  if (!ps_plan(tp, tq, rp, rq, N, D, n_taps, pl) || k_before < 0) return -1;
  long long n = 0, f = 0;
  if (smi_tempos_piece_len(pl.P, pl.Q, N, D, n_before, frames_before, len, last, &n, &f) < 0) return -1;
  long long E, K;
  if (last) {
    E = (n * pl.Q + pl.P - 1) / pl.P;   // M
    K = (n * tq + tp - 1) / tp;         // n_out
    if (rs_out_len(E, pl.up, pl.down) < K) return -1;
  } else {
    E = pl.P == pl.Q ? n : f * (N / 2);
    K = ps_final(E, pl);
  }
  if (K < k_before || E * pl.up >= (1LL << 31) || K * pl.down >= (1LL << 31)) return -1;
  if (n_after) *n_after = n;
  if (frames_after) *frames_after = f;
  if (k_after) *k_after = K;
  return K - k_before;
}

int smi_pitchs_create(int max_streams, int max_chunk, int N, int D, const double* win_host, int max_taps, smi_pitchs** out) {
  SMI_REQUIRE(out, "smi_pitchs_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_streams >= 1 && max_streams <= JN_MAX_STREAMS, "smi_pitchs_create: max_streams=%d outside 1..%d", max_streams, JN_MAX_STREAMS);
  SMI_REQUIRE(max_chunk >= 1 && max_chunk <= RS_MAX_SAMPLES, "smi_pitchs_create: max_chunk=%d outside 1..%d", max_chunk, RS_MAX_SAMPLES);
  SMI_REQUIRE(N >= 16 && N <= TP_MAX_N && !(N & 1), "smi_pitchs_create: N=%d must be even in 16..%d", N, TP_MAX_N);
  SMI_REQUIRE(D >= 0 && D <= TP_MAX_D, "smi_pitchs_create: D=%d outside 0..%d", D, TP_MAX_D);
  SMI_REQUIRE(win_host, "smi_pitchs_create: null win_host");
  SMI_REQUIRE(max_taps >= 0 && max_taps < RS_LDS_FLOATS, "smi_pitchs_create: max_taps=%d outside 0..%d", max_taps, RS_LDS_FLOATS - 1);
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_pitchs* h = new smi_pitchs();
  h->max_chunk = max_chunk; h->N = N; h->D = D; h->max_taps = max_taps;
  TsState& s = h->s;
  PsState& ps = h->ps;
  s.max_streams = max_streams;
  s.hcap = ts_hist_cap(N, D);
  s.fmax = (int)(4LL * ((long long)max_chunk + s.hcap) / (N / 2) + 4);   // frames one push can emit
  ps.tslot = 4 + ((max_taps + 3) & ~3);
  ps.tcap = max_taps + 1;   // E - rs_jlo(K down) <= 2 G / up < max_taps (include/sparkmi.h derives it)
  // one allocation: the window (float64), then the history sets, the tail sets and the slots' taps (fp32), the two sets of places
  // and the frames' work (int32)
  const size_t f64 = (size_t)N * sizeof(double);
  const size_t n_hist = 2 * (size_t)max_streams * s.hcap, n_tail = 2 * (size_t)max_streams * ps.tcap, n_taps = (size_t)max_streams * ps.tslot;
  const size_t n_pos = 2 * (size_t)max_streams, n_work = (size_t)RS_MAX_ROWS * (s.fmax + 1);
  const size_t bytes = f64 + (n_hist + n_tail + n_taps) * sizeof(float) + (n_pos + n_work) * sizeof(int32_t);
  if (h->pool.alloc(bytes, "smi_pitchs_create: stream state")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  s.win = (const double*)h->pool.get();
  s.hist = (float*)(h->pool + f64);
  ps.tail = s.hist + n_hist;
  ps.taps = ps.tail + n_tail;
  s.spos = (int32_t*)(ps.taps + n_taps);
  s.work = s.spos + n_pos;
  hipError_t e = hipMemset(h->pool, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->pool, win_host, f64, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    smi_set_error("smi_pitchs_create: upload of the window: %s", hipGetErrorString(e));
    delete h;
    return SMI_EHIP;
  }
  h->streams.assign((size_t)max_streams, PsStream{});
  h->stage.assign(n_taps, 0.f);
  *out = h;
  return SMI_OK;
}

int smi_pitchs_destroy(smi_pitchs* h) {
  delete h;
  return SMI_OK;
}

int smi_pitchs_open(smi_pitchs* h, int slot, int tp, int tq, int rp, int rq, const float* taps_host, int n_taps, void* stream) {
  SMI_REQUIRE(h, "smi_pitchs_open: null handle");
  SMI_REQUIRE(slot >= 0 && slot < h->s.max_streams, "smi_pitchs_open: slot=%d outside 0..%d", slot, h->s.max_streams - 1);
  SMI_REQUIRE(tp >= 1 && tp <= 32767, "smi_pitchs_open: tp=%d outside 1..32767", tp);
  SMI_REQUIRE(tq >= 1 && tq <= 32767, "smi_pitchs_open: tq=%d outside 1..32767", tq);
  SMI_REQUIRE(rp >= 1 && rp <= 32767, "smi_pitchs_open: rp=%d outside 1..32767", rp);
  SMI_REQUIRE(rq >= 1 && rq <= 32767, "smi_pitchs_open: rq=%d outside 1..32767", rq);
  PtPlan bp;
  SMI_REQUIRE(pt_plan(0, tp, tq, rp, rq, h->N, bp) && ts_args(bp.P, bp.Q, h->N, h->D),
              "smi_pitchs_open: the stretch (tp rq) / (tq rp) = (%d * %d) / (%d * %d) must lie in 1/4..4 with terms up to 32767", tp, rq, tq, rp);
  if (bp.up == 1 && bp.down == 1) {
    SMI_REQUIRE(n_taps == 0, "smi_pitchs_open: n_taps=%d must be 0 for a stream whose pitch ratio is 1/1", n_taps);
  } else {
    SMI_REQUIRE(n_taps >= 3 && (n_taps & 1), "smi_pitchs_open: n_taps=%d must be odd and at least 3 (taps h[0 .. 2G], G >= 1) at rp/rq = %d/%d",
                n_taps, rp, rq);
    SMI_REQUIRE(taps_host, "smi_pitchs_open: null taps_host");
    SMI_REQUIRE(n_taps <= h->max_taps, "smi_pitchs_open: n_taps=%d above the handle's max_taps=%d", n_taps, h->max_taps);
    SMI_REQUIRE(n_taps / 2 >= bp.up, "smi_pitchs_open: n_taps=%d gives G=%d below up=%d: the final outputs could pass the stream's length", n_taps,
                n_taps / 2, bp.up);
    const long long fl = (long long)n_taps + rs_window(bp.up, bp.down, n_taps / 2);
    SMI_REQUIRE(fl <= RS_LDS_FLOATS, "smi_pitchs_open: n_taps=%d with up/down = %d/%d needs %lld floats of LDS a tile, above %d", n_taps, bp.up,
                bp.down, fl, RS_LDS_FLOATS);
  }
  PsPlan pl;
  SMI_REQUIRE(ps_plan(tp, tq, rp, rq, h->N, h->D, n_taps, pl), "smi_pitchs_open: tp/tq = %d/%d, rp/rq = %d/%d, n_taps=%d give no plan", tp, tq, rp, rq,
              n_taps);
  float* st = h->stage.data() + (size_t)slot * h->ps.tslot;
  const int32_t head[4] = {pl.up, pl.down, pl.half, 0};
  memcpy(st, head, sizeof(head));
  if (n_taps) memcpy(st + 4, taps_host, (size_t)n_taps * sizeof(float));
  // behind the launches of the slot's earlier stream on this HIP stream, before this one's
  SMI_HIP(hipMemcpyAsync(h->ps.taps + (size_t)slot * h->ps.tslot, st, (size_t)(4 + n_taps) * sizeof(float), hipMemcpyHostToDevice,
                         (hipStream_t)stream));
  PsStream& ss = h->streams[(size_t)slot];
  ss.open = 1; ss.tp = tp; ss.tq = tq; ss.rp = rp; ss.rq = rq; ss.n_taps = n_taps; ss.pl = pl;
  ss.n = 0; ss.f = 0; ss.k = 0;   // (ss.set goes on alternating: a first push reads no state)
  return SMI_OK;
}

int smi_pitchs_push_rows(smi_pitchs* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, int32_t* pos_dev, long long pos_stride, float* out_dev, long long out_stride,
                         int32_t* n_out_host, void* stream) {
  SMI_REQUIRE(h && in_dev && stream_host && len_host && last_host && out_dev, "smi_pitchs_push_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_pitchs_push_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(stride >= 1, "smi_pitchs_push_rows: stride=%lld must be positive", stride);
  const TsState& s = h->s;
  const int H = h->N / 2;
  TsArgs A;
  PsArgs F;
  long long n_new[RS_MAX_ROWS], f_new[RS_MAX_ROWS], k_new[RS_MAX_ROWS], piece[RS_MAX_ROWS], need = 1, need_pos = 1;
  size_t lds = 0;
  for (int b = 0; b < B; ++b) {
    const int id = stream_host[b];
    SMI_REQUIRE(id >= 0 && id < s.max_streams, "smi_pitchs_push_rows: stream[%d]=%d outside 0..%d", b, id, s.max_streams - 1);
    for (int c = 0; c < b; ++c)
      SMI_REQUIRE(stream_host[c] != id, "smi_pitchs_push_rows: stream[%d]=%d is row %d's stream too (one chunk of a stream a call)", b, id, c);
    const PsStream& st = h->streams[(size_t)id];
    const PsPlan& pl = st.pl;
    SMI_REQUIRE(st.open, "smi_pitchs_push_rows: stream[%d]=%d is not open (smi_pitchs_open; a stream closes with its last chunk)", b, id);
    const int len = len_host[b], last = last_host[b];
    SMI_REQUIRE(last == 0 || last == 1, "smi_pitchs_push_rows: last[%d]=%d is neither 0 nor 1", b, last);
    SMI_REQUIRE(len >= 0 && len <= h->max_chunk && len <= stride, "smi_pitchs_push_rows: len[%d]=%d outside 0..min(max_chunk=%d, stride=%lld)", b,
                len, h->max_chunk, stride);
    SMI_REQUIRE(st.n + len <= TS_MAX_N, "smi_pitchs_push_rows: stream[%d]=%d would reach %lld samples: 2^28 is the limit of a stream", b, id,
                st.n + len);
    piece[b] = smi_pitchs_piece_len(st.tp, st.tq, st.rp, st.rq, h->N, h->D, st.n_taps, st.n, st.f, st.k, len, last, &n_new[b], &f_new[b], &k_new[b]);
    SMI_REQUIRE(piece[b] >= 0,
                "smi_pitchs_push_rows: len[%d]=%d gives no valid piece (E up or K down would reach 2^31, or the stretched stream resamples "
                "to fewer samples than the stream's length)", b, len);
    const bool copy = pl.P == pl.Q, plain = pl.up == 1 && pl.down == 1;
    const long long h0_old = copy ? st.n : ts_hist_start(st.f, pl.P, pl.Q, H, h->D);
    const long long h0_new = last ? -1 : copy ? n_new[b] : ts_hist_start(f_new[b], pl.P, pl.Q, H, h->D);
    const long long e_new = last ? (n_new[b] * pl.Q + pl.P - 1) / pl.P : copy ? n_new[b] : f_new[b] * H;
    SMI_REQUIRE(f_new[b] - st.f <= s.fmax, "smi_pitchs_push_rows: len[%d]=%d makes %lld frames final, the handle holds %d a push", b, len,
                f_new[b] - st.f, s.fmax);
    SMI_REQUIRE(last || (h0_new >= h0_old && n_new[b] - h0_new <= s.hcap),
                "smi_pitchs_push_rows: stream[%d]=%d needs %lld samples of history, the handle keeps %d", b, id, n_new[b] - h0_new, s.hcap);
    SMI_REQUIRE(last || plain || e_new - ps_tail_start(k_new[b], pl) <= h->ps.tcap,
                "smi_pitchs_push_rows: stream[%d]=%d needs %lld stretched samples of tail, the handle keeps %d", b, id,
                e_new - ps_tail_start(k_new[b], pl), h->ps.tcap);
    TsRow& r = A.r[b];
    r.slot = id; r.set = st.set; r.len = len; r.p = pl.P; r.q = pl.Q;
    r.n_old = (int32_t)st.n; r.n_new = (int32_t)n_new[b]; r.f_old = (int32_t)st.f; r.f_new = (int32_t)f_new[b];
    r.m_new = (int32_t)e_new;
    r.h0_old = (int32_t)h0_old; r.h0_new = (int32_t)h0_new;
    F.r[b].k_old = (int32_t)st.k; F.r[b].k_new = (int32_t)k_new[b];
    if (!plain) {
      const size_t fl = (size_t)st.n_taps + (size_t)rs_window(pl.up, pl.down, pl.half);   // <= RS_LDS_FLOATS: checked at open
      if (fl > lds) lds = fl;
    }
    if (piece[b] > need) need = piece[b];
    if (f_new[b] - st.f > need_pos) need_pos = f_new[b] - st.f;
  }
  SMI_REQUIRE(out_stride >= need && out_stride <= TP_MAX_OUT, "smi_pitchs_push_rows: out_stride=%lld outside %lld (the longest piece)..%d",
              out_stride, need, TP_MAX_OUT);
  SMI_REQUIRE(!pos_dev || (pos_stride >= need_pos && pos_stride <= TP_MAX_OUT),
              "smi_pitchs_push_rows: pos_stride=%lld outside %lld (the most frames of a piece)..%d", pos_stride, need_pos, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + (size_t)B * stride * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_pitchs_push_rows: out_dev overlaps in_dev");
    const char* p0 = h->pool.get();
    const char* p1 = p0 + h->pool.bytes();
    SMI_REQUIRE(p1 <= o0 || o1 <= p0, "smi_pitchs_push_rows: out_dev overlaps the handle's state");
  }
  for (int b = 0; b < B; ++b) {
    PsStream& st = h->streams[(size_t)stream_host[b]];
    if (n_out_host) n_out_host[b] = (int32_t)piece[b];
    st.n = n_new[b]; st.f = f_new[b]; st.k = k_new[b]; st.set ^= 1;
    if (last_host[b]) st.open = 0;
  }
  hipStream_t hs = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tempos_search, dim3(B), dim3(TP_BLOCK), 0, hs, A, s, h->N, h->D, in_dev, stride, pos_dev, pos_stride);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + RS_TILE - 1) / RS_TILE);
  hipLaunchKernelGGL(k_pitchs_ola, dim3(tiles, B), dim3(RS_BLOCK), lds * sizeof(float), hs, A, F, s, h->ps, h->N, in_dev, stride, out_dev,
                     out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// ---- loudness of joined streams (smi_louds_*): the host arithmetic of include/sparkmi.h's "Emission"
#define LS_MAX_N (1LL << 28)   // input samples of one stream, as for smi_tempos

struct LsStream {
  int open = 0, set = 0;
  long long n = 0;          // input samples so far: the knots made and the samples emitted follow from it (ls_plan)
  LsParam q = {0.0, 0.0, 1.0, 1.0, 1.0};
};
struct smi_louds {
  LsState s;
  int max_chunk;
  double abs_gate;
  DevBuf<char> pool;
  std::vector<LsStream> streams;
};

static bool ls_block_ok(int block) { return block >= 4 && block <= RS_MAX_SAMPLES && !(block & 3); }

extern "C" {

long long smi_louds_piece_len(int block, long long n_before, long long len, int last, long long* n_after, long long* knots_after) {
  if (!ls_block_ok(block) || n_before < 0 || len < 0 || n_before > LS_MAX_N || len > LS_MAX_N || n_before + len > LS_MAX_N) return -1;
  if (last != 0 && last != 1) return -1;
  const LsPlan p = ls_plan((int)n_before, (int)len, last, block / 4);
  if (n_after) *n_after = p.n_new;
  if (knots_after) *knots_after = p.k_new;
  return p.e_new - p.e_old;
}

int smi_louds_create(int max_streams, int max_chunk, int block, const double* coef_host, int max_blocks, smi_louds** out) {
  SMI_REQUIRE(out, "smi_louds_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_streams >= 1 && max_streams <= JN_MAX_STREAMS, "smi_louds_create: max_streams=%d outside 1..%d", max_streams, JN_MAX_STREAMS);
  SMI_REQUIRE(max_chunk >= 1 && max_chunk <= RS_MAX_SAMPLES, "smi_louds_create: max_chunk=%d outside 1..%d", max_chunk, RS_MAX_SAMPLES);
  SMI_REQUIRE(ls_block_ok(block), "smi_louds_create: block=%d must be a multiple of 4 in 4..%d", block, RS_MAX_SAMPLES);
  SMI_REQUIRE(max_blocks >= 1 && max_blocks <= (1 << 26), "smi_louds_create: max_blocks=%d outside 1..2^26", max_blocks);
  SMI_REQUIRE(coef_host, "smi_louds_create: null coef_host");
  for (int i = 0; i < 10; ++i)
    SMI_REQUIRE(std::isfinite(coef_host[i]), "smi_louds_create: coef[%d]=%g is not finite", i, coef_host[i]);
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_louds* h = new smi_louds();
  h->max_chunk = max_chunk;
  h->abs_gate = pow(10.0, (-70.0 + 0.691) / 10.0);
  LsState& s = h->s;
  for (int st = 0; st < 2; ++st) {
    for (int i = 0; i < 3; ++i) s.c.b[st][i] = coef_host[5 * st + i];
    s.c.a1[st] = coef_host[5 * st + 3];
    s.c.a2[st] = coef_host[5 * st + 4];
  }
  ld_transition(s.c);
  const int hop = block / 4;
  s.max_streams = max_streams; s.max_blocks = max_blocks; s.block = block;
  s.hcap = (5 * hop > LD_SEG ? 5 * hop : LD_SEG) + 2;   // n - min(E(n), the last segment edge) + the two samples before it
  s.pps = (LD_SEG - 1) / hop + 2;
  // a row's scratch: a push filters the tail short of a segment it held and its chunk
  const long long nseg = (long long)max_chunk / LD_SEG + 3, nhop = ((long long)max_chunk + LD_SEG) / hop + 8, nknot = (long long)max_chunk / hop + 10;
  s.w_s = 4 * nseg;
  s.w_parts = s.w_s + 4 * (nseg + 1);
  s.w_hops = s.w_parts + nseg * s.pps;
  s.w_gain = s.w_hops + nhop;
  s.wrow = s.w_gain + nknot;
  // one allocation: float64 first (states, blocks, scratch), then the two history sets (fp32)
  const size_t n_st = 2 * (size_t)max_streams * LS_STATE, n_z = (size_t)max_streams * max_blocks, n_work = (size_t)RS_MAX_ROWS * s.wrow;
  const size_t n_hist = 2 * (size_t)max_streams * s.hcap;
  const size_t bytes = (n_st + n_z + n_work) * sizeof(double) + n_hist * sizeof(float);
  if (h->pool.alloc(bytes, "smi_louds_create: stream state")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  s.st = (double*)h->pool.get();
  s.z = s.st + n_st;
  s.work = s.z + n_z;
  s.hist = (float*)(s.work + n_work);
  const hipError_t e = hipMemset(h->pool, 0, bytes);
  if (e != hipSuccess) {
    smi_set_error("smi_louds_create: clearing the state: %s", hipGetErrorString(e));
    delete h;
    return SMI_EHIP;
  }
  h->streams.assign((size_t)max_streams, LsStream{});
  *out = h;
  return SMI_OK;
}

int smi_louds_destroy(smi_louds* h) {
  delete h;
  return SMI_OK;
}

int smi_louds_open(smi_louds* h, int stream, double target, double max_gain_db, double ceiling, double max_slew_db) {
  SMI_REQUIRE(h, "smi_louds_open: null handle");
  SMI_REQUIRE(stream >= 0 && stream < h->s.max_streams, "smi_louds_open: stream=%d outside 0..%d", stream, h->s.max_streams - 1);
  SMI_REQUIRE(!std::isinf(target), "smi_louds_open: target=%g must be finite, or NaN to measure only", target);
  SMI_REQUIRE(std::isfinite(max_gain_db) && max_gain_db >= 0.0, "smi_louds_open: max_gain_db=%g must be finite and >= 0", max_gain_db);
  SMI_REQUIRE(std::isfinite(ceiling) && ceiling > 0.0, "smi_louds_open: ceiling=%g must be finite and > 0", ceiling);
  SMI_REQUIRE(std::isfinite(max_slew_db) && max_slew_db >= 0.0 && max_slew_db <= 200.0, "smi_louds_open: max_slew_db=%g outside 0..200", max_slew_db);
  LsStream& st = h->streams[(size_t)stream];
  st.open = 1; st.n = 0;   // (st.set goes on alternating: a first push reads no state)
  st.q.target = target; st.q.max_gain_db = max_gain_db; st.q.ceiling = ceiling;
  st.q.s_up = pow(10.0, max_slew_db / 20.0);
  st.q.s_dn = 1.0 / st.q.s_up;
  return SMI_OK;
}

int smi_louds_push_rows(smi_louds* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                        const int32_t* last_host, int B, double* gain_dev, long long gain_stride, float* out_dev, long long out_stride,
                        int32_t* n_out_host, double* stats_dev, void* stream) {
  SMI_REQUIRE(h && in_dev && stream_host && len_host && last_host && out_dev, "smi_louds_push_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_louds_push_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(stride >= 1, "smi_louds_push_rows: stride=%lld must be positive", stride);
  const LsState& s = h->s;
  const int hop = s.block / 4;
  LsArgs A;
  LsParams Q;
  LsPlan plan[RS_MAX_ROWS];
  long long need = 1, need_gain = 1;
  int nseg_max = 1;
  for (int b = 0; b < B; ++b) {
    const int id = stream_host[b];
    SMI_REQUIRE(id >= 0 && id < s.max_streams, "smi_louds_push_rows: stream[%d]=%d outside 0..%d", b, id, s.max_streams - 1);
    for (int c = 0; c < b; ++c)
      SMI_REQUIRE(stream_host[c] != id, "smi_louds_push_rows: stream[%d]=%d is row %d's stream too (one chunk of a stream a call)", b, id, c);
    const LsStream& st = h->streams[(size_t)id];
    SMI_REQUIRE(st.open, "smi_louds_push_rows: stream[%d]=%d is not open (smi_louds_open; a stream closes with its last chunk)", b, id);
    const int len = len_host[b], last = last_host[b];
    SMI_REQUIRE(last == 0 || last == 1, "smi_louds_push_rows: last[%d]=%d is neither 0 nor 1", b, last);
    SMI_REQUIRE(len >= 0 && len <= h->max_chunk && len <= stride, "smi_louds_push_rows: len[%d]=%d outside 0..min(max_chunk=%d, stride=%lld)", b,
                len, h->max_chunk, stride);
    SMI_REQUIRE(st.n + len <= LS_MAX_N, "smi_louds_push_rows: stream[%d]=%d would reach %lld samples: 2^28 is the limit of a stream", b, id,
                st.n + len);
    const LsPlan p = plan[b] = ls_plan((int)st.n, len, last, hop);
    SMI_REQUIRE(p.z_new <= s.max_blocks, "smi_louds_push_rows: stream[%d]=%d would reach %d blocks, the handle holds max_blocks=%d", b, id,
                p.z_new, s.max_blocks);
    SMI_REQUIRE(p.h0_new >= p.h0_old && p.n_new - p.h0_new <= s.hcap, "smi_louds_push_rows: stream[%d]=%d needs %d samples of history, the handle keeps %d",
                b, id, p.n_new - p.h0_new, s.hcap);
    LsRow& r = A.r[b];
    r.slot = id; r.set = st.set; r.n_old = (int32_t)st.n; r.len = len | (last << 30);
    Q.r[b] = st.q;
    if (p.e_new - p.e_old > need) need = p.e_new - p.e_old;
    if (2LL * (p.k_new - p.k_old) > need_gain) need_gain = 2LL * (p.k_new - p.k_old);
    if (p.nseg > nseg_max) nseg_max = p.nseg;
  }
  SMI_REQUIRE(out_stride >= need && out_stride <= TP_MAX_OUT, "smi_louds_push_rows: out_stride=%lld outside %lld (the longest piece)..%d",
              out_stride, need, TP_MAX_OUT);
  SMI_REQUIRE(!gain_dev || (gain_stride >= need_gain && gain_stride <= TP_MAX_OUT),
              "smi_louds_push_rows: gain_stride=%lld outside %lld (two values a knot of the row with the most)..%d", gain_stride, need_gain, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + (size_t)B * stride * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_louds_push_rows: out_dev overlaps in_dev");
  }
  for (int b = 0; b < B; ++b) {
    LsStream& st = h->streams[(size_t)stream_host[b]];
    if (n_out_host) n_out_host[b] = plan[b].e_new - plan[b].e_old;
    st.n = plan[b].n_new; st.set ^= 1;
    if (last_host[b]) st.open = 0;
  }
  hipStream_t hs = (hipStream_t)stream;
  const int tiles = (nseg_max + LD_LANES - 1) / LD_LANES;
  const size_t lds = (size_t)LD_LANES * LD_PITCH * sizeof(float);
  hipLaunchKernelGGL(k_louds_seg, dim3(tiles, B), dim3(LD_LANES), lds, hs, A, s, in_dev, stride);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_louds_carry, dim3(B), dim3(64), 0, hs, A, s);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_louds_energy, dim3(tiles, B), dim3(LD_LANES), lds, hs, A, s, in_dev, stride);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_louds_knots, dim3(B), dim3(LD_GATE), 0, hs, A, Q, s, h->abs_gate, in_dev, stride, gain_dev, gain_stride, stats_dev);
  SMI_LAUNCH_CHECK();
  const int gtiles = (int)((out_stride + GN_TILE - 1) / GN_TILE);
  hipLaunchKernelGGL(k_louds_apply, dim3(gtiles, B), dim3(RS_BLOCK), 0, hs, A, s, in_dev, stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"

// ---- limiter of joined streams (smi_limits_*): the host arithmetic of include/sparkmi.h's "Emission"
#define LT_MAX_N (1LL << 28)   // input samples of one stream, as for smi_tempos and smi_louds

struct LtStream {
  int open = 0, set = 0, tp = 0;
  long long n = 0;          // input samples so far: the samples emitted and the history held follow from it (lt_plan)
  double ceiling = 1.0;
};
struct smi_limits {
  LtState s;
  int max_chunk, n_taps, rows;
  DevBuf<char> pool;
  std::vector<LtStream> streams;
};

extern "C" {

long long smi_limits_piece_len(int lookahead, int release, long long n_before, long long len, int last, long long* n_after) {
  if (lookahead < 0 || lookahead > LM_MAX_A || release < 0 || release > LM_MAX_R) return -1;
  if (n_before < 0 || len < 0 || n_before > LT_MAX_N || len > LT_MAX_N || n_before + len > LT_MAX_N) return -1;
  if (last != 0 && last != 1) return -1;
  const LtPlan p = lt_plan((int)n_before, (int)len, last, lookahead + release);
  if (n_after) *n_after = p.n_new;
  return p.e_new - p.e_old;
}

int smi_limits_create(int max_streams, int max_chunk, int lookahead, int release, const double* win_host, const double* taps_host, int n_taps,
                      int phases, smi_limits** out) {
  SMI_REQUIRE(out, "smi_limits_create: null out");
  *out = nullptr;
  SMI_REQUIRE(max_streams >= 1 && max_streams <= JN_MAX_STREAMS, "smi_limits_create: max_streams=%d outside 1..%d", max_streams, JN_MAX_STREAMS);
  SMI_REQUIRE(max_chunk >= 1 && max_chunk <= RS_MAX_SAMPLES, "smi_limits_create: max_chunk=%d outside 1..%d", max_chunk, RS_MAX_SAMPLES);
  SMI_REQUIRE(phases >= 1 && phases <= LM_MAX_PHASES, "smi_limits_create: phases=%d outside 1..%d", phases, LM_MAX_PHASES);
  SMI_REQUIRE(n_taps == 0 || n_taps == 2 * LM_HALO * phases + 1,
              "smi_limits_create: n_taps=%d is neither 0 (the sample peak alone) nor %d = 2 * 10 * phases + 1 for phases=%d", n_taps,
              2 * LM_HALO * phases + 1, phases);
  SMI_REQUIRE(n_taps == 0 || taps_host, "smi_limits_create: null taps_host with n_taps=%d", n_taps);
  for (int i = 0; i < n_taps; ++i) SMI_REQUIRE(std::isfinite(taps_host[i]), "smi_limits_create: taps[%d]=%g is not finite", i, taps_host[i]);
  SMI_REQUIRE(lookahead >= 0 && lookahead <= LM_MAX_A, "smi_limits_create: lookahead=%d outside 0..%d", lookahead, LM_MAX_A);
  SMI_REQUIRE(release >= 0 && release <= LM_MAX_R, "smi_limits_create: release=%d outside 0..%d", release, LM_MAX_R);
  SMI_REQUIRE(win_host, "smi_limits_create: null win_host");
  const int W = lookahead + release, nw = W + 1;
  double wsum = 0.0;
  for (int i = 0; i < nw; ++i) {
    SMI_REQUIRE(std::isfinite(win_host[i]) && win_host[i] >= 0.0, "smi_limits_create: win[%d]=%g must be finite and >= 0", i, win_host[i]);
    wsum = wsum + win_host[i];
  }
  SMI_REQUIRE(std::fabs(wsum - 1.0) <= 1e-12, "smi_limits_create: win sums to 1%+.3g over its %d weights, not to 1 within 1e-12", wsum - 1.0, nw);
  char arch[128];
  const int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_limits* h = new smi_limits();
  h->max_chunk = max_chunk; h->n_taps = n_taps;
  h->rows = max_streams < RS_MAX_ROWS ? max_streams : RS_MAX_ROWS;   // a call holds a stream once, so never more rows than slots
  LtState& s = h->s;
  s.max_streams = max_streams; s.A = lookahead; s.R = release; s.phases = phases;
  s.hcap = 2 * W + 2 * LM_HALO - 1;   // n - max(0, E(n) - W - 9) with E(n) = n - (W + 10)
  // a row's scratch: the longest piece is max_chunk + W + 10 samples (a last push onto W + 10 held ones) and reads r over W more on
  // either side; then a max e a tile of those, and a min s and a count a tile of the piece
  const long long rcap = ((long long)max_chunk + 3LL * W + LM_HALO + 7) / 8 * 8, tiles = rcap / LM_TILE + 1;
  s.w_emax = rcap;
  s.w_smin = s.w_emax + tiles;
  s.w_cnt = s.w_smin + tiles;
  s.wrow = (s.w_cnt + tiles + 7) / 8 * 8;
  // one allocation: float64 first (window, taps, states, scratch), then the two history sets (fp32)
  const size_t n_win = ((size_t)nw + 7) / 8 * 8, n_taps8 = ((size_t)LM_MAX_TAPS + 7) / 8 * 8, n_st = 2 * (size_t)max_streams * LT_STATE;
  const size_t n_work = (size_t)h->rows * s.wrow, n_hist = 2 * (size_t)max_streams * s.hcap;
  const size_t bytes = (n_win + n_taps8 + n_st + n_work) * sizeof(double) + n_hist * sizeof(float);
  if (h->pool.alloc(bytes, "smi_limits_create: stream state")) {
    (void)hipGetLastError();
    delete h;
    return SMI_ENOMEM;
  }
  double* base = (double*)h->pool.get();
  s.win = base;
  s.taps = base + n_win;
  s.st = base + n_win + n_taps8;
  s.work = s.st + n_st;
  s.hist = (float*)(s.work + n_work);
  hipError_t e = hipMemset(h->pool, 0, bytes);
  if (e == hipSuccess) e = hipMemcpy(base, win_host, (size_t)nw * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && n_taps) e = hipMemcpy(base + n_win, taps_host, (size_t)n_taps * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    smi_set_error("smi_limits_create: upload of the window and the taps: %s", hipGetErrorString(e));
    delete h;
    return SMI_EHIP;
  }
  h->streams.assign((size_t)max_streams, LtStream{});
  *out = h;
  return SMI_OK;
}

int smi_limits_destroy(smi_limits* h) {
  delete h;
  return SMI_OK;
}

int smi_limits_open(smi_limits* h, int stream, int true_peak, double ceiling) {
  SMI_REQUIRE(h, "smi_limits_open: null handle");
  SMI_REQUIRE(stream >= 0 && stream < h->s.max_streams, "smi_limits_open: stream=%d outside 0..%d", stream, h->s.max_streams - 1);
  SMI_REQUIRE(true_peak == 0 || true_peak == 1, "smi_limits_open: true_peak=%d is neither 0 nor 1", true_peak);
  SMI_REQUIRE(!true_peak || h->n_taps, "smi_limits_open: true_peak=1 on a handle created with n_taps=0 (the sample peak alone)");
  SMI_REQUIRE(std::isfinite(ceiling) && ceiling > 0.0, "smi_limits_open: ceiling=%g must be finite and > 0", ceiling);
  LtStream& st = h->streams[(size_t)stream];
  st.open = 1; st.n = 0; st.tp = true_peak; st.ceiling = ceiling;   // (st.set goes on alternating: a first push reads no state)
  return SMI_OK;
}

int smi_limits_push_rows(smi_limits* h, const float* in_dev, long long stride, const int32_t* stream_host, const int32_t* len_host,
                         const int32_t* last_host, int B, float* out_dev, long long out_stride, int32_t* n_out_host, double* stats_dev,
                         void* stream) {
  SMI_REQUIRE(h && in_dev && stream_host && len_host && last_host && out_dev, "smi_limits_push_rows: null argument");
  SMI_REQUIRE(B >= 1 && B <= RS_MAX_ROWS, "smi_limits_push_rows: B=%d outside 1..%d", B, RS_MAX_ROWS);
  SMI_REQUIRE(stride >= 1, "smi_limits_push_rows: stride=%lld must be positive", stride);
  const LtState& s = h->s;
  const int W = s.A + s.R;
  LtArgs A;
  LtPlan plan[RS_MAX_ROWS];
  long long need = 1;
  int r_max = 1;
  for (int b = 0; b < B; ++b) {
    const int id = stream_host[b];
    SMI_REQUIRE(id >= 0 && id < s.max_streams, "smi_limits_push_rows: stream[%d]=%d outside 0..%d", b, id, s.max_streams - 1);
    for (int c = 0; c < b; ++c)
      SMI_REQUIRE(stream_host[c] != id, "smi_limits_push_rows: stream[%d]=%d is row %d's stream too (one chunk of a stream a call)", b, id, c);
    const LtStream& st = h->streams[(size_t)id];
    SMI_REQUIRE(st.open, "smi_limits_push_rows: stream[%d]=%d is not open (smi_limits_open; a stream closes with its last chunk)", b, id);
    const int len = len_host[b], last = last_host[b];
    SMI_REQUIRE(last == 0 || last == 1, "smi_limits_push_rows: last[%d]=%d is neither 0 nor 1", b, last);
    SMI_REQUIRE(len >= 0 && len <= h->max_chunk && len <= stride, "smi_limits_push_rows: len[%d]=%d outside 0..min(max_chunk=%d, stride=%lld)", b,
                len, h->max_chunk, stride);
    SMI_REQUIRE(st.n + len <= LT_MAX_N, "smi_limits_push_rows: stream[%d]=%d would reach %lld samples: 2^28 is the limit of a stream", b, id,
                st.n + len);
    const LtPlan p = plan[b] = lt_plan((int)st.n, len, last, W);
    SMI_REQUIRE(last || (p.h0_new >= p.h0_old && p.n_new - p.h0_new <= s.hcap),
                "smi_limits_push_rows: stream[%d]=%d needs %d samples of history, the handle keeps %d", b, id, p.n_new - p.h0_new, s.hcap);
    SMI_REQUIRE(p.r_hi - p.r_lo <= s.w_emax, "smi_limits_push_rows: stream[%d]=%d needs %d values of scratch, the handle keeps %lld", b, id,
                p.r_hi - p.r_lo, s.w_emax);
    LtRow& r = A.r[b];
    r.slot = id; r.set = st.set; r.n_old = (int32_t)st.n; r.len = len | (last << 30);
    r.tp = st.tp; r.ceiling = st.ceiling;
    r.c32 = (float)st.ceiling;   // the largest float32 <= ceiling
    if ((double)r.c32 > st.ceiling) r.c32 = nextafterf(r.c32, 0.f);
    if (p.e_new - p.e_old > need) need = p.e_new - p.e_old;
    if (p.r_hi - p.r_lo > r_max) r_max = p.r_hi - p.r_lo;
  }
  SMI_REQUIRE(out_stride >= need && out_stride <= TP_MAX_OUT, "smi_limits_push_rows: out_stride=%lld outside %lld (the longest piece)..%d",
              out_stride, need, TP_MAX_OUT);
  {
    const char* i0 = (const char*)in_dev;
    const char* i1 = i0 + (size_t)B * stride * sizeof(float);
    const char* o0 = (const char*)out_dev;
    const char* o1 = o0 + (size_t)B * out_stride * sizeof(float);
    SMI_REQUIRE(i1 <= o0 || o1 <= i0, "smi_limits_push_rows: out_dev overlaps in_dev");
  }
  for (int b = 0; b < B; ++b) {
    LtStream& st = h->streams[(size_t)stream_host[b]];
    if (n_out_host) n_out_host[b] = plan[b].e_new - plan[b].e_old;
    st.n = plan[b].n_new; st.set ^= 1;
    if (last_host[b]) st.open = 0;
  }
  hipStream_t hs = (hipStream_t)stream;
  const int etiles = (r_max + LM_TILE - 1) / LM_TILE;
  hipLaunchKernelGGL(k_limits_env, dim3(etiles, B), dim3(RS_BLOCK), 0, hs, A, s, in_dev, stride);
  SMI_LAUNCH_CHECK();
  const int tiles = (int)((out_stride + LM_TILE - 1) / LM_TILE);
  const size_t lds = (size_t)(LM_TILE + 2 * W) * sizeof(double);
  hipLaunchKernelGGL(k_limits_apply, dim3(tiles, B), dim3(RS_BLOCK), lds, hs, A, s, in_dev, stride, out_dev, out_stride);
  SMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_limits_stats, dim3(B), dim3(RS_BLOCK), 0, hs, A, s, stats_dev);
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

}  // extern "C"
