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
#include <vector>

#include "smi_common.h"

#define RS_MAX_ROWS 64          // rows of one call: their descriptors travel as kernel arguments
#define RS_TILE 1024            // output samples a block
#define RS_BLOCK 256
#define RS_LDS_FLOATS 16384     // taps + input window of one tile: 64 KiB of LDS
#define RS_POOL_FLOATS (1 << 18)
#define RS_MAX_SAMPLES (1 << 24)
#define PR_BLOCK 1024
#define PR_BINS 2048

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
  for (int i = tid; i < RS_TILE && k0 + i < out_stride; i += RS_BLOCK) {
    const long long k = k0 + i;
    float acc = 0.f;
    if (k < r.n_out) {
      const int kd = (int)k * r.down;
      const int jl = rs_jlo(kd, r.up, r.half);
      const int jh = min(rs_jhi(kd, r.up, r.half), r.n_in - 1);
      int t = r.half + kd - jl * r.up;   // tap of the first term, in [0, 2H]
      const int w = jl - j0;
      const int n = jh - jl + 1;
      for (int m = 0; m < n; ++m, t -= r.up) acc = acc + xw[w + m] * ht[t];
    }
    y[k] = acc;
  }
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

}  // namespace

struct smi_rs {
  int max_rows, max_in, max_out;
  float* pool;
  int pool_used;
  std::vector<Filter> filters;
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
  h->pool = nullptr; h->pool_used = 0;
  if (hipMalloc((void**)&h->pool, (size_t)RS_POOL_FLOATS * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    delete h;
    smi_set_error("smi_rs_create: device allocation of the tap pool failed");
    return SMI_ENOMEM;
  }
  *out = h;
  return SMI_OK;
}

int smi_rs_destroy(smi_rs* h) {
  if (!h) return SMI_OK;
  if (h->pool) (void)hipFree(h->pool);
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

}  // extern "C"
