// smi_net.hip -- the kernels and launch builders shared by the BiCodec vocoder (smi_voc.hip) and the prompt encoder
// (smi_enc.hip): the implicit-GEMM conv / linear kernel on the exact-fp32 matrix pipe and on the bf16-split pipe, the fused
// ResidualUnit, depthwise-conv + LayerNorm, the per-utterance GEMV, codebook / FSQ lookups, the table of their instantiations
// and the builders that turn a layer into a launch.  The clients see smi_net.h; every launch of these kernels is in this file.
#include "smi_net.h"
#include <type_traits>

namespace smi_net __attribute__((visibility("hidden"))) {
namespace {

// fast: the hardware sine (v_sin_f32 on x / 2 pi, ~1e-6 absolute) -- the layers of the bf16-split pipe, whose products already
// carry 2^-17 relative error; the library sine costs ~2500 of the ~4000 vector instructions a thread of a conv block issues
// (32 Snake values per thread), which is what bounded the one-tap layers and a third of the 7-tap ones.
__device__ __forceinline__ float snake_f(float x, float a, bool fast) {
  const float s = fast ? __sinf(a * x) : sinf(a * x);
  return x + (1.0f / (a + 1e-9f)) * (s * s);
}

// Shared tail of the conv kernels: (KS) fixed-order reduction of the four waves' partial tiles through LDS, then bias,
// per-utterance bias, activation, layer scale, residual, tanh, the 3x of SamplingBlock(ratio 1), and the two outputs
// (raw and Snake'd).  acc follows the 32x32 MFMA D layout: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5),
// column l & 31.
template <int QB, bool KS>
__device__ __forceinline__ void conv_finish(const ConvP& p, f32x16 (&acc)[QB], float* lds, int ct, bool live, int b, int phase,
                                            int q0, int olen, int lane, int wave) {
  if (KS) {
    // fixed-order reduction of the four waves' partial tiles, then each wave finishes 4 of the 16 rows-groups
    __syncthreads();
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int r = 0; r < 16; ++r) lds[((wave * QB + qb) * 16 + r) * 64 + lane] = acc[qb][r];
    __syncthreads();
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        float s = lds[((0 * QB + qb) * 16 + r) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += lds[((w * QB + qb) * 16 + r) * 64 + lane];
        acc[qb][rr] = s;
      }
  }
  if (!live) return;

  // Epilogue loads first, arithmetic second.  Written element by element (`if (p.bias) y += p.bias[co]; ... if (p.R) y = p.R[o] + y;`)
  // hipcc branches around every load and waits for it on the spot: up to six dependent round trips per element, ~190
  // `s_waitcnt vmcnt(0)` per block -- the one-tap layers then ran at 1.3 TB/s of traffic with blocks alive for ~50 us.  Here
  // every load of eight output rows is unconditional (an absent operand reads a valid dummy address and is dropped by a
  // select), so they are all in flight together; the arithmetic and its order are unchanged.
  const long long yboff = (long long)b * p.yb;
  constexpr int NREG = KS ? 4 : 16, GRP = KS ? 4 : 8;
  const bool hb = p.bias != nullptr, hbb = p.bbias != nullptr, hg = p.gamma != nullptr, hbe = p.beta != nullptr, hr = p.R != nullptr,
             hs = p.Ys != nullptr;
  const bool fsin = p.fast_sin != 0;
  const float* dummy = p.X;                       // any readable floats: index < Cout <= the first activation row's size
  const float* pb = hb ? p.bias : dummy;
  const float* pbb = hbb ? p.bbias + (long long)b * p.Cout : dummy;
  const float* pg = hg ? p.gamma : dummy;
  const float* pbe = hbe ? p.beta : dummy;
  const float* pa = hs ? p.alpha : dummy;
  bool qok[QB];
  int tq[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + qb * 32 + (lane & 31);
    qok[qb] = q < olen;
    tq[qb] = (qok[qb] ? q : olen - 1) * p.S + phase;   // (q0 < olen: the block has at least one live column)
  }
#pragma unroll
  for (int r0 = 0; r0 < NREG; r0 += GRP) {
    int co[GRP];
    bool cok[GRP];
    float bv[GRP], bbv[GRP], gv[GRP], bev[GRP], av[GRP], rv[QB][GRP];
#pragma unroll
    for (int i = 0; i < GRP; ++i) {
      const int r = KS ? wave * 4 + r0 + i : r0 + i;
      co[i] = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      cok[i] = co[i] < p.Cout;
      const int cc = cok[i] ? co[i] : p.Cout - 1;
      bv[i] = pb[cc]; bbv[i] = pbb[cc]; gv[i] = pg[cc]; bev[i] = pbe[cc]; av[i] = pa[cc];
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const float* rp = hr ? p.R + (yboff + (long long)cc * p.ystride + tq[qb]) : dummy;
        rv[qb][i] = *rp;
      }
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
      for (int i = 0; i < GRP; ++i) {
        float y = acc[qb][r0 + i];
        y = hb ? y + bv[i] : y;
        y = hbb ? y + bbv[i] : y;
        if (p.act == ACT_GELU) y = gelu_f(y);
        if (p.act == ACT_RELU) y = fmaxf(y, 0.f);
        y = hg ? gv[i] * y : y;
        y = hbe ? y + bev[i] : y;
        y = hr ? rv[qb][i] + y : y;
        if (p.act == ACT_TANH) y = tanhf(y);
        if (p.out_scale != 1.0f) y = (y + y) + y;  // SamplingBlock(ratio 1): x + x + x
        if (qok[qb] && cok[i]) {
          const long long o = yboff + (long long)co[i] * p.ystride + tq[qb];
          if (p.Y) p.Y[o] = y;
          if (hs) p.Ys[o] = snake_f(y, av[i], fsin);
        }
      }
    }
  }
}

// QB: 32-wide time sub-tiles per wave.  KS: waves split the input channels of ONE 32-row output
// tile (large C, short T) instead of owning a 32-row output tile each.  CHG: a staged chunk holds
// 32*CHG input channels (1-tap layers use 128 so a chunk carries enough MFMAs per barrier).  NC:
// the staged row (tile * input stride + halo) is up to 64 * NC columns wide.  NWV: waves per block (3 when the number of
// 32-row output tiles is a multiple of 3 but not of 4 -- C = 96, 192: with four waves a quarter of every block, and so one
// SIMD of every CU, would idle).
template <int QB, bool KS, int CHG, int NC, bool WPF = false, int NWV = 4>
__global__ __launch_bounds__(256) void k_conv(ConvP p) {
  static_assert(NWV == 4 || !KS, "the channel-split mode reduces over four waves");
  constexpr int kCh = 8 * NWV * CHG;   // channels per staged chunk: eight rows per wave and CHG
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int QT = QB * 32;
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int b = bz / p.S, phase = bz - b * p.S;
  const int q0 = bx * QT;
  const int len = p.lens[b];
  const int olen = p.olens ? p.olens[b] : len;
  if (q0 >= olen) return;
  const int ct = KS ? by : by * NWV + wave;
  const bool live = ct * 32 < p.Cout;
  const int ntap = p.ntaps[phase];
  const int groups = p.CinP >> 3;
  const float* Xb = p.X + (long long)b * p.xb;
  const float4* Wp = (const float4*)(p.W + p.wphase[phase]) + (long long)ct * ntap * groups * 64;

  f32x16 acc[QB];
#pragma unroll
  for (int i = 0; i < QB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int xw = p.xw;
  // Staging: wave w owns rows 8w..8w+7 of the 32-channel chunk, lanes run along time (coalesced rows).
  // The next chunk's rows are requested before the MFMAs of the current one and written to LDS after
  // them, so global latency hides behind the matrix pipe.  With KS each wave multiplies exactly the
  // rows it staged, so only the wave itself has to see its LDS writes (no block barrier).
  constexpr int RW = 8 * CHG;   // rows staged per wave
  float sreg[RW][NC];
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int ci = c0 + wave * RW + r;
      const float* xr = Xb + (long long)ci * p.xstride;
      const float* x2r = p.X2 ? p.X2 + (long long)b * p.xb + (long long)ci * p.xstride : nullptr;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + 64 * k, t = q0 * p.istr - p.halo_l + col;
        const bool ok = ci < p.Cin && col < xw && t >= 0 && t < len;
        float v = ok ? xr[t] : 0.f;
        if (x2r && ok) v += x2r[t];
        sreg[r][k] = v;
      }
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      float* lr = lds + (wave * RW + r) * xw;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (lane + 64 * k < xw) lr[lane + 64 * k] = sreg[r][k];
    }
  };
  if constexpr (KS && CHG == 4 && WPF) {
    // One-tap layers with the channels split over the waves, launched with so few blocks that a SIMD holds one wave
    // (short sequences: encoder FFNs, point-wise convs; with more blocks occupancy hides the latency and the extra
    // registers only cost).  A
    // wave's weights for a chunk are CHG float4 per lane; they are requested one chunk ahead together with the
    // staged rows, so the L2 latency of both hides behind the previous chunk's MFMAs instead of sitting in front of
    // every group of four.  Channels past CinP multiply zero weights (same accumulation order, same bits).
    float4 wn[CHG];
    auto wload = [&](int c0) {
#pragma unroll
      for (int g = 0; g < CHG; ++g) {
        const int gi = (c0 >> 3) + wave * CHG + g;
        wn[g] = (live && gi < groups) ? Wp[(long long)gi * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    stage_load(0);
    wload(0);
    const int col0 = p.halo_l + p.off[phase][0] + (lane & 31) * p.istr;
    for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
      if (c0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage_store();
      float4 wc[CHG];
#pragma unroll
      for (int g = 0; g < CHG; ++g) wc[g] = wn[g];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (c0 + kCh < p.CinP) { stage_load(c0 + kCh); wload(c0 + kCh); }
#pragma unroll
      for (int g = 0; g < CHG; ++g) {
        const float wa[4] = {wc[g].x, wc[g].y, wc[g].z, wc[g].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* xr = lds + ((wave * CHG + g) * 8 + j * 2 + (lane >> 5)) * xw + col0;
#pragma unroll
          for (int qb = 0; qb < QB; ++qb)
            acc[qb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j], xr[qb * 32 * p.istr], acc[qb], 0, 0, 0);
        }
      }
    }
  } else {
  stage_load(0);
  for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
    if (c0) { if (KS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else __syncthreads(); }   // previous chunk fully read
    stage_store();
    if (KS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else __syncthreads();
    if (c0 + kCh < p.CinP) stage_load(c0 + kCh);
    if (live) {
      // (tap, 8-channel group) steps in order over this wave's groups of the chunk (all of them, or with KS its own CHG),
      // the NEXT step's packed weights requested before this step's MFMAs and fenced there (the plain loop loads a float4,
      // waits an L2 round trip, issues 4 * QB MFMAs, and leaves hiding that latency to the other waves of the SIMD)
      typedef float f32x4v __attribute__((ext_vector_type(4)));
      const int gbase = KS ? wave * CHG : 0, gcap = KS ? CHG : NWV * CHG;
      int gl = (p.CinP - c0 + 7) / 8 - gbase;   // live groups of this chunk from gbase on
      gl = gl < gcap ? gl : gcap;
      const int nstep = gl > 0 ? ntap * gl : 0;
      const f32x4v* Wq = (const f32x4v*)Wp + ((long long)(c0 >> 3) + gbase) * 64 + lane;
      // two weight registers used in turn (see k_convb's step loop: one register rotated with `wv = wn` makes hipcc wait for the
      // weights it has just requested in the middle of the current step)
      auto advance = [&](int& t, int& gg) { if (++gg == gl) { gg = 0; ++t; } };
      auto wptr = [&](int t, int gg) { return Wq + ((long long)(t < ntap ? t : ntap - 1) * groups + gg) * 64; };
      auto step = [&](const f32x4v& wv, int t, int gg) {
        const int col0 = p.halo_l + p.off[phase][t] + (lane & 31) * p.istr;
        const float wa[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* xr = lds + ((gbase + gg) * 8 + j * 2 + (lane >> 5)) * xw + col0;
#pragma unroll
          for (int qb = 0; qb < QB; ++qb)
            acc[qb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j], xr[qb * 32 * p.istr], acc[qb], 0, 0, 0);
        }
      };
      if (nstep > 0) {
        int ta = 0, ga = 0;
        f32x4v wa_ = Wq[0];
        for (int st = 0; st < nstep; st += 2) {
          int tb = ta, gb = ga;
          advance(tb, gb);
          const f32x4v wb_ = *wptr(tb, gb);
          __builtin_amdgcn_sched_barrier(0);
          step(wa_, ta, ga);
          ta = tb; ga = gb;
          advance(ta, ga);
          wa_ = *wptr(ta, ga);
          __builtin_amdgcn_sched_barrier(0);
          if (st + 1 < nstep) step(wb_, tb, gb);
        }
      }
    }
  }

  }
  conv_finish<QB, KS>(p, acc, lds, ct, live, b, phase, q0, olen, lane, wave);
}


// ------------------------------------------------------------------------------------------
// k_convb: the same implicit GEMM on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, 16x the rate of the exact-fp32
// MFMA) with fp32 accuracy kept by a 2-plane split of BOTH operands: x = x_hi + x_mid (+ 2^-16 |x|), w likewise, and
//   w x ~= w_hi x_hi + w_hi x_mid + w_mid x_hi          (three products; the dropped terms are ~2^-17 relative)
// accumulated in fp32.  On the 0.5B vocoder this moves the waveform by 5e-5 max-abs against the fp32 path (CPU emulation
// and GPU test; north_star allows 1e-3).  Weights are split at pack time (two bf16 planes in A-operand order:
// [ct][tap][16-channel step][plane][lane][8 bf16], lane l = row l & 31, channels 8 (l >> 5) ..+7 of the step);
// activations are split while a chunk is staged: the thread that loaded eight consecutive channels of one time column packs
// them into one 16-byte B-operand piece per plane, LDS image [plane][octet][column][8 bf16].
// QB / KS / CHG / NC as k_conv (four waves; KS needs CHG >= 2 so that a wave owns whole 16-channel steps).
// ------------------------------------------------------------------------------------------
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {   // round-to-nearest-even pair -> packed bf16 (v_cvt_pk_bf16_f32)
  const bf16x2v h = __builtin_convertvector((f32x2v){a, b}, bf16x2v);
  return __builtin_bit_cast(uint32_t, h);
}
// eight fp32 -> hi plane and mid plane (x - hi, rounded again), 8 bf16 each
__device__ __forceinline__ void split2x8(const float (&v)[8], uint4& hi, uint4& mid) {
  uint32_t h[4], m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
    const float ra = v[2 * i] - __uint_as_float(h[i] << 16), rb = v[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u);
    m[i] = pk_bf16(ra, rb);
  }
  hi = make_uint4(h[0], h[1], h[2], h[3]);
  mid = make_uint4(m[0], m[1], m[2], m[3]);
}

// four waves per SIMD (<= 128 VGPRs; the kernels needed 112-134: no spill at 4, 100-220 bytes of scratch at 5).  PMC said the waves
// of these kernels are parked at s_waitcnt / s_barrier half of their cycles; a fourth resident wave covers more of that than deeper
// software pipelining did (A/B as separate builds, one box: vocoder batch 32 31.0 -> 29.8 ms, 8 prompt encodes 27.6 -> 27.2 ms).
#ifndef SMI_CB_OCC
#define SMI_CB_OCC 4
#endif
template <int QB, bool KS, int CHG, int NC, bool WPF = false, bool WALL = false>
__global__ __launch_bounds__(256, WALL ? 2 : SMI_CB_OCC) void k_convb(ConvP p) {
  static_assert(!KS || CHG % 2 == 0, "channel-split waves own whole 16-channel steps");
  static_assert(!WPF || (KS && CHG == 4), "WPF: one-tap layers with the channels split over the waves, 128-channel chunks");
  static_assert(!WALL || (KS && CHG == 2 && !WPF), "WALL: several taps, the channels split over the waves, one 16-channel step per wave and chunk");
  constexpr int kCh = 32 * CHG;        // channels per staged chunk (four waves x CHG octets)
  constexpr int NOCT = 4 * CHG;        // octets per chunk
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint4* lds16 = (uint4*)lds;          // [2 planes][NOCT][xw]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int QT = QB * 32;
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int b = bz / p.S, phase = bz - b * p.S;
  const int q0 = bx * QT;
  const int len = p.lens[b];
  const int olen = p.olens ? p.olens[b] : len;
  if (q0 >= olen) return;
  const int ct = KS ? by : by * 4 + wave;
  const bool live = ct * 32 < p.Cout;
  const int ntap = p.ntaps[phase];
  const int ksteps = (p.Cin + 15) >> 4;                 // 16-channel steps of the packed weights
  const float* Xb = p.X + (long long)b * p.xb;
  const uint4* Wp = (const uint4*)(p.W + p.wphase[phase]) + (long long)ct * ntap * ksteps * 128;

  f32x16 acc[QB];
#pragma unroll
  for (int i = 0; i < QB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int xw = p.xw;
  constexpr int RW = 8 * CHG;   // rows staged per wave = CHG octets
  float sreg[RW][NC];
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int ci = c0 + wave * RW + r;
      const float* xr = Xb + (long long)ci * p.xstride;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + 64 * k, t = q0 - p.halo_l + col;
        const bool ok = ci < p.Cin && col < xw && t >= 0 && t < len;
        sreg[r][k] = ok ? xr[t] : 0.f;
      }
    }
  };
  auto stage_store = [&]() {   // split + pack: one 16-byte piece per (octet, column, plane)
#pragma unroll
    for (int g = 0; g < CHG; ++g)
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = sreg[g * 8 + r][k];
        uint4 hi, mid;
        split2x8(v, hi, mid);
        if (lane + 64 * k < xw) {
          lds16[(size_t)(wave * CHG + g) * xw + lane + 64 * k] = hi;
          lds16[(size_t)(NOCT + wave * CHG + g) * xw + lane + 64 * k] = mid;
        }
      }
  };
  if constexpr (WPF) {
    // One-tap layers with the channels split over the waves, launched with so few blocks that a SIMD holds one or two waves
    // (one utterance: the prenet's point-wise convs, 80 blocks of 12 chunks at 150 frames).  A wave's work per chunk is 3 * QB * 2
    // MFMAs, so the loop runs at the pace of its memory round trips: with the weights requested one step ahead INSIDE a chunk
    // there were three of them per chunk (staged rows, first step's weights, second step's weights: ~3 us per chunk, 35 us per
    // layer).  Here the chunk's weights -- two steps x two planes, 16 registers -- are requested one chunk ahead together with
    // its staged rows: one round trip per chunk, hidden behind the previous chunk.  Same steps in the same order: same bits.
    if constexpr (QB == 1) {
      // One 32-column tile (short sequences): lanes 32-63 would idle in a row load, so a load instruction takes TWO rows (lanes 0-31 row j,
      // lanes 32-63 row 16 + j of the wave's 32): 16 + 4 loads per chunk -- and with 20 instead of 36 loads per chunk TWO chunks fit the
      // 6-bit vmcnt: two register sets, A and B, used in turn, every request unconditional (past the end: clamped addresses, masked
      // values, skipped steps) so that hipcc can count what is in flight: a chunk's round trip hides behind the chunk before it AND the
      // one being multiplied.  (With 36 loads per set the counter overflowed and the waits drained to vmcnt(0): measured, no gain.)
      const int rh = lane >> 5, colq = lane & 31;
      auto loadx = [&](float (&sr)[16], uint4 (&wq)[4], int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int ci = c0 + wave * RW + rh * 16 + j;
          const float* xr = Xb + (long long)(ci < p.Cin ? ci : p.Cin - 1) * p.xstride;
          const int t = q0 - p.halo_l + colq;
          sr[j] = xr[t < 0 ? 0 : (t < len ? t : len - 1)];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          int st = (c0 >> 4) + wave * 2 + g;
          st = st < ksteps ? st : ksteps - 1;
          wq[2 * g] = Wp[(long long)st * 128 + lane];          // (channel-split mode: every block's output tile is live)
          wq[2 * g + 1] = Wp[(long long)st * 128 + 64 + lane];
        }
      };
      const int col0 = p.halo_l + p.off[phase][0] + (lane & 31);
      auto chunk = [&](float (&sr)[16], uint4 (&wq)[4], int c0, bool first) {
        if (!first) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the previous chunk's LDS reads are done
        const int t = q0 - p.halo_l + colq;
        const bool okc = colq < xw && t >= 0 && t < len;
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = (okc && c0 + wave * RW + rh * 16 + o * 8 + r < p.Cin) ? sr[o * 8 + r] : 0.f;
          uint4 hi, mid;
          split2x8(v, hi, mid);
          if (colq < xw) {
            lds16[(size_t)(wave * CHG + 2 * rh + o) * xw + colq] = hi;
            lds16[(size_t)(NOCT + wave * CHG + 2 * rh + o) * xw + colq] = mid;
          }
        }
        uint4 wc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wc[i] = wq[i];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        loadx(sr, wq, c0 + 2 * kCh);                                       // this set's next chunk: two chunks ahead, unconditionally
        if (live) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            if ((c0 >> 4) + wave * 2 + g < ksteps) {   // wave-uniform
              const uint4* bp = lds16 + (size_t)(2 * (wave * 2 + g) + (lane >> 5)) * xw + col0;
              const bf16x8 ah = __builtin_bit_cast(bf16x8, wc[2 * g]), am = __builtin_bit_cast(bf16x8, wc[2 * g + 1]);
              const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[0]);
              const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)NOCT * xw]);
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[0], 0, 0, 0);
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[0], 0, 0, 0);
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[0], 0, 0, 0);
            }
          }
        }
      };
      float sa[16], sb[16];
      uint4 wa[4], wb[4];
      loadx(sa, wa, 0);
      loadx(sb, wb, kCh);
      for (int c0 = 0; c0 < p.CinP; c0 += 2 * kCh) {   // chunks in pairs (an odd count ends with a chunk of masked rows and skipped steps)
        chunk(sa, wa, c0, c0 == 0);
        chunk(sb, wb, c0 + kCh, false);
      }
      conv_finish<QB, KS>(p, acc, lds, ct, live, b, phase, q0, olen, lane, wave);
      return;
    }
    uint4 wn[4];
    const int ksl = ksteps;   // (steps past the last one multiply zero rows: their weights are clamped loads, never used)
    auto wload = [&](int c0) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        int st = (c0 >> 4) + wave * 2 + g;
        st = st < ksl ? st : ksl - 1;
        wn[2 * g] = live ? Wp[(long long)st * 128 + lane] : make_uint4(0u, 0u, 0u, 0u);
        wn[2 * g + 1] = live ? Wp[(long long)st * 128 + 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
      }
    };
    stage_load(0);
    wload(0);
    const int col0 = p.halo_l + p.off[phase][0] + (lane & 31);
    for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
      if (c0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage_store();
      uint4 wc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) wc[i] = wn[i];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (c0 + kCh < p.CinP) { stage_load(c0 + kCh); wload(c0 + kCh); }
      if (live) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          if ((c0 >> 4) + wave * 2 + g < ksl) {   // wave-uniform
            const uint4* bp = lds16 + (size_t)(2 * (wave * 2 + g) + (lane >> 5)) * xw + col0;
            const bf16x8 ah = __builtin_bit_cast(bf16x8, wc[2 * g]), am = __builtin_bit_cast(bf16x8, wc[2 * g + 1]);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
              const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
              const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)NOCT * xw + qb * 32]);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[qb], 0, 0, 0);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[qb], 0, 0, 0);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[qb], 0, 0, 0);
            }
          }
        }
      }
    }
    conv_finish<QB, KS>(p, acc, lds, ct, live, b, phase, q0, olen, lane, wave);
    return;
  }
  if constexpr (WALL) {
    // Several taps, the channels split over the waves, launched with about a block per CU (one utterance: the 7-tap convs at C = 768 /
    // 384, conv_in, the prenet's embed convs, the transposed convs of the first two decoder blocks).  A wave's chunk is ONE 16-channel
    // step x taps; with the next tap's weights requested one step ahead the taps were a chain of dependent round trips to cold
    // weights -- 7 x ~0.8 us per chunk, 72 us for the 7-tap conv at C = 768 where its MFMAs need 7.  Here ALL taps' weight planes of the
    // chunk (<= 8 x 2 KiB per wave: 64 registers, hence two waves per SIMD) are requested together at the top of the chunk, behind the
    // staged rows requested one chunk earlier: one round trip per chunk.  Same taps in the same order: same bits.
    stage_load(0);
    for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
      const int stp = (c0 >> 4) + wave;                 // this wave's 16-channel step of the chunk
      const bool has = live && stp < ksteps;             // wave-uniform
      uint4 wt[kMaxTaps][2];
      {
        const uint4* Wq = Wp + (long long)(stp < ksteps ? stp : ksteps - 1) * 128 + lane;
#pragma unroll
        for (int t = 0; t < kMaxTaps; ++t) {
          const int tc = t < ntap ? t : ntap - 1;
          wt[t][0] = live ? Wq[(long long)tc * ksteps * 128] : make_uint4(0u, 0u, 0u, 0u);
          wt[t][1] = live ? Wq[(long long)tc * ksteps * 128 + 64] : make_uint4(0u, 0u, 0u, 0u);
        }
      }
      if (c0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      stage_store();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (c0 + kCh < p.CinP) stage_load(c0 + kCh);
      if (has) {
#pragma unroll
        for (int t = 0; t < kMaxTaps; ++t) {
          if (t < ntap) {   // uniform
            const int col0 = p.halo_l + p.off[phase][t] + (lane & 31);
            const uint4* bp = lds16 + (size_t)(2 * wave + (lane >> 5)) * xw + col0;
            const bf16x8 ah = __builtin_bit_cast(bf16x8, wt[t][0]), am = __builtin_bit_cast(bf16x8, wt[t][1]);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
              const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
              const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)NOCT * xw + qb * 32]);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[qb], 0, 0, 0);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[qb], 0, 0, 0);
              acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[qb], 0, 0, 0);
            }
          }
        }
      }
    }
    conv_finish<QB, KS>(p, acc, lds, ct, live, b, phase, q0, olen, lane, wave);
    return;
  }
  stage_load(0);
  for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
    if (c0) { if (KS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else __syncthreads(); }   // previous chunk fully read
    stage_store();
    if (KS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else __syncthreads();
    if (c0 + kCh < p.CinP) stage_load(c0 + kCh);
    if (live) {
      // (tap, 16-channel step) steps in order over this wave's steps of the chunk (all 2 CHG of them, or with KS its own
      // CHG / 2); the NEXT step's two weight planes are requested before this step's MFMAs and fenced there
      const int sbase = KS ? wave * (CHG / 2) : 0, scap = KS ? CHG / 2 : 2 * CHG;
      int sl = ksteps - (c0 >> 4) - sbase;            // live steps of this chunk from sbase on
      sl = sl < scap ? sl : scap;
      const int nstep = sl > 0 ? ntap * sl : 0;
      const uint4* Wq = Wp + ((long long)(c0 >> 4) + sbase) * 128 + lane;
      // Two weight sets, A and B, used in turn (the loop advances two steps per trip): written as ONE set with `w = w_next` at the end
      // of a step, hipcc copies the registers there and waits vmcnt(0) for the just-requested next weights in the MIDDLE of the
      // current step's MFMAs (round-4 ISA of the 7-tap conv: every step exposed a whole L2 round trip; the prefetch hid nothing).
      // A set that is loaded straight into its own registers after its last use needs no copy, and the wait in front of a step's
      // MFMAs leaves the other set's request in flight.
      auto advance = [&](int& t, int& gg) { if (++gg == sl) { gg = 0; ++t; } };
      auto wptr = [&](int t, int gg) { return Wq + ((long long)(t < ntap ? t : ntap - 1) * ksteps + gg) * 128; };   // (past the end: a valid address, never used)
      auto step = [&](const uint4& wh, const uint4& wm, int t, int gg) {
        const int col0 = p.halo_l + p.off[phase][t] + (lane & 31);
        const uint4* bp = lds16 + (size_t)(2 * (sbase + gg) + (lane >> 5)) * xw + col0;
        const bf16x8 ah = __builtin_bit_cast(bf16x8, wh), am = __builtin_bit_cast(bf16x8, wm);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
          const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)NOCT * xw + qb * 32]);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[qb], 0, 0, 0);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[qb], 0, 0, 0);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[qb], 0, 0, 0);
        }
      };
      if (nstep > 0) {
        int ta = 0, ga = 0;                      // set A's step
        uint4 wah = Wq[0], wam = Wq[64];
        for (int st = 0; st < nstep; st += 2) {
          int tb = ta, gb = ga;
          advance(tb, gb);                       // set B's step = A's successor
          const uint4* pb = wptr(tb, gb);
          const uint4 wbh = pb[0], wbm = pb[64];
          __builtin_amdgcn_sched_barrier(0);
          step(wah, wam, ta, ga);
          ta = tb; ga = gb;
          advance(ta, ga);                       // A's next step = B's successor
          const uint4* pa = wptr(ta, ga);
          wah = pa[0]; wam = pa[64];
          __builtin_amdgcn_sched_barrier(0);
          if (st + 1 < nstep) step(wbh, wbm, tb, gb);
        }
      }
    }
  }
  conv_finish<QB, KS>(p, acc, lds, ct, live, b, phase, q0, olen, lane, wave);
}

// k_convbT (round 4): ConvTranspose1d on the bf16-split pipe with PH output PHASES per block.  As a polyphase conv on k_convb
// every phase r is its own set of blocks (grid.z = B * S): the input tile is staged S times, and -- what costs -- output element
// (q, r) lives at t = q * S + r, so a phase's stores put 4 bytes per lane at a stride of 4 S bytes: 64 store instructions per wave
// (16 rows x 2 column tiles x 2 outputs), each spread over 64 different 32-byte sectors -- about half of the kernel's time
// (the transposed convs ran at 118-154 TFLOP/s fp32-equivalent beside 280-320 for the 7-tap convs of the same shapes).  Here a
// block keeps PH accumulator sets (PH * 16 registers) for ONE 32-column tile: the chunk is staged once for the PH phases -- 32 + halo
// <= 64 columns, one 64-lane pass per row -- and in the epilogue a lane holds the PH consecutive outputs t = q S + r0 .. + PH - 1 of
// each of its rows: one 16-byte store (PH = 4) or PH dword stores per row.  Measured (profiles/r04_convT_multi_phase.txt): what pays
// is the STAGING -- a 2-tap phase carries 24 MFMAs per 32 staged channels against ~150 staging instructions (loads, the fp32 -> 2 x
// bf16 split, LDS writes), PH phases share them; the stores alone (first build: two passes per row as in k_convb) changed nothing.
// A phase's taps and 16-channel steps run in k_convb's order (64-channel chunks), one accumulator per phase: the bits of k_convb
// with CHG = 2.  Epilogue: bias, raw output and / or the next layer's Snake -- what the WaveGenerator's transposed convs need (the
// launch builder checks that nothing else is asked for).
template <int PH>
__global__ __launch_bounds__(256, 3) void k_convbT(ConvP p) {
  constexpr int QB = 1, NC = 1, CHG = 2, NOCT = 4 * CHG, kCh = 32 * CHG, RW = 8 * CHG;   // 32 + halo <= 64 staged columns: ONE 64-lane pass per row
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint4* lds16 = (uint4*)lds;          // [2 planes][NOCT][xw]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int QT = QB * 32;
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int ngrp = p.S / PH;
  const int b = bz / ngrp, phase0 = (bz - b * ngrp) * PH;
  const int q0 = bx * QT;
  const int len = p.lens[b];
  if (q0 >= len) return;
  const int ct = by * 4 + wave;
  const bool live = ct * 32 < p.Cout;
  const int ksteps = (p.Cin + 15) >> 4;
  const float* Xb = p.X + (long long)b * p.xb;
  f32x16 acc[PH][QB];
#pragma unroll
  for (int h = 0; h < PH; ++h)
#pragma unroll
    for (int i = 0; i < QB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[h][i][r] = 0.f;
  const int xw = p.xw;
  float sreg[RW][NC];
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int ci = c0 + wave * RW + r;
      const float* xr = Xb + (long long)(ci < p.Cin ? ci : p.Cin - 1) * p.xstride;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + 64 * k, t = q0 - p.halo_l + col;
        const bool ok = ci < p.Cin && col < xw && t >= 0 && t < len;
        const float v = xr[t < 0 ? 0 : (t < len ? t : len - 1)];   // unconditional load from a clamped address, masked by value
        sreg[r][k] = ok ? v : 0.f;
      }
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int g = 0; g < CHG; ++g)
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = sreg[g * 8 + r][k];
        uint4 hi, mid;
        split2x8(v, hi, mid);
        if (lane + 64 * k < xw) {
          lds16[(size_t)(wave * CHG + g) * xw + lane + 64 * k] = hi;
          lds16[(size_t)(NOCT + wave * CHG + g) * xw + lane + 64 * k] = mid;
        }
      }
  };
  // weights of (phase, tap, step): two 1-KiB planes at wbase(phase) + ((tap * ksteps + step) * 128 + lane [+ 64])
  auto wbase = [&](int phase) { return (const uint4*)(p.W + p.wphase[phase]) + (long long)ct * p.ntaps[phase] * ksteps * 128 + lane; };
  stage_load(0);
  for (int c0 = 0; c0 < p.CinP; c0 += kCh) {
    if (c0) __syncthreads();   // previous chunk fully read
    stage_store();
    __syncthreads();
    if (c0 + kCh < p.CinP) stage_load(c0 + kCh);
    if (live) {
      int sl = ksteps - (c0 >> 4);
      sl = sl < 2 * CHG ? sl : 2 * CHG;            // live 16-channel steps of this chunk (>= 1)
      const long long so = (long long)(c0 >> 4) * 128;
      // two weight sets used in turn, as in k_convb (a single set rotated with `w = w_next` makes hipcc wait for the just-requested
      // weights in the middle of the current step); a phase's last step requests the NEXT phase's first weights
      uint4 wah, wam;
      { const uint4* w0 = wbase(phase0) + so; wah = w0[0]; wam = w0[64]; }
#pragma unroll
      for (int h = 0; h < PH; ++h) {
        const int phase = phase0 + h, ntap = p.ntaps[phase];
        const uint4* Wq = wbase(phase) + so;
        const uint4* Wnext = wbase(h + 1 < PH ? phase + 1 : phase) + so;   // the next phase's first step (last phase: any valid address)
        const int nstep = ntap * sl;
        auto advance = [&](int& t, int& gg) { if (++gg == sl) { gg = 0; ++t; } };
        auto wptr = [&](int t, int gg) { return t >= ntap ? Wnext : Wq + ((long long)t * ksteps + gg) * 128; };
        auto step = [&](const uint4& wh, const uint4& wm, int t, int gg) {
          const int col0 = p.halo_l + p.off[phase][t] + (lane & 31);
          const uint4* bp = lds16 + (size_t)(2 * gg + (lane >> 5)) * xw + col0;
          const bf16x8 ah = __builtin_bit_cast(bf16x8, wh), am = __builtin_bit_cast(bf16x8, wm);
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
            const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)NOCT * xw + qb * 32]);
            acc[h][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[h][qb], 0, 0, 0);
            acc[h][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[h][qb], 0, 0, 0);
            acc[h][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[h][qb], 0, 0, 0);
          }
        };
        int ta = 0, ga = 0;
        for (int st = 0; st < nstep; st += 2) {
          int tb = ta, gb = ga;
          advance(tb, gb);
          const uint4* pb = wptr(tb, gb);                 // (an odd step count: the phase's successor, i.e. the next phase's first weights)
          uint4 wbh = pb[0], wbm = pb[64];
          __builtin_amdgcn_sched_barrier(0);
          step(wah, wam, ta, ga);
          if (st + 1 < nstep) {
            ta = tb; ga = gb;
            advance(ta, ga);
            const uint4* pa = wptr(ta, ga);
            wah = pa[0]; wam = pa[64];
            __builtin_amdgcn_sched_barrier(0);
            step(wbh, wbm, tb, gb);
          } else {
            wah = wbh; wam = wbm;                          // odd count: B already holds the next phase's first weights
          }
        }
      }
    }
  }
  if (!live) return;
  // epilogue: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 (the 32x32 MFMA D layout)
  const long long yboff = (long long)b * p.yb;
  const bool hb = p.bias != nullptr, hs = p.Ys != nullptr, hy = p.Y != nullptr, fsin = p.fast_sin != 0;
  const float* dummy = p.X;
#pragma unroll
  for (int r0 = 0; r0 < 16; r0 += 8) {
    float bv[8], av[8];
    int co[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + i;
      co[i] = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const int cc = co[i] < p.Cout ? co[i] : p.Cout - 1;
      bv[i] = (hb ? p.bias : dummy)[cc];
      av[i] = (hs ? p.alpha : dummy)[cc];
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const int q = q0 + qb * 32 + (lane & 31);
      if (q >= len) continue;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (co[i] >= p.Cout) continue;
        float y[PH], ys[PH];
#pragma unroll
        for (int h = 0; h < PH; ++h) {
          y[h] = acc[h][qb][r0 + i];
          y[h] = hb ? y[h] + bv[i] : y[h];
          ys[h] = snake_f(y[h], av[i], fsin);
        }
        const long long o = yboff + (long long)co[i] * p.ystride + (long long)q * p.S + phase0;
        if constexpr (PH == 4) {
          if (hy) *(float4*)(p.Y + o) = make_float4(y[0], y[1], y[2], y[3]);
          if (hs) *(float4*)(p.Ys + o) = make_float4(ys[0], ys[1], ys[2], ys[3]);
        } else {
#pragma unroll
          for (int h = 0; h < PH; ++h) {
            if (hy) p.Y[o + h] = y[h];
            if (hs) p.Ys[o + h] = ys[h];
          }
        }
      }
    }
  }
}

// k_resunit (round 4): a whole ResidualUnit (blocks/layers.py:51-67) in ONE launch where a block can hold every channel of its
// time tile -- C = 96 (three waves) and C = 192 (six waves), the two resolutions at which the unit is bound by memory, not by the
// matrix pipe: y = x + conv1(snake(conv7_dil(snake(x)))).  As two launches the 7-tap conv writes A = snake(conv7 + b) to HBM and the
// 1x1 conv reads it back, stages it and splits it again: six passes over a [C][T] tensor per unit (Xs in, A out | A in, residual in,
// raw out, Snake'd out).  Here wave w owns output tile w in BOTH convs: phase 1 is k_convb's 7-tap loop (48-channel chunks: 8 rows per
// wave x 6 waves, or 16 x 3); its accumulators -- register r of lane l = channel 32 w + (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31:
// four consecutive channels per lane -- get bias and Snake, are split into the two bf16 planes and go straight into the LDS image of
// the 1x1 conv's B operand ([plane][octet][column][8 bf16], over the dead staging rows); phase 2 multiplies W1 (2 KiB per step from
// L2) against that image, adds bias and the residual and writes the unit's two outputs.  Four passes per unit, no second staging.
// Same products and the same (tap, step) order per chunk as k_convb; the 7-tap sum runs over 48- instead of 32-channel chunks.
template <int NWV>
__global__ __launch_bounds__(NWV * 64) void k_resunit(ResP p) {
  constexpr int QB = 2, NC = 2, RW = 48 / NWV, OPW = RW / 8;   // 64 columns per block; rows / octets staged per wave per 48-channel chunk
  static_assert(NWV == 3 || NWV == 6, "C = 96 or 192");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  uint4* lds16 = (uint4*)lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, q0 = blockIdx.x * (QB * 32);
  const int len = p.lens[b];
  if (q0 >= len) return;
  const int C = p.C, ksteps = C >> 4, xw = p.xw;
  const float* Xb = p.Xs + (long long)b * p.bs;
  f32x16 acc[QB];
#pragma unroll
  for (int i = 0; i < QB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float sreg[RW][NC];
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float* xr = Xb + (long long)(c0 + wave * RW + r) * p.stride;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + 64 * k, t = q0 - p.halo_l + col;
        const bool ok = col < xw && t >= 0 && t < len;
        const float v = xr[t < 0 ? 0 : (t < len ? t : len - 1)];
        sreg[r][k] = ok ? v : 0.f;
      }
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int g = 0; g < OPW; ++g)
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = sreg[g * 8 + r][k];
        uint4 hi, mid;
        split2x8(v, hi, mid);
        if (lane + 64 * k < xw) {
          lds16[(size_t)(wave * OPW + g) * xw + lane + 64 * k] = hi;
          lds16[(size_t)(6 + wave * OPW + g) * xw + lane + 64 * k] = mid;
        }
      }
  };
  // ---- phase 1: the dilated 7-tap conv, output tile `wave`
  {
    const uint4* Wp = (const uint4*)p.W7 + (long long)wave * 7 * ksteps * 128 + lane;
    stage_load(0);
    for (int c0 = 0; c0 < C; c0 += 48) {
      if (c0) __syncthreads();
      stage_store();
      __syncthreads();
      if (c0 + 48 < C) stage_load(c0 + 48);
      const uint4* Wq = Wp + (long long)(c0 >> 4) * 128;
      // 7 taps x 3 steps, two weight sets used in turn (k_convb's step loop: no register rotation, no wait for the set just requested)
      auto advance = [&](int& t, int& gg) { if (++gg == 3) { gg = 0; ++t; } };
      auto wptr = [&](int t, int gg) { return Wq + ((long long)(t < 7 ? t : 6) * ksteps + gg) * 128; };
      auto step = [&](const uint4& wh, const uint4& wm, int t, int gg) {
        const uint4* bp = lds16 + (size_t)(2 * gg + (lane >> 5)) * xw + p.halo_l + p.off[t] + (lane & 31);
        const bf16x8 ah = __builtin_bit_cast(bf16x8, wh), am = __builtin_bit_cast(bf16x8, wm);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
          const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)6 * xw + qb * 32]);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[qb], 0, 0, 0);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[qb], 0, 0, 0);
          acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[qb], 0, 0, 0);
        }
      };
      int ta = 0, ga = 0;
      uint4 wah = Wq[0], wam = Wq[64];
      for (int st = 0; st < 7 * 3; st += 2) {
        int tb = ta, gb = ga;
        advance(tb, gb);
        const uint4* pb = wptr(tb, gb);
        const uint4 wbh = pb[0], wbm = pb[64];
        __builtin_amdgcn_sched_barrier(0);
        step(wah, wam, ta, ga);
        ta = tb; ga = gb;
        advance(ta, ga);
        const uint4* pa = wptr(ta, ga);
        wah = pa[0]; wam = pa[64];
        __builtin_amdgcn_sched_barrier(0);
        if (st + 1 < 7 * 3) step(wbh, wbm, tb, gb);
      }
    }
  }
  // ---- A = snake(conv7 + b7, alpha2) -> the 1x1 conv's B operand in LDS: [plane][octet = channel / 8][64 columns][8 bf16]
  const int noct = C >> 3;
  const uint4* W1p = (const uint4*)p.W1 + (long long)wave * ksteps * 128 + lane;
  uint4 wh = W1p[0], wm = W1p[64];         // the first step's 1x1 weights travel under the Snake arithmetic
  __syncthreads();                          // every wave has read the last staged chunk: the image may overwrite it
  {
    const bool fsin = p.fast_sin != 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float bv[4], av[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const int c = wave * 32 + 8 * k + 4 * (lane >> 5) + e; bv[e] = p.b7[c]; av[e] = p.alpha2[c]; }
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = snake_f(acc[qb][4 * k + e] + bv[e], av[e], fsin);
        const uint32_t h0 = pk_bf16(a[0], a[1]), h1 = pk_bf16(a[2], a[3]);
        const uint32_t m0 = pk_bf16(a[0] - __uint_as_float(h0 << 16), a[1] - __uint_as_float(h0 & 0xffff0000u));
        const uint32_t m1 = pk_bf16(a[2] - __uint_as_float(h1 << 16), a[3] - __uint_as_float(h1 & 0xffff0000u));
        unsigned char* q = (unsigned char*)lds + ((size_t)(wave * 4 + k) * 64 + qb * 32 + (lane & 31)) * 16 + 8 * (lane >> 5);
        *(uint2*)q = make_uint2(h0, h1);
        *(uint2*)(q + (size_t)noct * 64 * 16) = make_uint2(m0, m1);
      }
    }
  }
  __syncthreads();
  // ---- phase 2: the 1x1 conv on the image, output tile `wave`
#pragma unroll
  for (int i = 0; i < QB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  {
    auto step2 = [&](const uint4& xh, const uint4& xm, int st) {
      const uint4* bp = lds16 + (size_t)(2 * st + (lane >> 5)) * 64 + (lane & 31);
      const bf16x8 ah = __builtin_bit_cast(bf16x8, xh), am = __builtin_bit_cast(bf16x8, xm);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, bp[qb * 32]);
        const bf16x8 bm = __builtin_bit_cast(bf16x8, bp[(size_t)noct * 64 + qb * 32]);
        acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[qb], 0, 0, 0);
        acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[qb], 0, 0, 0);
        acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[qb], 0, 0, 0);
      }
    };
    for (int st = 0; st < ksteps; st += 2) {      // ksteps = C / 16 = 6 or 12: even; (wh, wm) is set A, already requested
      const uint4 wbh = W1p[(long long)(st + 1) * 128], wbm = W1p[(long long)(st + 1) * 128 + 64];
      __builtin_amdgcn_sched_barrier(0);
      step2(wh, wm, st);
      const int sn = st + 2 < ksteps ? st + 2 : st;
      wh = W1p[(long long)sn * 128]; wm = W1p[(long long)sn * 128 + 64];
      __builtin_amdgcn_sched_barrier(0);
      step2(wbh, wbm, st + 1);
    }
  }
  // ---- epilogue: + b1 + residual; raw and Snake'd outputs (all loads of eight rows first, as in conv_finish)
  const long long boff = (long long)b * p.bs;
  const bool hs = p.Ys != nullptr, hy = p.Y != nullptr, fsin = p.fast_sin != 0;
  bool qok[QB];
  int tq[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) { const int q = q0 + qb * 32 + (lane & 31); qok[qb] = q < len; tq[qb] = qok[qb] ? q : len - 1; }
#pragma unroll
  for (int r0 = 0; r0 < 16; r0 += 8) {
    float bv[8], av[8], rv[QB][8];
    int co[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + i;
      co[i] = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      bv[i] = p.b1[co[i]];
      av[i] = (hs ? p.alpha_next : p.b1)[co[i]];
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) rv[qb][i] = p.U[boff + (long long)co[i] * p.stride + tq[qb]];
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float y = acc[qb][r0 + i];
        y = y + bv[i];
        y = rv[qb][i] + y;
        if (qok[qb]) {
          const long long o = boff + (long long)co[i] * p.stride + tq[qb];
          if (hy) p.Y[o] = y;
          if (hs) p.Ys[o] = snake_f(y, av[i], fsin);
        }
      }
  }
}

// Conv1d with ONE output channel (the vocoder's last layer: C -> 1, 7 taps, tanh): y[b][q] = act(bias + sum_ci sum_tap W[ci][tap]
// x[b][ci][q + off[tap]]).  On the MFMA kernels 31 of a tile's 32 output rows are padding and the layer -- 393 MB of
// activations at batch 32 -- ran at 0.3 TB/s (1.3 ms); here a thread owns one output sample, rows are read coalesced along time
// (a sample is re-read by its 7 taps: L1 hits), weights come from LDS (unpacked from the conv layout: lane l, slot j of group g
// holds W[l & 31][8g + 2j + (l >> 5)]), every load is unconditional (clamped index, masked value).
template <int NTAP>
__global__ __launch_bounds__(256) void k_conv_c1(ConvP p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];      // [Cin][NTAP]
  const int tid = threadIdx.x, b = blockIdx.y, q = blockIdx.x * 256 + tid;
  const int len = p.lens[b], olen = p.olens ? p.olens[b] : len;
  if ((int)blockIdx.x * 256 >= olen) return;
  const int groups = p.CinP >> 3;
  const float* Wf = p.W + p.wphase[0];
  for (int i = tid; i < p.Cin * NTAP; i += 256) {
    const int ci = i / NTAP, tap = i - ci * NTAP;
    lds[i] = Wf[((size_t)(tap * groups + (ci >> 3)) * 64 + (ci & 1) * 32) * 4 + ((ci & 7) >> 1)];
  }
  __syncthreads();
  if (q >= olen) return;
  int tt[NTAP];
  bool ok[NTAP];
#pragma unroll
  for (int k = 0; k < NTAP; ++k) {
    const int t = q + p.off[0][k];
    ok[k] = t >= 0 && t < len;
    tt[k] = t < 0 ? 0 : (t < len ? t : len - 1);
  }
  const float* Xb = p.X + (long long)b * p.xb;
  float acc = 0.f;
  for (int c0 = 0; c0 < p.Cin; c0 += 4) {
    float v[4][NTAP];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ci = c0 + u < p.Cin ? c0 + u : p.Cin - 1;
      const float* xr = Xb + (long long)ci * p.xstride;
#pragma unroll
      for (int k = 0; k < NTAP; ++k) v[u][k] = xr[tt[k]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (c0 + u < p.Cin) {
#pragma unroll
        for (int k = 0; k < NTAP; ++k) acc = fmaf(lds[(c0 + u) * NTAP + k], ok[k] ? v[u][k] : 0.f, acc);
      }
    }
  }
  float y = acc;
  if (p.bias) y += p.bias[0];
  if (p.act == ACT_GELU) y = gelu_f(y);
  if (p.act == ACT_RELU) y = fmaxf(y, 0.f);
  if (p.act == ACT_TANH) y = tanhf(y);
  p.Y[(long long)b * p.yb + q] = y;
}

// Linear layer on one vector per utterance (d-vector projection, AdaLN parameters): y[b][co] =
// bias[co] + sum_ci W[co][ci] x[b][ci], fp32, reading the same packed conv weights (lane l, slot j of
// group g holds W[32*ct + (l&31)][8g + 2j + (l>>5)]).  One block per 32 outputs, waves split K.
__global__ __launch_bounds__(256) void k_gemv1(ConvP p) {
  __shared__ float part[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ct = blockIdx.x, b = blockIdx.y;
  const int groups = p.CinP >> 3;
  const float4* Wp = (const float4*)p.W + (long long)ct * groups * 64;
  const float* x = p.X + (long long)b * p.xb;           // xstride == 1: x[ci]
  float acc = 0.f;
  for (int g = wave; g < groups; g += 4) {
    const float4 w = Wp[(long long)g * 64 + lane];
    const int ci = g * 8 + (lane >> 5);
    const float x0 = ci < p.Cin ? x[ci] : 0.f, x1 = ci + 2 < p.Cin ? x[ci + 2] : 0.f;
    const float x2 = ci + 4 < p.Cin ? x[ci + 4] : 0.f, x3 = ci + 6 < p.Cin ? x[ci + 6] : 0.f;
    acc += (w.x * x0 + w.y * x1) + (w.z * x2 + w.w * x3);
  }
  acc += __shfl_xor(acc, 32, 64);
  if (lane < 32) part[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < 32) {
    const int co = ct * 32 + threadIdx.x;
    if (co < p.Cout) {
      float y = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
      if (p.bias) y += p.bias[co];
      if (p.act == ACT_RELU) y = fmaxf(y, 0.f);
      if (p.act == ACT_SIGMOID) y = 1.0f / (1.0f + expf(-y));
      p.Y[(long long)b * p.yb + co] = y;
    }
  }
}

template <int CPT>  // channels per thread (C <= 32*CPT): 8 time steps x 32 channel groups per block
__global__ __launch_bounds__(256) void k_dwln(LnP p) {
  __shared__ float red[32][8];
  const int tt = threadIdx.x & 7, cg = threadIdx.x >> 3;
  const int b = blockIdx.y, t = blockIdx.x * 8 + tt;
  const int len = p.lens[b];
  const bool tv = t < len;
  const float* Xb = p.X + (long long)b * p.bs;
  float v[CPT];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = cg + 32 * i;
    float x = 0.f;
    if (c < p.C && tv) {
      const float* xr = Xb + (long long)c * p.stride;
      if (p.dww) {
        x = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int tj = t + j - 3;
          const float xv = (tj >= 0 && tj < len) ? xr[tj] : 0.f;
          x += p.dww[c * 7 + j] * xv;
        }
        x += p.dwb[c];
      } else {
        x = xr[t];
      }
    }
    v[i] = x;
    s += x;
  }
  red[cg][tt] = s;
  __syncthreads();
  float mean = 0.f;
#pragma unroll
  for (int g = 0; g < 32; ++g) mean += red[g][tt];
  mean /= (float)p.C;
  __syncthreads();
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = cg + 32 * i;
    if (c < p.C) { const float d = v[i] - mean; q += d * d; }
  }
  red[cg][tt] = q;
  __syncthreads();
  float var = 0.f;
#pragma unroll
  for (int g = 0; g < 32; ++g) var += red[g][tt];
  const float rstd = 1.0f / sqrtf(var / (float)p.C + p.eps);
  if (!tv) return;
  float* Yb = p.Y + (long long)b * p.bs;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = cg + 32 * i;
    if (c >= p.C) continue;
    float y = (v[i] - mean) * rstd;
    if (p.ada) y = y * p.ada[(long long)b * p.ada_stride + c] + p.ada[(long long)b * p.ada_stride + p.C + c];
    else y = y * p.w[c] + p.bsh[c];
    if (p.triple) y = (y + y) + y;
    if (p.gelu) y = gelu_f(y);
    Yb[(long long)c * p.stride + t] = y;
  }
}

// codebook lookup: Z[b][d][t] = codebook[sem[b][t]][d]   (factorized_vector_quantize.py:160-167)
__global__ void k_codebook(const int64_t* sem, int semstride, const float* cb, int D, int cbsize,
                           const int* lens, float* Z, int zstride, long long zb) {
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lens[b]) return;
  long long id = sem[(long long)b * semstride + t];
  id = id < 0 ? 0 : (id >= cbsize ? cbsize - 1 : id);
  for (int d = 0; d < D; ++d) Z[(long long)b * zb + (long long)d * zstride + t] = cb[id * D + d];
}

// FSQ index -> level codes -> Linear(nd -> latent), written d-major: out[b][d*Ntok + t]
// (finite_scalar_quantization.py:143-162, residual_fsq.py:191-199, speaker_encoder.py:109-110)
__global__ void k_fsq(FsqP p) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < p.latent * p.Ntok; i += blockDim.x) {
    const int d = i / p.Ntok, t = i - d * p.Ntok;
    int idx = p.glob[b * p.Ntok + t];
    float acc = 0.f;
    int basis = 1;
    for (int j = 0; j < p.nd; ++j) {
      const int L = p.levels[j], half = L / 2;
      const int lvl = (idx / basis) % L;
      const float code = (float)(lvl - half) / (float)half;
      acc += code * p.W1[d * p.nd + j];
      basis *= L;
    }
    p.out[(long long)b * p.latent * p.Ntok + i] = acc + p.b1[d];
  }
}

__global__ void k_zero_tail(float* wav, int stride, const int* lens, int hop) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < stride && t >= lens[b] * hop) wav[(long long)b * stride + t] = 0.f;
}

}  // namespace

// Conv1d (S = 1): tap j reads x[t + j*dil - pad].  ConvTranspose1d (stride S, padding pad):
// out[q*S + r] += W[ci][co][j] * x[ci][(q*S + r + pad - j)/S] for j == (r + pad) mod S.
ConvGeom conv_geom(int Cout, int Cin, int K, int dil, int pad, int S, bool bf) {
  ConvGeom g;
  memset(&g, 0, sizeof(g));
  g.S = S;
  long long o = 0;
  int lo = 0, hi = 0;
  // fp32 packing: [ct][tap][8-channel group][lane][4 floats]; bf16-split packing: [ct][tap][16-channel step][2 planes][lane][8 bf16]
  const long long per_tap = bf ? (long long)(pad32(Cout) / 32) * ((Cin + 15) / 16) * 512
                               : (long long)(pad32(Cout) / 32) * (pad8(Cin) / 8) * 256;
  for (int r = 0; r < S; ++r) {
    g.wphase[r] = o;
    int n = 0;
    if (S == 1) {
      for (int j = 0; j < K; ++j) { g.off[r][n] = j * dil - pad; g.tapk[r][n] = j; ++n; }
    } else {
      const int j0 = (r + pad) % S, c = (r + pad) / S;
      for (int i = 0; j0 + S * i < K; ++i) { g.off[r][n] = c - i; g.tapk[r][n] = j0 + S * i; ++n; }
    }
    g.ntaps[r] = n;
    for (int i = 0; i < n; ++i) { lo = g.off[r][i] < lo ? g.off[r][i] : lo; hi = g.off[r][i] > hi ? g.off[r][i] : hi; }
    o += per_tap * n;
  }
  g.halo_l = -lo; g.halo_r = hi; g.floats = o;
  return g;
}

namespace {
// every launcher takes grid, block and dynamic LDS from the record make_conv() left
typedef void (*ConvLaunchFn)(const Launch&, hipStream_t);
template <int QB, bool KS, int CHG, int NC, bool WPF, int NWV>
void launch_k_conv(const Launch& L, hipStream_t st) { hipLaunchKernelGGL((k_conv<QB, KS, CHG, NC, WPF, NWV>), L.grid, dim3(L.blk), L.lds, st, L.cp); }
template <int QB, bool KS, int CHG, int NC, bool WPF, bool WALL>
void launch_k_convb(const Launch& L, hipStream_t st) { hipLaunchKernelGGL((k_convb<QB, KS, CHG, NC, WPF, WALL>), L.grid, dim3(L.blk), L.lds, st, L.cp); }
template <int PH>
void launch_k_convbT(const Launch& L, hipStream_t st) { hipLaunchKernelGGL((k_convbT<PH>), L.grid, dim3(L.blk), L.lds, st, L.cp); }
inline void launch_k_conv_c1(const Launch& L, hipStream_t st) { hipLaunchKernelGGL((k_conv_c1<7>), L.grid, dim3(L.blk), L.lds, st, L.cp); }
inline void launch_k_gemv1(const Launch& L, hipStream_t st) { hipLaunchKernelGGL(k_gemv1, L.grid, dim3(L.blk), L.lds, st, L.cp); }

struct ConvFormEntry { ConvForm form; ConvLaunchFn launch; };
#define SMI_F_CONV(QB_, KS_, CHG_, NC_, WPF_, NWV_) {{CONV_K_CONV, QB_, KS_, CHG_, NC_, NWV_, WPF_, 0, 0}, launch_k_conv<QB_, KS_, CHG_, NC_, WPF_, NWV_>}
#define SMI_F_CONVB(QB_, KS_, CHG_, NC_, WPF_, WALL_) {{CONV_K_CONVB, QB_, KS_, CHG_, NC_, 4, WPF_, WALL_, 0}, launch_k_convb<QB_, KS_, CHG_, NC_, WPF_, WALL_>}
// every instantiation the library carries (the order is the enumeration order of smi_conv_form_entry)
const ConvFormEntry kConvForms[] = {
  // exact-fp32 matrix pipe: 32-channel chunks, rows up to 128 columns
  SMI_F_CONV(1, false, 1, 2, false, 4), SMI_F_CONV(2, false, 1, 2, false, 4), SMI_F_CONV(1, true, 1, 2, false, 4), SMI_F_CONV(2, true, 1, 2, false, 4),
  // strided convs: up to 192 staged columns
  SMI_F_CONV(1, false, 1, 3, false, 4), SMI_F_CONV(2, false, 1, 3, false, 4), SMI_F_CONV(1, true, 1, 3, false, 4), SMI_F_CONV(2, true, 1, 3, false, 4),
  // three output tiles per block
  SMI_F_CONV(1, false, 1, 2, false, 3), SMI_F_CONV(2, false, 1, 2, false, 3), SMI_F_CONV(1, false, 1, 3, false, 3), SMI_F_CONV(2, false, 1, 3, false, 3),
  // 1-tap layers: 128-channel chunks
  SMI_F_CONV(1, false, 4, 1, false, 4), SMI_F_CONV(2, false, 4, 1, false, 4), SMI_F_CONV(1, true, 4, 1, false, 4), SMI_F_CONV(2, true, 4, 1, false, 4),
  SMI_F_CONV(1, true, 4, 1, true, 4), SMI_F_CONV(2, true, 4, 1, true, 4),
  // bf16-split matrix pipe: one output tile per wave, 32- / 64- / 128-channel chunks
  SMI_F_CONVB(1, false, 1, 1, false, false), SMI_F_CONVB(1, false, 1, 2, false, false), SMI_F_CONVB(2, false, 1, 2, false, false),
  SMI_F_CONVB(1, false, 2, 2, false, false), SMI_F_CONVB(2, false, 2, 2, false, false),
  SMI_F_CONVB(1, false, 4, 1, false, false), SMI_F_CONVB(2, false, 4, 1, false, false),
  // channel-split: 64-channel chunks (plain and WALL), 128-channel chunks (plain and WPF)
  SMI_F_CONVB(1, true, 2, 1, false, false), SMI_F_CONVB(1, true, 2, 2, false, false), SMI_F_CONVB(2, true, 2, 2, false, false),
  SMI_F_CONVB(1, true, 2, 1, false, true), SMI_F_CONVB(1, true, 2, 2, false, true), SMI_F_CONVB(2, true, 2, 2, false, true),
  SMI_F_CONVB(1, true, 4, 1, false, false), SMI_F_CONVB(2, true, 4, 1, false, false),
  SMI_F_CONVB(1, true, 4, 1, true, false), SMI_F_CONVB(2, true, 4, 1, true, false),
  // transposed convs with 4 / 5 output phases per block
  {{CONV_K_CONVBT, 1, 0, 2, 1, 4, 0, 0, 4}, launch_k_convbT<4>}, {{CONV_K_CONVBT, 1, 0, 2, 1, 4, 0, 0, 5}, launch_k_convbT<5>},
  // one output channel (7 taps); one vector per utterance
  {{CONV_K_C1, 0, 0, 0, 0, 4, 0, 0, 7}, launch_k_conv_c1}, {{CONV_K_GEMV, 0, 0, 0, 0, 4, 0, 0, 0}, launch_k_gemv1},
};
#undef SMI_F_CONV
#undef SMI_F_CONVB
constexpr int kNumConvForms = (int)(sizeof(kConvForms) / sizeof(kConvForms[0]));
}  // namespace

int conv_form_count() { return kNumConvForms; }
const ConvForm& conv_form_at(int index) { return kConvForms[index].form; }
int conv_form_index(const ConvForm& f) {
  for (int i = 0; i < kNumConvForms; ++i)
    if (kConvForms[i].form == f) return i;
  return -1;
}

int run_launch(const Launch& L, hipStream_t st) {
  switch (L.kind) {
    case 0:
      SMI_REQUIRE(L.plan.form >= 0, "%s: no kernel instantiation for this launch plan", L.name.c_str());   // (a list that skipped check_conv)
      kConvForms[L.plan.form].launch(L, st);
      break;
    case 1:
      switch (dwln_form(L.cpt)) {
        case 2: hipLaunchKernelGGL(k_dwln<2>, L.grid, dim3(256), 0, st, L.lp); break;
        case 4: hipLaunchKernelGGL(k_dwln<4>, L.grid, dim3(256), 0, st, L.lp); break;
        case 12: hipLaunchKernelGGL(k_dwln<12>, L.grid, dim3(256), 0, st, L.lp); break;
        case 16: hipLaunchKernelGGL(k_dwln<16>, L.grid, dim3(256), 0, st, L.lp); break;
        default: hipLaunchKernelGGL(k_dwln<32>, L.grid, dim3(256), 0, st, L.lp); break;
      }
      break;
    case 2:
      hipLaunchKernelGGL(k_codebook, L.grid, dim3(128), 0, st, L.sem, L.semstride, L.cb, L.D, L.cbsize, L.lens, L.Z, L.zstride, L.zb);
      break;
    case 3:
      hipLaunchKernelGGL(k_fsq, dim3(L.B), dim3(256), 0, st, L.fp);
      break;
    case 4:
      hipLaunchKernelGGL(k_zero_tail, L.grid, dim3(256), 0, st, L.wav, L.wstride, L.lens, L.hop);
      break;
    case 5:
      if (L.res_nwv == 3) hipLaunchKernelGGL((k_resunit<3>), L.grid, dim3(192), L.lds, st, L.rp);
      else hipLaunchKernelGGL((k_resunit<6>), L.grid, dim3(384), L.lds, st, L.rp);
      break;
    case 9:
      L.fn(st);
      break;
  }
  SMI_LAUNCH_CHECK();
  return SMI_OK;
}

namespace {
bool env_is(const char* name, char v) { const char* e = smi_env(name); return e && e[0] == v; }

// Where k_conv_c1 can stand in for the MFMA kernels: an exact 7-tap stride-1 conv to ONE channel with bias and activation only,
// its weights within 48 KiB of LDS (SPARKMI_VOC_C1=0: never, A/B)
bool c1_eligible(const ConvSpec& s) {
  return !s.bf && s.Cout == 1 && s.S == 1 && s.istr == 1 && s.K == 7 && !s.X2 && !s.bbias && !s.gamma && !s.beta && !s.R && !s.Ys && s.Y &&
         s.out_scale == 1.0f && s.Cin * 7 * 4 <= 48 * 1024 && !env_is("SPARKMI_VOC_C1", '0');
}
}  // namespace

Launch make_conv(const ConvSpec& s) {
  const int Cout = s.Cout, Cin = s.Cin, K = s.K, S = s.S, istr = s.istr;
  const bool bf = s.bf;
  Launch L;
  L.kind = 0; L.name = s.name;
  const ConvGeom g = conv_geom(Cout, Cin, K, s.dil, s.pad, S, bf);
  ConvP& p = L.cp;
  memset(&p, 0, sizeof(p));
  p.X = s.X; p.X2 = s.X2; p.W = s.W; p.bias = s.bias; p.bbias = s.bbias; p.gamma = s.gamma; p.beta = s.beta;
  p.R = s.R; p.alpha = s.alpha; p.Y = s.Y; p.Ys = s.Ys; p.lens = s.lens; p.olens = s.olens;
  p.Cin = Cin; p.CinP = pad8(Cin); p.Cout = Cout; p.S = S; p.act = s.act;
  p.xstride = s.xstride; p.ystride = s.ystride; p.xb = s.xb; p.yb = s.yb;
  p.out_scale = s.out_scale; p.istr = istr; p.halo_l = g.halo_l;
  p.fast_sin = bf && !env_is("SPARKMI_SNAKE_SINF", '1');   // SPARKMI_SNAKE_SINF=1: library sine everywhere (A/B)
  int maxtap = 0;
  double taps = 0;
  for (int r = 0; r < S; ++r) {
    p.ntaps[r] = g.ntaps[r];
    p.wphase[r] = g.wphase[r];
    for (int i = 0; i < g.ntaps[r]; ++i) p.off[r][i] = g.off[r][i];
    maxtap = g.ntaps[r] > maxtap ? g.ntaps[r] : maxtap;
    taps += g.ntaps[r];
  }
  L.flops = 2.0 * Cout * Cin * taps * s.Lmax * s.B;   // all phases together cover S*Lmax outputs
  const int cot = pad32(Cout) / 32;
  // ---- the plan: from here to the grid, (B, Lmax) is the plan shape; (s.B, s.Lmax) stays the extent
  int B = s.B, Lmax = s.Lmax;
  if (s.ps) { B = 1; Lmax = s.ps->len(Lmax); }
  // waves split the input channels when there are few time tiles and many channels
  // 64-column time tiles unless that leaves most CUs idle (short sequences): then 32-column tiles double the blocks
  const long long blocks64 = (long long)((Lmax + 63) / 64) * cot * B * S;
  int qb = (Lmax <= 32 || (blocks64 < 256 && smi_env("SPARKMI_QB2") == nullptr)) ? 1 : 2;
  const int qt = qb * 32, nq = (Lmax + qt - 1) / qt;
  const long long blocks_cosplit = (long long)nq * ((cot + 3) / 4) * B * S;
  // (a partial last group of output tiles just idles its spare waves).  The choice depends on the call's shape
  // (B, longest row): a row is independent of its neighbours and padding bit for bit, and equal to fp32
  // re-association between calls of different shapes.
  const bool ks = blocks_cosplit < 512 && Cin >= 8;
  int xw = (qt - 1) * istr + 1 + g.halo_l + g.halo_r;
  // three-wave blocks where four would leave a wave (and so a SIMD of each CU) without an output tile; measured at
  // 150 frames: 75.0 -> 73.2 ms at B = 32, 21.0 -> 20.5 at B = 8, but 4.66 -> 4.72 at B = 1, hence the grid-size condition
  const int nwv = (!bf && !ks && cot % 3 == 0 && cot % 4 != 0 && blocks_cosplit >= 2048) ? 3 : 4;
  dim3 pg(nq, ks ? cot : (cot + nwv - 1) / nwv, B * S);   // the plan's grid
  int chg = (S == 1 && K == 1 && Cin >= 128 && ks) ? 4 : 1;   // K-split 1-tap layers stage 128 channels per chunk
  if (bf && ks && chg == 1) chg = 2;                          // k_convb: a channel-split wave owns whole 16-channel steps
  // k_convb, one output tile per wave, few taps per phase (1x1 convs: 1; transposed convs: 2-3): a 32-channel chunk carries only
  // 6 * taps MFMAs per wave between its two barriers and its staging round trip.  128-channel chunks where the staged row is one
  // 64-column pass (1 tap), 64-channel chunks up to 128 columns (round 4; SPARKMI_CB_CHG=0: 32-channel chunks everywhere, A/B).
  // A 1-tap layer sums its channels in the same order whatever the chunk; a transposed conv's order goes from (32 channels, taps)
  // to (64 channels, taps) -- the choice depends on the layer's shape only, never on the batch.
  if (bf && !ks && istr == 1 && Cin >= 128 && maxtap <= 3 && !env_is("SPARKMI_CB_CHG", '0')) chg = xw <= 64 ? 4 : (xw <= 128 ? 2 : 1);
  // transposed convs with a grid that still fills the chip with PH phases per block: k_convbT (SPARKMI_CBT=0: off, A/B).  Its
  // epilogue knows bias, the raw output and the Snake'd output only: a residual or an activation keeps the layer on k_convb, and
  // check_conv() refuses a k_convbT launch that asks for any other operand.
  int tph = 0;
  if (bf && !ks && S > 1 && istr == 1 && Cin >= 64 && s.olens == nullptr && !env_is("SPARKMI_CBT", '0')) {
    const int ph = S % 4 == 0 ? 4 : (S == 5 ? 5 : 0);   // (S = 2: two phases x two column tiles measured level with k_convb -- it stays there)
    const int nqt = (Lmax + 31) / 32, xwt = 32 + g.halo_l + g.halo_r;   // one 32-column tile
    // (eight blocks per CU and more: at 900 blocks the stride-5 layer of an 8-row batch lost 0.40 -> 0.48 ms, at 3000+ every layer gained)
    if (ph && (long long)nqt * ((cot + 3) / 4) * B * (S / ph) >= 2048 && xwt <= 64 && !s.R && s.act == ACT_NONE) {
      tph = ph; qb = 1; chg = 2; xw = xwt;
      pg = dim3(nqt, (cot + 3) / 4, B * (S / ph));
    }
  }
  p.xw = xw;
  L.plan_blocks = (long long)pg.x * pg.y * pg.z;
  const bool small = L.plan_blocks <= 512;   // about two blocks per CU: what the WPF / WALL forms are for
  // ---- the kernel form of that plan
  ConvForm f{CONV_K_CONV, qb, 0, 1, 2, 4, 0, 0, 0};
  if (tph) {                    // transposed conv, several output phases per block
    f = ConvForm{CONV_K_CONVBT, 1, 0, 2, 1, 4, 0, 0, tph};
  } else if (bf) {              // bf16-split matrix pipe (k_convb): weights packed as two bf16 planes
    f.kernel = CONV_K_CONVB;
    f.nc = (qb == 1 && xw <= 64) ? 1 : 2;
    if (chg == 4) {
      // one tap, channels split over the waves, at most two blocks per CU: the chunk's weights are requested one chunk ahead (WPF)
      f.chg = 4; f.nc = 1; f.ks = ks; f.wpf = ks && S == 1 && maxtap == 1 && small && !smi_env("SPARKMI_CB_NOWPF");
    } else if (ks) {
      // several taps on a grid of about a block per CU: all taps' weights of a chunk requested together (WALL)
      // (measured at one / two utterances, 150 frames: 7-tap convs 71 -> 62 us at 456 blocks but 101 -> 115 at 912; the first transposed conv,
      // 2 taps per phase, 85 -> 129 us: stride-1 layers with four taps or more on at most two blocks per CU)
      f.ks = 1; f.chg = 2; f.wall = maxtap >= 4 && S == 1 && small && !smi_env("SPARKMI_CB_NOWALL");
    } else if (chg == 2) {      // few taps per phase, rows wider than 64 columns (transposed convs): 64-channel chunks
      f.chg = 2; f.nc = 2;
    }
  } else if (chg == 4) {        // 1-tap layers: 128-channel chunks, narrow rows
    // WPF measured (profiles/README.md): pays up to about two blocks per CU, costs beyond (fewer waves fit)
    f.chg = 4; f.nc = 1; f.ks = ks; f.wpf = ks && small;
  } else {                      // three output tiles per block (never channel-split); strided convs: up to 192 staged columns
    f.nwv = nwv; f.nc = xw > 128 ? 3 : 2; f.ks = ks;
  }
  // ---- what runs: the MFMA form on the extent's grid, or the kernel the caller asked for
  L.grid = s.ps ? dim3((s.Lmax + 32 * qb - 1) / (32 * qb), pg.y, pg.z * s.B) : pg;
  L.blk = 64 * nwv;
  const size_t stage = (size_t)8 * nwv * chg * xw * 4, red = ks ? (size_t)4 * qb * 16 * 64 * 4 : 0;
  L.lds = stage > red ? stage : red;
  bool mfma = true;
  if (s.want == CONV_GEMV) {    // one block per 32 outputs and utterance; anything but an exact 1-tap layer on one position finds no form
    mfma = false;
    f = ConvForm{(!bf && K == 1 && S == 1 && istr == 1 && s.Lmax == 1) ? CONV_K_GEMV : -1, 0, 0, 0, 0, 4, 0, 0, 0};
    L.grid = dim3(cot, s.B); L.blk = 256; L.lds = 0; L.plan_blocks = (long long)cot * B;
  } else if (s.want == CONV_C1 && c1_eligible(s)) {   // a thread per output sample instead of a 32-row MFMA tile with one live row
    mfma = false;
    f = ConvForm{CONV_K_C1, 0, 0, 0, 0, 4, 0, 0, 7};
    L.grid = dim3((s.Lmax + 255) / 256, s.B); L.blk = 256; L.lds = (size_t)Cin * 7 * 4;
  }
  L.plan = ConvPlan{conv_form_index(f), qb, ks, chg, nwv, tph, xw, mfma ? (int)pg.y : 0, mfma && small};
  return L;
}

int check_conv(const Launch& L, const char* who) {
  const ConvP& p = L.cp;
  const ConvPlan& q = L.plan;
  const char* n = L.name.c_str();
  SMI_REQUIRE(p.W, "%s: arena entry for %s not found", who, n);
  SMI_REQUIRE(q.form >= 0, "%s: %s: no kernel instantiation for this launch plan", who, n);
  SMI_REQUIRE(L.lds <= 64 * 1024, "%s: %s needs %zu bytes of LDS", who, n, L.lds);
  // the staging limits: a strided layer (exact pipe) up to 192 columns in 32-channel chunks, else one 64-column pass; every other
  // layer up to 128 columns, a 128-channel chunk one pass
  if (p.istr > 1) SMI_REQUIRE(q.xw <= 192 && (q.chg == 1 || q.xw <= 64), "%s: %s stages %d columns", who, n, q.xw);
  else SMI_REQUIRE(q.xw <= 128 && (q.chg != 4 || q.xw <= 64), "%s: %s stages %d columns", who, n, q.xw);
  if (q.tph) SMI_REQUIRE(!p.bbias && !p.gamma && !p.beta && !p.R && !p.X2 && p.out_scale == 1.0f && p.act == ACT_NONE,
                         "%s: %s: the multi-phase transposed conv has a bias / Snake epilogue only", who, n);
  return SMI_OK;
}

std::vector<long long> plan_signature(const std::vector<Launch>& P) {
  static_assert(sizeof(ConvPlan) % sizeof(int) == 0 && std::is_trivially_copyable<ConvPlan>::value, "the plan record is a row of ints");
  std::vector<long long> sig;
  for (const Launch& L : P) {
    sig.push_back(L.kind);
    if (L.kind == 0) {
      const int* v = (const int*)&L.plan;   // the whole record: every choice made from the plan shape
      sig.insert(sig.end(), v, v + sizeof(ConvPlan) / sizeof(int));
    } else if (L.kind == 5) {
      for (long long v : {(long long)L.res_nwv, (long long)L.rp.xw, (long long)L.lds}) sig.push_back(v);
    } else if (L.kind == 1) {
      sig.push_back(L.cpt);
    }
  }
  return sig;
}

int time_launch(const Launch& L, hipEvent_t ev0, hipEvent_t ev1, int iters, float* ms_avg, double* flops, char* name, int name_cap,
                hipStream_t st) {
  int rc = run_launch(L, st);
  if (rc) return rc;
  SMI_HIP(hipEventRecord(ev0, st));
  for (int i = 0; i < iters; ++i)
    if ((rc = run_launch(L, st))) return rc;
  SMI_HIP(hipEventRecord(ev1, st));
  SMI_HIP(hipEventSynchronize(ev1));
  float ms = 0.f;
  SMI_HIP(hipEventElapsedTime(&ms, ev0, ev1));
  *ms_avg = ms / iters;
  if (flops) *flops = L.flops;
  if (name && name_cap > 0) { strncpy(name, L.name.c_str(), (size_t)name_cap - 1); name[name_cap - 1] = 0; }
  return SMI_OK;
}

}  // namespace smi_net
