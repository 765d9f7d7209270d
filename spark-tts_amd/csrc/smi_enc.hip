// smi_enc.hip -- voice-clone prompt encoder for gfx950 (MI355X): BiCodecTokenizer.tokenize
// (sparktts/models/audio_tokenizer.py:85-130) behind a flat C ABI (include/sparkmi.h, smi_enc_*).
//
//   wav -> zero-mean / unit-variance (Wav2Vec2FeatureExtractor)                 k_wavnorm
//       -> wav2vec2 feature encoder: 7 x [Conv1d(stride) -> LayerNorm -> GELU]  k_conv0 / k_conv(istr) + k_dwln
//       -> LayerNorm -> Linear 512->1024, + GELU(grouped pos-conv k=128)        k_dwln, k_conv, k_posconv
//       -> 16 pre-LN transformer layers (only hidden states 11/14/16 are used)  k_dwln, k_conv, k_mha
//       -> mean of the three tapped hidden states                               k_tap
//   feat -> BiCodec Encoder (Vocos backbone + 2 x [3x, Vocos(2)] + Linear)      k_conv, k_dwln  (feat_encoder.py:76-87)
//        -> in_project, cosine-VQ arg-max over the codebook = semantic ids      k_conv, k_vq    (factorized_vector_quantize.py:148-187)
//   ref clip -> mel (framed DFT as a GEMM, magnitude, slaney filterbank)        k_frames, k_conv, k_mag
//        -> ECAPA-TDNN up to its latent                                         k_conv(ReLU+BN epilogue), k_rowmean, k_gemv1, k_se
//        -> perceiver resampler (2 x [cross-attn incl. queries, GEGLU FF])      k_conv, k_mha, k_geglu, k_rmsn
//        -> FSQ project_in / bound / round = global ids                         k_fsq_quant     (residual_fsq.py:211-276)
//
// Activations are [C][T] fp32 (time contiguous), one utterance per call like the reference's tokenize().
// Dense contractions run on the exact-fp32 matrix pipe through the vocoder's implicit-GEMM kernel
// (smi_net.hip); attention and the 128-tap grouped positional conv are VALU kernels (small: T <= ~1500).
#include "smi_net.h"
#include <math.h>
#include <algorithm>
#include <map>

using namespace smi_net;

namespace {

// ------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------

// Every kernel below carries a row dimension: block z is row b of the launch, the row's lengths come from device arrays indexed by
// b (one per length kind) and its buffers sit b batch strides on.  A row's arithmetic depends on its own lengths only and blocks
// beyond a row's own extent exit without writing, so a row of a ragged launch carries the bits of its solo launch (the same
// kernels over one row: smi_enc_forward's list).

// (x - mean) / sqrt(var + 1e-7), feature_extraction_wav2vec2.py zero_mean_unit_var_norm; one block per row.
__global__ __launch_bounds__(1024) void k_wavnorm(const float* x, long long xbs, const int* ns, float* y, long long ybs) {
  __shared__ double red[1024];
  const int tid = threadIdx.x, n = ns[blockIdx.z];
  x += blockIdx.z * xbs; y += blockIdx.z * ybs;
  double s = 0.0;
  for (int i = tid; i < n; i += 1024) s += (double)x[i];
  red[tid] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
  const double mean = red[0] / n;
  __syncthreads();
  double q = 0.0;
  for (int i = tid; i < n; i += 1024) { const double d = (double)x[i] - mean; q += d * d; }
  red[tid] = q;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
  const float fm = (float)mean;
  const float rs = 1.0f / sqrtf((float)(red[0] / n) + 1e-7f);
  for (int i = tid; i < n; i += 1024) y[i] = (x[i] - fm) * rs;
}

// first feature-encoder conv: Conv1d(1 -> C, K, stride), no padding.  W [C][K].
__global__ void k_conv0(const float* x, const float* W, const float* bias, int K, int stride, float* Y, int C, const int* Ts, int ystride,
                        long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (t >= Ts[blockIdx.z]) return;
  x += blockIdx.z * bs; Y += blockIdx.z * bs;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc += W[c * K + k] * x[t * stride + k];
  Y[(long long)c * ystride + t] = acc + (bias ? bias[c] : 0.f);
}

// grouped positional conv (Wav2Vec2PositionalConvEmbedding): out[c][t] = x[c][t] + gelu(b[c] +
//   sum_{ci < Cg, k < K} W[c][ci][k] * x[g*Cg + ci][t + k - K/2]);  the SamePad layer drops the extra last frame.
// Block = 16 output channels of one group x 64 frames; wave w computes channels 4w..4w+3 (weights wave-uniform).
__global__ __launch_bounds__(256) void k_posconv(const float* X, const float* W, const float* bias, float* Y, int C, int Cg, int K,
                                                 const int* Ts, int stride, long long bs) {
  extern __shared__ float xs[];            // [Cg][64 + K - 1]
  const int t0 = blockIdx.x * 64, cot = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = Ts[blockIdx.z];
  if (t0 >= T) return;                     // (a block beyond the row: the launch covers the longest row)
  X += blockIdx.z * bs; Y += blockIdx.z * bs;
  const int co0 = cot * 16 + wave * 4, g = (cot * 16) / Cg;
  const int xw = 64 + K - 1;
  for (int i = threadIdx.x; i < Cg * xw; i += 256) {
    const int ci = i / xw, col = i - ci * xw, t = t0 + col - K / 2;
    xs[i] = (t >= 0 && t < T) ? X[(long long)(g * Cg + ci) * stride + t] : 0.f;
  }
  __syncthreads();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* w0 = W + (long long)co0 * Cg * K;
  for (int ci = 0; ci < Cg; ++ci) {
    const float* xr = xs + ci * xw + lane;
    for (int k = 0; k < K; ++k) {
      const float xv = xr[k];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] += w0[((long long)c * Cg + ci) * K + k] * xv;
    }
  }
  const int t = t0 + lane;
  if (t < T) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long o = (long long)(co0 + c) * stride + t;
      Y[o] = X[o] + gelu_f(acc[c] + bias[co0 + c]);
    }
  }
}

// Multi-head attention, head_dim 64, no mask: O[h*64+d][q] = sum_j softmax_j(scale * Q[:,q].K[:,j]) V[h*64+d][j].
// Q/K/V/O are channel-major [rows][stride].  Block = (8 queries, head); scores of the 8 rows live in LDS.
struct MhaP {
  const float *Q, *K, *V;
  float* O;
  int qs, ks, vs, os;   // row strides
  int Tq, Tk;           // (set by the kernel from the two arrays)
  float scale;
  const int *Tqs, *Tks; // [rows] queries / keys of each row
  long long bs;         // batch stride of the four buffers
};
__global__ __launch_bounds__(256) void k_mha(MhaP p) {
  extern __shared__ float sm[];
  p.Tq = p.Tqs[blockIdx.z]; p.Tk = p.Tks[blockIdx.z];
  if ((int)blockIdx.x * 8 >= p.Tq) return;
  p.Q += blockIdx.z * p.bs; p.K += blockIdx.z * p.bs; p.V += blockIdx.z * p.bs; p.O += blockIdx.z * p.bs;
  float* qs = sm;                       // [64][8]
  float* S = sm + 512;                  // [8][Tk]
  float* Vs = S + 8 * p.Tk;             // [64][65]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * 8, h = blockIdx.y;
  const float* Qh = p.Q + (long long)h * 64 * p.qs;
  const float* Kh = p.K + (long long)h * 64 * p.ks;
  const float* Vh = p.V + (long long)h * 64 * p.vs;
  for (int i = tid; i < 512; i += 256) {
    const int d = i >> 3, qi = i & 7;
    qs[i] = (q0 + qi < p.Tq) ? Qh[(long long)d * p.qs + q0 + qi] : 0.f;
  }
  __syncthreads();
  for (int j = tid; j < p.Tk; j += 256) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < 64; ++d) {
      const float kv = Kh[(long long)d * p.ks + j];
#pragma unroll
      for (int qi = 0; qi < 8; ++qi) acc[qi] += qs[d * 8 + qi] * kv;
    }
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) S[qi * p.Tk + j] = acc[qi] * p.scale;
  }
  __syncthreads();
  // softmax: wave w owns rows 2w, 2w+1
  for (int r = wave * 2; r < wave * 2 + 2; ++r) {
    float* row = S + r * p.Tk;
    float m = -INFINITY;
    for (int j = lane; j < p.Tk; j += 64) m = fmaxf(m, row[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    for (int j = lane; j < p.Tk; j += 64) { const float e = expf(row[j] - m); row[j] = e; s += e; }
    s = smi_wave_sum(s);
    const float inv = 1.0f / s;
    for (int j = lane; j < p.Tk; j += 64) row[j] *= inv;
  }
  __syncthreads();
  // O = P V: thread (d = lane, rows 2*wave, 2*wave+1); V staged 64 keys at a time
  float o0 = 0.f, o1 = 0.f;
  const float* P0 = S + (wave * 2) * p.Tk;
  const float* P1 = P0 + p.Tk;
  for (int j0 = 0; j0 < p.Tk; j0 += 64) {
    for (int i = tid; i < 64 * 64; i += 256) {
      const int d = i >> 6, jj = i & 63;
      Vs[d * 65 + jj] = (j0 + jj < p.Tk) ? Vh[(long long)d * p.vs + j0 + jj] : 0.f;
    }
    __syncthreads();
    const int n = p.Tk - j0 < 64 ? p.Tk - j0 : 64;
    for (int jj = 0; jj < n; ++jj) {
      const float v = Vs[lane * 65 + jj];
      o0 += P0[j0 + jj] * v;
      o1 += P1[j0 + jj] * v;
    }
    __syncthreads();
  }
  float* Oh = p.O + (long long)h * 64 * p.os;
  const int qa = q0 + wave * 2;
  if (qa < p.Tq) Oh[(long long)lane * p.os + qa] = o0;
  if (qa + 1 < p.Tq) Oh[(long long)lane * p.os + qa + 1] = o1;
}

// hidden-state taps: mode 0: acc = h; 1: acc = acc + h; 2: out = (acc + h) / 3   (audio_tokenizer.py:96-98)
// [Hd][stride] per row, indexed by (channel, frame) -- a row's own T is not its stride
__global__ void k_tap(const float* h, float* acc, float* out, const int* Ts, int stride, long long bs, int mode) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Ts[blockIdx.z]) return;
  const long long i = blockIdx.z * bs + (long long)blockIdx.y * stride + t;
  if (mode == 0) acc[i] = h[i];
  else if (mode == 1) acc[i] = acc[i] + h[i];
  else out[i] = (acc[i] + h[i]) / 3.0f;
}

// framed, reflect-padded reference clip: F[k][t] = xpad[t*hop + k], xpad = reflect pad of n_fft/2 (torch.stft center=True)
__global__ void k_frames(const float* x, long long xbs, const int* ns, int n_fft, int hop, float* F, const int* Ts, int stride, long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (t >= Ts[blockIdx.z]) return;
  const int n = ns[blockIdx.z];
  x += blockIdx.z * xbs; F += blockIdx.z * bs;
  int i = t * hop + k - n_fft / 2;
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  F[(long long)k * stride + t] = x[i];
}

// |re + i im| of the DFT rows: D [2*nf][stride] (re rows then im rows) -> M [nf][stride]
__global__ void k_mag(const float* D, int nf, const int* Ts, int stride, float* M, long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (t >= Ts[blockIdx.z]) return;
  D += blockIdx.z * bs; M += blockIdx.z * bs;
  const float re = D[(long long)f * stride + t], im = D[(long long)(nf + f) * stride + t];
  M[(long long)f * stride + t] = sqrtf(re * re + im * im);
}

// mean over time of every channel (SE_Connect, ecapa_tdnn.py:104): one wave per channel
__global__ __launch_bounds__(256) void k_rowmean(const float* X, int C, const int* Ts, int stride, float* out, long long bs) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  const int T = Ts[blockIdx.z];
  X += blockIdx.z * bs; out += blockIdx.z * bs;
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += X[(long long)c * stride + t];
  s = smi_wave_sum(s);
  if (lane == 0) out[c] = s / (float)T;
}

// SE_Res2Block tail: out[c][t] = xin[c][t] + y[c][t] * s[c]   (ecapa_tdnn.py:107,133)
__global__ void k_se(const float* xin, const float* y, const float* s, float* out, const int* Ts, int istride, int ostride, long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (t >= Ts[blockIdx.z]) return;
  xin += blockIdx.z * bs; y += blockIdx.z * bs; s += blockIdx.z * bs; out += blockIdx.z * bs;
  out[(long long)c * ostride + t] = xin[(long long)c * istride + t] + y[(long long)c * istride + t] * s[c];
}

// GEGLU (perceiver_encoder.py:213-216): Y[c][t] = gelu(X[inner + c][t]) * X[c][t]
__global__ void k_geglu(const float* X, int inner, int T, int stride, float* Y, long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (t >= T) return;
  X += blockIdx.z * bs; Y += blockIdx.z * bs;
  Y[(long long)c * stride + t] = gelu_f(X[(long long)(inner + c) * stride + t]) * X[(long long)c * stride + t];
}

// perceiver RMSNorm over channels of T columns: x / max(||x||, 1e-12) * sqrt(C) * gamma (perceiver_encoder.py:180-191)
__global__ void k_rmsn(const float* X, int C, int T, int stride, const float* gamma, float* Y, int ystride, long long bs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  X += blockIdx.z * bs; Y += blockIdx.z * bs;
  float ss = 0.f;
  for (int c = 0; c < C; ++c) { const float v = X[(long long)c * stride + t]; ss += v * v; }
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  const float sc = sqrtf((float)C);
  for (int c = 0; c < C; ++c) Y[(long long)c * ystride + t] = X[(long long)c * stride + t] / nrm * sc * gamma[c];
}

// codebook rows L2-normalised once at create (F.normalize(codebook), factorized_vector_quantize.py:176)
__global__ void k_cbnorm(const float* cb, int n, int D, float* out, float* c2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ss = 0.f;
  for (int d = 0; d < D; ++d) ss += cb[i * D + d] * cb[i * D + d];
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  float s2 = 0.f;
  for (int d = 0; d < D; ++d) { const float v = cb[i * D + d] / nrm; out[i * D + d] = v; s2 += v * v; }
  c2[i] = s2;
}

// cosine-VQ arg-max of one frame per block: -(|e|^2 - 2 e.c + |c|^2), lowest index on ties (torch .max(1)[1])
__global__ __launch_bounds__(256) void k_vq(const float* Ze, int D, const int* Ts, int stride, long long bs, const float* cbn, const float* c2,
                                            int ncode, int64_t* sem, long long sem_bs) {
  __shared__ float bv[256];
  __shared__ int bi[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  if (t >= Ts[blockIdx.z]) return;
  Ze += blockIdx.z * bs; sem += blockIdx.z * sem_bs;
  float e[16];
  float ss = 0.f;
  for (int d = 0; d < D; ++d) { e[d] = Ze[(long long)d * stride + t]; ss += e[d] * e[d]; }
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  float e2 = 0.f;
  for (int d = 0; d < D; ++d) { e[d] = e[d] / nrm; e2 += e[d] * e[d]; }
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int i = tid; i < ncode; i += 256) {
    float dot = 0.f;
    for (int d = 0; d < D; ++d) dot += e[d] * cbn[i * D + d];
    const float v = -((e2 - 2.0f * dot) + c2[i]);
    if (v > best) { best = v; besti = i; }
  }
  bv[tid] = best; bi[tid] = besti;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      if (bv[tid + o] > bv[tid] || (bv[tid + o] == bv[tid] && bi[tid + o] < bi[tid])) { bv[tid] = bv[tid + o]; bi[tid] = bi[tid + o]; }
    }
    __syncthreads();
  }
  if (tid == 0) sem[t] = bi[0];
}

// FSQ: z = W x + b; bounded = tanh(z + shift) * half_l - offset; round (half to even, torch.round); index
// (finite_scalar_quantization.py:113-137, residual_fsq.py:211-276 with one quantizer)
struct FsqQP {
  const float* X;     // [latent][stride]
  const float* W;     // [nd][latent]
  const float* b;     // [nd]
  int32_t* out;       // [Ntok]
  float* bounded;     // [Ntok][nd] (debug) or null
  int latent, stride, Ntok, nd;
  int levels[8];
  long long bs, obs;  // batch strides of X and bounded, of out
};
__global__ void k_fsq_quant(FsqQP p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.Ntok) return;
  p.X += blockIdx.z * p.bs; p.out += blockIdx.z * p.obs;
  if (p.bounded) p.bounded += blockIdx.z * p.bs;
  int idx = 0, basis = 1;
  for (int j = 0; j < p.nd; ++j) {
    float z = 0.f;
    for (int d = 0; d < p.latent; ++d) z += p.W[j * p.latent + d] * p.X[(long long)d * p.stride + t];
    z += p.b[j];
    const int L = p.levels[j];
    const float half_l = (float)(L - 1) * (1.0f + 1e-3f) / 2.0f;
    const float offset = (L % 2 == 0) ? 0.5f : 0.0f;
    const float shift = atanhf(offset / half_l);
    const float bd = tanhf(z + shift) * half_l - offset;
    if (p.bounded) p.bounded[t * p.nd + j] = bd;
    const float q = rintf(bd);
    const int half_w = L / 2;
    idx += ((int)q + half_w) * basis;
    basis *= L;
  }
  p.out[t] = idx;
}

__global__ void k_copy2d(const float* src, int sstride, long long sbs, float* dst, int dstride, long long dbs, int rows, const int* cols) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (t < cols[blockIdx.z] && r < rows) dst[blockIdx.z * dbs + (long long)r * dstride + t] = src[blockIdx.z * sbs + (long long)r * sstride + t];
}

// ------------------------------------------------------------------------------------------
// layout
// ------------------------------------------------------------------------------------------
struct EncLayout {
  std::vector<Entry> e;
  size_t total;
};

constexpr int kMaxKeys = 2040;        // k_mha: 8 score rows of Tk floats + the Q and V tiles within the 96 KB dynamic LDS window
constexpr int kMaxSpkTokens = 1024;   // k_geglu's block

bool enc_cfg_ok(const smi_enc_cfg* c) {
  if (!c) return false;
  if (c->w2v_nconv < 2 || c->w2v_nconv > 8 || c->w2v_conv_dim < 32 || c->w2v_conv_dim % 32 || c->w2v_conv_dim > 1024) return false;
  for (int i = 0; i < c->w2v_nconv; ++i)
    if (c->w2v_kernel[i] < 1 || c->w2v_stride[i] < 1 || (i > 0 && (c->w2v_kernel[i] > kMaxTaps || c->w2v_stride[i] > 2))) return false;
  if (c->w2v_hidden % 64 || c->w2v_hidden != c->w2v_heads * 64 || c->w2v_hidden > 1024 || c->w2v_layers < 1) return false;
  if (c->w2v_pos_k < 2 || c->w2v_pos_k % 2 || c->w2v_pos_groups < 1 || c->w2v_hidden % c->w2v_pos_groups) return false;
  if ((c->w2v_hidden / c->w2v_pos_groups) % 16) return false;
  for (int i = 0; i < 3; ++i) if (c->w2v_taps[i] < 0 || c->w2v_taps[i] > c->w2v_layers) return false;
  if (c->enc_in != c->w2v_hidden || c->enc_dim < 1 || c->enc_dim > 1024 || c->enc_layers < 1 || c->enc_num_down < 0) return false;
  if (c->codebook_dim < 1 || c->codebook_dim > 16 || c->codebook_size < 1) return false;
  if (c->n_fft < 16 || c->n_fft % 2 || c->win_length > c->n_fft || c->hop_length < 1 || c->num_mels < 1) return false;
  // k_geglu runs one block of 64 * ceil(spk_tokens / 64) threads per channel: at most 1024 threads
  if (c->ecapa_channels % 64 || c->ecapa_channels < 64 || c->spk_latent < 1 || c->spk_tokens < 1 || c->spk_tokens > kMaxSpkTokens) return false;
  if (c->fsq_dims < 1 || c->fsq_dims > 8 || c->perc_depth < 1 || c->perc_heads < 1 || c->perc_ff_inner < 1) return false;
  if (c->max_samples < 400 || c->max_ref_samples < c->n_fft) return false;
  return true;
}

EncLayout enc_layout(const smi_enc_cfg* c) {
  EncLayout L;
  size_t o = 0;
  auto add = [&](const std::string& name, int kind, int Cout, int Cin, int K, size_t floats) {
    Entry e{name, kind, Cout, Cin, K, 1, 0, o, floats * 4};
    L.e.push_back(e);
    o += smi_align_up(floats * 4, 256);
  };
  auto raw = [&](const std::string& name, size_t n) { add(name, PACK_RAW, 0, 0, 0, n); };
  auto conv = [&](const std::string& name, int Cout, int Cin, int K) {
    add(name, PACK_CONV, Cout, Cin, K, (size_t)conv_geom(Cout, Cin, K, 1, 0, 1).floats);
  };
  // convb: the dense stride-1 layers that carry the FLOPs (wav2vec2's transformer projections, the BiCodec encoder's
  // ConvNeXt stack) -- on the bf16-split matrix pipe (k_convb, smi_net.hip) unless the handle asks for exact fp32
  auto convb = [&](const std::string& name, int Cout, int Cin, int K) {
    const bool bf = !c->exact_fp32 && Cin >= 32 && Cout >= 32;
    add(name, bf ? PACK_CONV_B : PACK_CONV, Cout, Cin, K, (size_t)conv_geom(Cout, Cin, K, 1, 0, 1, bf).floats);
  };
  // ---- wav2vec2
  const int CD = c->w2v_conv_dim, H = c->w2v_hidden, I = c->w2v_inter;
  for (int i = 0; i < c->w2v_nconv; ++i) {
    const std::string p = "w2v.feature_extractor.conv_layers." + std::to_string(i);
    if (i == 0) raw(p + ".conv.weight", (size_t)CD * c->w2v_kernel[0]);
    else conv(p + ".conv.weight", CD, CD, c->w2v_kernel[i]);
    raw(p + ".conv.bias", CD);
    raw(p + ".layer_norm.weight", CD);
    raw(p + ".layer_norm.bias", CD);
  }
  raw("w2v.feature_projection.layer_norm.weight", CD);
  raw("w2v.feature_projection.layer_norm.bias", CD);
  conv("w2v.feature_projection.projection.weight", H, CD, 1);
  raw("w2v.feature_projection.projection.bias", H);
  raw("w2v.encoder.pos_conv_embed.conv.weight", (size_t)H * (H / c->w2v_pos_groups) * c->w2v_pos_k);
  raw("w2v.encoder.pos_conv_embed.conv.bias", H);
  for (int l = 0; l < c->w2v_layers; ++l) {
    const std::string p = "w2v.encoder.layers." + std::to_string(l);
    raw(p + ".layer_norm.weight", H);
    raw(p + ".layer_norm.bias", H);
    convb("cat:" + p + ".attention.q_proj.weight|" + p + ".attention.k_proj.weight|" + p + ".attention.v_proj.weight", 3 * H, H, 1);
    raw("cat:" + p + ".attention.q_proj.bias|" + p + ".attention.k_proj.bias|" + p + ".attention.v_proj.bias", (size_t)3 * H);
    convb(p + ".attention.out_proj.weight", H, H, 1);
    raw(p + ".attention.out_proj.bias", H);
    raw(p + ".final_layer_norm.weight", H);
    raw(p + ".final_layer_norm.bias", H);
    convb(p + ".feed_forward.intermediate_dense.weight", I, H, 1);
    raw(p + ".feed_forward.intermediate_dense.bias", I);
    convb(p + ".feed_forward.output_dense.weight", H, I, 1);
    raw(p + ".feed_forward.output_dense.bias", H);
  }
  // ---- BiCodec encoder + quantizer
  const int D = c->enc_dim, EI = c->enc_inter;
  auto vocos = [&](const std::string& p, int cin, int nl) {
    convb(p + ".embed.weight", D, cin, 7);
    raw(p + ".embed.bias", D);
    raw(p + ".norm.weight", D);
    raw(p + ".norm.bias", D);
    for (int j = 0; j < nl; ++j) {
      const std::string b = p + ".convnext." + std::to_string(j);
      raw(b + ".dwconv.weight", (size_t)D * 7);
      raw(b + ".dwconv.bias", D);
      raw(b + ".norm.weight", D);
      raw(b + ".norm.bias", D);
      convb(b + ".pwconv1.weight", EI, D, 1);
      raw(b + ".pwconv1.bias", EI);
      convb(b + ".pwconv2.weight", D, EI, 1);
      raw(b + ".pwconv2.bias", D);
      raw(b + ".gamma", D);
    }
    raw(p + ".final_layer_norm.weight", D);
    raw(p + ".final_layer_norm.bias", D);
  };
  vocos("encoder.encoder", c->enc_in, c->enc_layers);
  for (int i = 0; i < c->enc_num_down; ++i) vocos("encoder.downsample." + std::to_string(i) + ".1", D, 2);
  conv("encoder.project.weight", c->enc_out, D, 1);
  raw("encoder.project.bias", c->enc_out);
  conv("quantizer.in_project.weight", c->codebook_dim, c->enc_out, 1);
  raw("quantizer.in_project.bias", c->codebook_dim);
  raw("quantizer.codebook.weight", (size_t)c->codebook_size * c->codebook_dim);
  // ---- mel (derived on the host)
  const int nf = c->n_fft / 2 + 1;
  conv("mel.dft", 2 * nf, c->n_fft, 1);
  conv("mel.fb", c->num_mels, nf, 1);
  // ---- ECAPA-TDNN up to `latent`
  const int C = c->ecapa_channels, W = C / 8;
  const std::string se = "speaker_encoder.speaker_encoder";
  auto crb = [&](const std::string& p, int co, int ci, int k) {
    conv(p + ".conv.weight", co, ci, k);
    raw(p + ".conv.bias", co);
    raw("bnscale:" + p + ".bn", co);
    raw("bnshift:" + p + ".bn", co);
  };
  crb(se + ".layer1", C, c->num_mels, 5);
  for (int li = 2; li <= 4; ++li) {
    const std::string b = se + ".layer" + std::to_string(li) + ".se_res2block";
    crb(b + ".0", C, C, 1);
    for (int j = 0; j < 7; ++j) {
      conv(b + ".1.convs." + std::to_string(j) + ".weight", W, W, 3);
      raw(b + ".1.convs." + std::to_string(j) + ".bias", W);
      raw("bnscale:" + b + ".1.bns." + std::to_string(j), W);
      raw("bnshift:" + b + ".1.bns." + std::to_string(j), W);
    }
    crb(b + ".2", C, C, 1);
    conv(b + ".3.linear1.weight", 128, C, 1);
    raw(b + ".3.linear1.bias", 128);
    conv(b + ".3.linear2.weight", C, 128, 1);
    raw(b + ".3.linear2.bias", C);
  }
  conv(se + ".conv.weight", c->ecapa_out, 3 * C, 1);
  raw(se + ".conv.bias", c->ecapa_out);
  // ---- perceiver + FSQ
  const std::string ps = "speaker_encoder.perceiver_sampler";
  const int Ld = c->spk_latent, inner = c->perc_heads * 64, FI = c->perc_ff_inner;
  conv(ps + ".proj_context.weight", Ld, c->ecapa_out, 1);
  raw(ps + ".proj_context.bias", Ld);
  raw("transpose:" + ps + ".latents", (size_t)Ld * c->spk_tokens);
  for (int i = 0; i < c->perc_depth; ++i) {
    const std::string a = ps + ".layers." + std::to_string(i) + ".0", f = ps + ".layers." + std::to_string(i) + ".1";
    conv(a + ".to_q.weight", inner, Ld, 1);
    conv(a + ".to_kv.weight", 2 * inner, Ld, 1);
    conv(a + ".to_out.weight", Ld, inner, 1);
    conv(f + ".0.weight", 2 * FI, Ld, 1);
    raw(f + ".0.bias", (size_t)2 * FI);
    conv(f + ".2.weight", Ld, FI, 1);
    raw(f + ".2.bias", Ld);
  }
  raw(ps + ".norm.gamma", Ld);
  raw("speaker_encoder.quantizer.project_in.weight", (size_t)c->fsq_dims * Ld);
  raw("speaker_encoder.quantizer.project_in.bias", c->fsq_dims);
  L.total = o;
  return L;
}

int conv_out_len(int n, int k, int s) { return n < k ? 0 : (n - k) / s + 1; }

// every working buffer of an encode of up to max_samples / max_ref_samples (floats): one row's slab of a workspace
std::map<std::string, size_t> enc_buffers(const smi_enc_cfg& c, int max_samples, int max_ref_samples) {
  std::map<std::string, size_t> out;
  // frame counts at the longest input
  int n = max_samples;
  std::vector<int> Ts;
  for (int i = 0; i < c.w2v_nconv; ++i) { n = conv_out_len(n, c.w2v_kernel[i], c.w2v_stride[i]); Ts.push_back(n); }
  const int T0 = Ts[0] + 8, T = Ts.back() + 8;
  const int Tm = max_ref_samples / c.hop_length + 1 + 8;
  const int nf = c.n_fft / 2 + 1;
  auto want = [&](const std::string& name, size_t floats) { out[name] = floats; };
  want("wavn", (size_t)max_samples + 64);
  want("cf0", (size_t)c.w2v_conv_dim * T0);
  want("cf1", (size_t)c.w2v_conv_dim * T0);
  const int Hh = c.w2v_hidden;
  const int wide = c.w2v_inter > 3 * Hh ? c.w2v_inter : 3 * Hh;
  want("h", (size_t)Hh * T);
  want("x", (size_t)Hh * T);
  want("wide", (size_t)wide * T);
  want("att", (size_t)Hh * T);
  want("acc", (size_t)Hh * T);
  want("feat", (size_t)Hh * T);
  want("dbg_hs0", (size_t)Hh * T);
  const int D = c.enc_dim;
  const int ew = c.enc_inter > c.enc_out ? c.enc_inter : c.enc_out;
  want("e0", (size_t)(D > c.codebook_dim ? D : c.codebook_dim) * T);
  want("e1", (size_t)D * T);
  want("e2", (size_t)D * T);
  want("ew", (size_t)ew * T);
  want("frames", (size_t)c.n_fft * Tm);
  want("dft", (size_t)2 * nf * Tm);
  want("mag", (size_t)nf * Tm);
  want("mel", (size_t)c.num_mels * Tm);
  const int C = c.ecapa_channels;
  want("ec_a", (size_t)C * Tm);
  want("ec_b", (size_t)C * Tm);
  want("ec_c", (size_t)C * Tm);
  want("ec_cat", (size_t)3 * C * Tm);
  want("ec_lat", (size_t)c.ecapa_out * Tm);
  want("ec_vec", (size_t)4 * (C + 128));
  const int Tc = c.spk_tokens + Tm;
  const int inner = c.perc_heads * 64;
  want("pctx", (size_t)c.spk_latent * Tc);
  want("pq", (size_t)inner * c.spk_tokens);
  want("pkv", (size_t)2 * inner * Tc);
  want("po", (size_t)inner * c.spk_tokens);
  want("pff", (size_t)2 * c.perc_ff_inner * c.spk_tokens);
  want("pg", (size_t)c.perc_ff_inner * c.spk_tokens);
  want("pout", (size_t)c.spk_latent * c.spk_tokens);
  want("fsqb", (size_t)c.spk_tokens * 8);
  want("in_wav", (size_t)max_samples + 64);
  want("in_ref", (size_t)max_ref_samples + 64);
  want("out_sem", (size_t)2 * T);           // int64 ids
  want("out_glob", (size_t)c.spk_tokens + 64);
  return out;
}

// Every length a launch reads, by kind: the feature encoder's layer outputs (the last is T, the frame count), the two inputs,
// mel frames Tm, perceiver keys Tk = Nt + Tm, and the two constants the vector projections and the latent-side layers use.
enum { LK_T0 = 0 /* .. LK_T0 + 7 */, LK_NS = 8, LK_NREF = 9, LK_TM = 10, LK_TK = 11, LK_ONE = 12, LK_NT = 13, LK_COUNT = 14 };
struct RowLens { int v[LK_COUNT]; };

}  // namespace

struct smi_enc {
  smi_enc_cfg cfg;
  EncLayout lay;
  const unsigned char* arena;
  DevBuf<float> cbn, c2;                    // normalised codebook, |c|^2
  struct Stage { const float* ptr; int rows, cols, stride; };
  // A workspace: max_rows slabs, a slab holding every working buffer of one row (enc_buffers) at `off`, the rows' lengths by
  // kind, and the launch list last built on it with its debug views.  The handle has two: `solo` (one row of the config's own
  // limits, allocated at create; smi_enc_forward and its graphs) and `rows` (smi_enc_rows_reserve; smi_enc_forward_rows).
  struct Ws {
    int max_rows = 0, max_samples = 0, max_ref = 0;
    DevBuf<float> ws;
    long long slab = 0;                     // floats per row: the one batch stride of every buffer
    std::map<std::string, size_t> off, floats;
    DevBuf<int> lens_dev;                   // [length kind][max_rows]
    std::vector<int32_t> host_lens;
    std::vector<Launch> prog;
    std::vector<int> run_start;             // first row of every run of the last list
    std::vector<std::map<std::string, Stage>> stages;   // per row: debug views of the last list
    int lastB = 0;
    float* at(int row, const char* name) const { return ws + row * slab + off.at(name); }
  } solo, rows;
  std::map<std::pair<int, int>, std::vector<long long>> sigs;   // (n_samples, n_ref) -> the plan signature of that row's one-row list
  int last_frames;
  hipEvent_t ev0, ev1;
  // One hipGraph per (n_samples, n_ref): the ~260 launches of an encode replayed as one graph launch.  The graph reads the
  // prompt from / leaves the ids in handle-owned buffers (in_wav, in_ref, out_sem, out_glob of the solo workspace), so it does
  // not depend on the caller's pointers; the row's lengths are uploaded before every launch (they differ from key to key).
  struct Graph {
    hipGraphExec_t exec = nullptr;
    std::vector<int32_t> lens;
    std::vector<Launch> prog;
    std::vector<std::map<std::string, Stage>> stages;
    int frames = 0;
    unsigned long long used = 0;
    hipStream_t last = nullptr; bool launched = false;   // the stream of its last launch: synchronised before the exec is destroyed
  };
  std::map<std::pair<int, int>, Graph> graphs;
  std::map<std::pair<int, int>, int> seen;   // a shape is captured at its second occurrence: traffic whose shapes never repeat runs eagerly
  std::pair<int, int> prog_key{-1, -1};
  unsigned long long tick = 0;
  bool use_graph = true;
  hipStream_t gstream = nullptr;            // graph launches of callers on the null stream (which cannot be captured) run here
  hipEvent_t gev0 = nullptr, gev1 = nullptr;
};

namespace {

const float* ent(const smi_enc* h, const std::string& name) {
  for (const Entry& e : h->lay.e)
    if (e.name == name) return (const float*)(h->arena + e.offset);
  return nullptr;
}
bool ent_is_bf(const smi_enc* h, const std::string& name) {
  for (const Entry& e : h->lay.e)
    if (e.name == name) return e.kind == PACK_CONV_B || e.kind == PACK_CONVT_B;
  return false;
}

// W becomes a workspace of max_rows rows of up to max_samples / max_ref; what it held is freed first.  On failure W is empty.
int ws_alloc(const smi_enc_cfg& c, smi_enc::Ws& W, const char* who, int max_rows, int max_samples, int max_ref) {
  W = smi_enc::Ws();
  W.floats = enc_buffers(c, max_samples, max_ref);
  size_t o = 0;
  for (const auto& kv : W.floats) { W.off[kv.first] = o; o += smi_align_up(kv.second, 64); }
  W.slab = (long long)o;
  if (W.ws.alloc((size_t)max_rows * o * 4, who) || W.lens_dev.alloc((size_t)LK_COUNT * max_rows * 4, who)) {
    W = smi_enc::Ws();
    return SMI_EHIP;
  }
  W.max_rows = max_rows; W.max_samples = max_samples; W.max_ref = max_ref;
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_enc_arena_count(const smi_enc_cfg* cfg) {
  if (!enc_cfg_ok(cfg)) { smi_set_error("smi_enc_arena_count: invalid config"); return SMI_EINVAL; }
  return (int)enc_layout(cfg).e.size();
}

size_t smi_enc_arena_bytes(const smi_enc_cfg* cfg) {
  if (!enc_cfg_ok(cfg)) return 0;
  return enc_layout(cfg).total;
}

int smi_enc_arena_entry(const smi_enc_cfg* cfg, int index, char* name, int name_cap, size_t* offset, size_t* bytes, int32_t* info) {
  SMI_REQUIRE(enc_cfg_ok(cfg), "smi_enc_arena_entry: invalid config");
  EncLayout L = enc_layout(cfg);
  SMI_REQUIRE(index >= 0 && index < (int)L.e.size(), "smi_enc_arena_entry: index %d out of range", index);
  const Entry& e = L.e[index];
  if (name && name_cap > 0) {
    SMI_REQUIRE((int)e.name.size() < name_cap, "smi_enc_arena_entry: name buffer too small (%zu needed)", e.name.size() + 1);
    strncpy(name, e.name.c_str(), (size_t)name_cap - 1); name[name_cap - 1] = 0;
  }
  if (offset) *offset = e.offset;
  if (bytes) *bytes = e.bytes;
  if (info) { info[0] = e.kind; info[1] = e.Cout; info[2] = e.Cin; info[3] = e.K; info[4] = e.S; info[5] = e.pad; }
  return SMI_OK;
}

int smi_enc_create(const smi_enc_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_enc** out) {
  SMI_REQUIRE(out, "smi_enc_create: null out");
  *out = nullptr;
  SMI_REQUIRE(enc_cfg_ok(cfg), "smi_enc_create: invalid or unsupported config");
  SMI_REQUIRE(arena_dev, "smi_enc_create: null arena");
  char arch[128];
  int rc = smi_device_check(arch, sizeof(arch));
  if (rc) return rc;
  smi_enc* h = new smi_enc();
  h->cfg = *cfg;
  h->lay = enc_layout(cfg);
  h->arena = (const unsigned char*)arena_dev;
  if (arena_bytes < h->lay.total) {
    smi_set_error("smi_enc_create: arena is %zu bytes, layout needs %zu", arena_bytes, h->lay.total);
    delete h;
    return SMI_EINVAL;
  }
  const smi_enc_cfg& c = h->cfg;
  // the perceiver attends over its latents and one context column per mel frame: the longest reference clip must fit k_mha
  if (c.spk_tokens + c.max_ref_samples / c.hop_length + 1 > kMaxKeys) {
    smi_set_error("smi_enc_create: spk_tokens=%d + %d mel frames of max_ref_samples=%d exceed the attention kernel's %d-key score buffer",
                  c.spk_tokens, c.max_ref_samples / c.hop_length + 1, c.max_ref_samples, kMaxKeys);
    delete h;
    return SMI_EINVAL;
  }
  {
    const char* e = smi_env("SPARKMI_ENC_GRAPH");
    h->use_graph = !(e && e[0] == '0');
  }
  // more than the default dynamic LDS window for the attention / positional-conv kernels (per device, before any capture)
  {
    const hipError_t e1 = hipFuncSetAttribute((const void*)k_mha, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    const hipError_t e2 = e1 == hipSuccess ? hipFuncSetAttribute((const void*)k_posconv, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) : e1;
    if (e2 != hipSuccess) {
      smi_set_error("smi_enc_create: could not raise the dynamic LDS window of %s to 96 KB: %s", e1 != hipSuccess ? "k_mha" : "k_posconv",
                    hipGetErrorString(e2));
      smi_enc_destroy(h);
      return SMI_EHIP;
    }
  }
  if (ws_alloc(c, h->solo, "smi_enc_create", 1, c.max_samples, c.max_ref_samples) ||
      h->cbn.alloc((size_t)c.codebook_size * c.codebook_dim * 4, "smi_enc_create: cbn") || h->c2.alloc((size_t)c.codebook_size * 4, "smi_enc_create: c2")) {
    smi_enc_destroy(h);
    return SMI_EHIP;
  }
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
      hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->gev0, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->gev1, hipEventDisableTiming) != hipSuccess) {
    smi_set_error("smi_enc_create: event / stream creation failed");
    smi_enc_destroy(h);
    return SMI_EHIP;
  }
  hipLaunchKernelGGL(k_cbnorm, dim3((c.codebook_size + 255) / 256), dim3(256), 0, 0, ent(h, "quantizer.codebook.weight"),
                     c.codebook_size, c.codebook_dim, h->cbn, h->c2);
  if (hipDeviceSynchronize() != hipSuccess) {
    smi_set_error("smi_enc_create: codebook normalisation failed");
    smi_enc_destroy(h);
    return SMI_EHIP;
  }
  *out = h;
  return SMI_OK;
}

int smi_enc_destroy(smi_enc* h) {
  if (!h) return SMI_OK;
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  for (auto& kv : h->graphs)
    if (kv.second.exec) {
      if (kv.second.launched) (void)hipStreamSynchronize(kv.second.last);   // an exec is never destroyed while a launch of it may be running
      (void)hipGraphExecDestroy(kv.second.exec);
    }
  if (h->gev0) (void)hipEventDestroy(h->gev0);
  if (h->gev1) (void)hipEventDestroy(h->gev1);
  if (h->gstream) (void)hipStreamDestroy(h->gstream);
  delete h;
  return SMI_OK;
}

}  // extern "C"

namespace {

RowLens row_lens(const smi_enc_cfg& c, int n_samples, int n_ref) {
  RowLens r;
  memset(&r, 0, sizeof(r));
  int n = n_samples;
  for (int i = 0; i < c.w2v_nconv; ++i) { n = conv_out_len(n, c.w2v_kernel[i], c.w2v_stride[i]); r.v[LK_T0 + i] = n; }
  r.v[LK_NS] = n_samples; r.v[LK_NREF] = n_ref;
  r.v[LK_TM] = n_ref / c.hop_length + 1; r.v[LK_TK] = c.spk_tokens + r.v[LK_TM];
  r.v[LK_ONE] = 1; r.v[LK_NT] = c.spk_tokens;
  return r;
}

// What one launch sequence covers: rows r0 .. r0 + B of workspace W, whose launch plans agree.  `ext` (the longest row, kind by
// kind) sizes grids, row strides and dynamic LDS, `plan` (the first row's own lengths) picks every conv launch's tiling and
// kernel form (PlanShape), and each row's lengths are read from W.lens_dev[kind][r0 + b].  smi_enc_forward's list is the span of
// one row on the solo workspace: ext = plan = the row's own lengths.
struct EncSpan {
  const smi_enc::Ws* W;
  int r0, B;
  RowLens ext, plan;
  const RowLens* own;      // [B] each row's lengths (debug views)
  const float* wav; long long wav_bs;
  const float* ref; long long ref_bs;
  int64_t* sem; long long sem_bs;
  int32_t* glob; long long glob_bs;
};

// The launch sequence of one span (P) and the debug views of its rows (stages[0 .. B), or null); nothing runs here and nothing
// of the handle changes.
int enc_program(smi_enc* h, const EncSpan& sp, std::vector<Launch>& P, std::map<std::string, smi_enc::Stage>* stages) {
  const smi_enc_cfg& c = h->cfg;
  const smi_enc::Ws& W = *sp.W;
  const RowLens& E = sp.ext;
  const int kT = LK_T0 + c.w2v_nconv - 1;
  const int T = E.v[kT], Tm = E.v[LK_TM], n_samples = E.v[LK_NS];
  auto len = [&](int kind) -> const int* { return W.lens_dev + (size_t)kind * W.max_rows + sp.r0; };
  const long long bs = W.slab;      // one batch stride for every working buffer
  const unsigned nB = (unsigned)sp.B;
  auto B = [&](const char* n) -> float* { return W.at(sp.r0, n); };
  // a small kernel: the launch runs with the grid / block / dynamic LDS recorded here (what smi_enc_debug_launch reports)
  using Geo = std::function<void(hipStream_t, dim3, dim3, size_t)>;
  auto closure = [&](const std::string& name, double flops, dim3 grid, int blk, size_t lds, Geo fn) {
    Launch L; L.kind = 9; L.name = name; L.flops = flops * sp.B; grid.z = nB; L.grid = grid; L.blk = blk; L.lds = lds;
    L.fn = [=](hipStream_t s) { fn(s, grid, dim3(blk), lds); };
    P.push_back(std::move(L));
  };
  // cols: a length kind (>= 0) or the literal -cols
  auto stage = [&](const std::string& name, const float* p, int rows, int cols, int stride) {
    if (!stages) return;
    for (int b = 0; b < sp.B; ++b) stages[b][name] = {p + b * bs, rows, cols >= 0 ? sp.own[b].v[cols] : -cols, stride};
  };
  auto lnorm = [&](const std::string& name, const std::string& pfx, const float* dww, const float* dwb, const float* X, float* Y, int C,
                   int kind, float eps, int gelu, int triple) {
    const int Tn = E.v[kind];
    Launch L; L.kind = 1; L.name = name; L.flops = ((dww ? 14.0 : 0.0) * C * Tn + 8.0 * C * Tn) * sp.B;
    LnP& p = L.lp; memset(&p, 0, sizeof(p));
    p.X = X; p.Y = Y; p.dww = dww; p.dwb = dwb; p.lens = len(kind); p.C = C; p.stride = Tn; p.bs = bs; p.triple = triple;
    p.w = ent(h, pfx + ".weight"); p.bsh = ent(h, pfx + ".bias"); p.eps = eps; p.gelu = gelu;
    L.cpt = (C + 31) / 32; L.grid = dim3((Tn + 7) / 8, nB); L.blk = 256; L.lds = 0;
    P.push_back(L);
  };
  // Linear / Conv1d on [C][T] activations: input lengths of kind kin, output lengths of kind kout; row strides are the span's
  // extents, the plan is the plan row's own output length.  spec: the layer's ConvSpec, for a caller that names further epilogue
  // operands; conv: the launch of that spec as it stands.
  PlanShape kps[LK_COUNT];   // the plan row's length of every kind, as given
  for (int k = 0; k < LK_COUNT; ++k) kps[k] = PlanShape{0, 0, sp.plan.v[k]};
  auto spec = [&](const std::string& name, const std::string& wname, const std::string& bname, int Cout, int Cin, int K, int dil, int pad,
                  const float* X, int xstride, float* Y, const float* R, int ystride, int kin, int kout, int act, int istr) {
    ConvSpec s;
    s.name = name; s.W = ent(h, wname); s.bias = bname.empty() ? nullptr : ent(h, bname); s.bf = ent_is_bf(h, wname);
    s.Cout = Cout; s.Cin = Cin; s.K = K; s.dil = dil; s.pad = pad; s.istr = istr; s.act = act;
    s.X = X; s.xstride = xstride; s.xb = bs; s.Y = Y; s.R = R; s.ystride = ystride; s.yb = bs;
    s.lens = len(kin); s.olens = kin == kout ? nullptr : len(kout); s.B = sp.B; s.Lmax = E.v[kout]; s.ps = &kps[kout];
    return s;
  };
  auto conv = [&](auto&&... a) { P.push_back(make_conv(spec(a...))); };
  // attention of every row over its own kq queries and kk keys; the score rows in LDS are sized by the span's longest row
  auto mha = [&](const std::string& name, const float* Q, int qs, const float* K, int ks, const float* V, int vs, float* O, int os,
                 int heads, int kq, int kk) {
    MhaP m{Q, K, V, O, qs, ks, vs, os, 0, 0, 0.125f, len(kq), len(kk), bs};
    const int Tq = E.v[kq], Tk = E.v[kk];
    const size_t lds = (size_t)(512 + 8 * Tk + 64 * 65) * 4;
    closure(name, 4.0 * heads * 64.0 * Tq * Tk, dim3((Tq + 7) / 8, heads), 256, lds, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_mha, g, b, l, s, m);
    });
  };

  // ================= wav2vec2 =================
  float* wavn = B("wavn");
  {
    const float* wav = sp.wav;
    const long long wbs = sp.wav_bs;
    const int* ns = len(LK_NS);
    closure("w2v.normalize", 4.0 * n_samples, dim3(1), 1024, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_wavnorm, g, b, l, s, wav, wbs, ns, wavn, bs);
    });
  }
  stage("input_values", wavn, 1, LK_NS, n_samples);
  const int CD = c.w2v_conv_dim;
  float* cf[2] = {B("cf0"), B("cf1")};
  int cur = 0;
  {
    const float* W0 = ent(h, "w2v.feature_extractor.conv_layers.0.conv.weight");
    const float* b0 = ent(h, "w2v.feature_extractor.conv_layers.0.conv.bias");
    float* Y = cf[0];
    const int K0 = c.w2v_kernel[0], S0 = c.w2v_stride[0], T0 = E.v[LK_T0];
    const int* t0s = len(LK_T0);
    closure("w2v.conv0", 2.0 * CD * K0 * T0, dim3((T0 + 255) / 256, CD), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_conv0, g, b, l, s, wavn, W0, b0, K0, S0, Y, CD, t0s, T0, bs);
    });
    lnorm("w2v.conv0.ln+gelu", "w2v.feature_extractor.conv_layers.0.layer_norm", nullptr, nullptr, cf[0], cf[1], CD, LK_T0, 1e-5f, 1, 0);
    cur = 1;
  }
  for (int i = 1; i < c.w2v_nconv; ++i) {
    const std::string p = "w2v.feature_extractor.conv_layers." + std::to_string(i);
    const int Tc = E.v[LK_T0 + i - 1], Tn = E.v[LK_T0 + i];
    // conv reads cf[cur] (stride Tc), writes cf[1-cur] (stride Tn); LN + GELU back into cf[cur] with stride Tn
    conv(p + ".conv", p + ".conv.weight", p + ".conv.bias", CD, CD, c.w2v_kernel[i], 1, 0, cf[cur], Tc, cf[1 - cur], nullptr, Tn, LK_T0 + i - 1,
         LK_T0 + i, ACT_NONE, c.w2v_stride[i]);
    lnorm(p + ".ln+gelu", p + ".layer_norm", nullptr, nullptr, cf[1 - cur], cf[cur], CD, LK_T0 + i, 1e-5f, 1, 0);
  }
  stage("conv_feats", cf[cur], CD, kT, T);
  const int Hd = c.w2v_hidden, I = c.w2v_inter;
  float *hbuf = B("h"), *x = B("x"), *wide = B("wide"), *att = B("att"), *acc = B("acc"), *feat = B("feat");
  const int* Tlen = len(kT);
  lnorm("w2v.feature_projection.ln", "w2v.feature_projection.layer_norm", nullptr, nullptr, cf[cur], cf[1 - cur], CD, kT, c.w2v_eps, 0, 0);
  conv("w2v.feature_projection.projection", "w2v.feature_projection.projection.weight", "w2v.feature_projection.projection.bias", Hd, CD, 1, 1,
       0, cf[1 - cur], T, x, nullptr, T, kT, kT, ACT_NONE, 1);
  {
    const float* Wp = ent(h, "w2v.encoder.pos_conv_embed.conv.weight");
    const float* bp = ent(h, "w2v.encoder.pos_conv_embed.conv.bias");
    const int Cg = Hd / c.w2v_pos_groups, K = c.w2v_pos_k;
    const size_t lds = (size_t)Cg * (64 + K - 1) * 4;
    closure("w2v.pos_conv+gelu+res", 2.0 * Hd * Cg * K * T, dim3((T + 63) / 64, Hd / 16), 256, lds, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_posconv, g, b, l, s, x, Wp, bp, hbuf, Hd, Cg, K, Tlen, T, bs);
    });
  }
  {   // test view of hidden_states[0] (the residual stream is updated in place by the layers)
    float* d0 = B("dbg_hs0");
    closure("w2v.hs0(dbg copy)", 0.0, dim3((T + 255) / 256, Hd), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_copy2d, g, b, l, s, hbuf, T, bs, d0, T, bs, Hd, Tlen);
    });
    stage("hs0", d0, Hd, kT, T);
  }
  auto tap = [&](int idx) {
    // hidden_states[idx] is the residual stream before layer idx
    for (int k = 0; k < 3; ++k) {
      if (c.w2v_taps[k] != idx) continue;
      const int mode = k;
      closure("w2v.tap" + std::to_string(idx), 1.0 * Hd * T, dim3((T + 255) / 256, Hd), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
        hipLaunchKernelGGL(k_tap, g, b, l, s, hbuf, acc, feat, Tlen, T, bs, mode);
      });
    }
  };
  SMI_REQUIRE(c.w2v_taps[0] < c.w2v_taps[1] && c.w2v_taps[1] < c.w2v_taps[2], "smi_enc_forward: hidden-state taps must be increasing");
  tap(0);
  for (int l = 0; l < c.w2v_layers; ++l) {
    const std::string p = "w2v.encoder.layers." + std::to_string(l);
    lnorm(p + ".ln1", p + ".layer_norm", nullptr, nullptr, hbuf, x, Hd, kT, c.w2v_eps, 0, 0);
    conv(p + ".qkv", "cat:" + p + ".attention.q_proj.weight|" + p + ".attention.k_proj.weight|" + p + ".attention.v_proj.weight",
         "cat:" + p + ".attention.q_proj.bias|" + p + ".attention.k_proj.bias|" + p + ".attention.v_proj.bias", 3 * Hd, Hd, 1, 1, 0, x, T,
         wide, nullptr, T, kT, kT, ACT_NONE, 1);
    mha(p + ".attention", wide, T, wide + (size_t)Hd * T, T, wide + (size_t)2 * Hd * T, T, att, T, c.w2v_heads, kT, kT);
    conv(p + ".out_proj+res", p + ".attention.out_proj.weight", p + ".attention.out_proj.bias", Hd, Hd, 1, 1, 0, att, T, hbuf, hbuf, T, kT, kT,
         ACT_NONE, 1);
    lnorm(p + ".ln2", p + ".final_layer_norm", nullptr, nullptr, hbuf, x, Hd, kT, c.w2v_eps, 0, 0);
    conv(p + ".ffn1+gelu", p + ".feed_forward.intermediate_dense.weight", p + ".feed_forward.intermediate_dense.bias", I, Hd, 1, 1, 0, x, T,
         wide, nullptr, T, kT, kT, ACT_GELU, 1);
    conv(p + ".ffn2+res", p + ".feed_forward.output_dense.weight", p + ".feed_forward.output_dense.bias", Hd, I, 1, 1, 0, wide, T, hbuf, hbuf,
         T, kT, kT, ACT_NONE, 1);
    tap(l + 1);
  }
  stage("feat", feat, Hd, kT, T);

  // ================= BiCodec encoder + VQ (feat_encoder.py:76-87) =================
  {
    const int D = c.enc_dim, EI = c.enc_inter;
    float *e0 = B("e0"), *e1 = B("e1"), *e2 = B("e2"), *ew = B("ew");
    const float* in = feat;
    int cin = Hd;
    // Vocos backbone: embed conv7 -> LN -> nl x ConvNeXt -> final LN (vocos.py:324-335); result in e1 ([D][T])
    auto vocos = [&](const std::string& p, int nl, int triple_out) {
      conv(p + ".embed", p + ".embed.weight", p + ".embed.bias", D, cin, 7, 1, 3, in, T, e0, nullptr, T, kT, kT, ACT_NONE, 1);
      lnorm(p + ".norm", p + ".norm", nullptr, nullptr, e0, e2, D, kT, 1e-6f, 0, 0);     // residual stream in e2
      for (int j = 0; j < nl; ++j) {
        const std::string b = p + ".convnext." + std::to_string(j);
        lnorm(b + ".dwconv+norm", b + ".norm", ent(h, b + ".dwconv.weight"), ent(h, b + ".dwconv.bias"), e2, e0, D, kT, 1e-6f, 0, 0);
        conv(b + ".pwconv1", b + ".pwconv1.weight", b + ".pwconv1.bias", EI, D, 1, 1, 0, e0, T, ew, nullptr, T, kT, kT, ACT_GELU, 1);
        ConvSpec s = spec(b + ".pwconv2", b + ".pwconv2.weight", b + ".pwconv2.bias", D, EI, 1, 1, 0, ew, T, e2, e2, T, kT, kT, ACT_NONE, 1);
        s.gamma = ent(h, b + ".gamma");
        P.push_back(make_conv(s));
      }
      lnorm(p + ".final_layer_norm", p + ".final_layer_norm", nullptr, nullptr, e2, e1, D, kT, 1e-6f, 0, triple_out);
      in = e1; cin = D;
    };
    vocos("encoder.encoder", c.enc_layers, c.enc_num_down > 0 ? 1 : 0);   // SamplingBlock(ratio 1) = 3x (samper.py:79-100)
    for (int i = 0; i < c.enc_num_down; ++i) vocos("encoder.downsample." + std::to_string(i) + ".1", 2, (i + 1 < c.enc_num_down) ? 1 : 0);
    conv("encoder.project", "encoder.project.weight", "encoder.project.bias", c.enc_out, D, 1, 1, 0, e1, T, ew, nullptr, T, kT, kT, ACT_NONE, 1);
    stage("z", ew, c.enc_out, kT, T);
    conv("quantizer.in_project", "quantizer.in_project.weight", "quantizer.in_project.bias", c.codebook_dim, c.enc_out, 1, 1, 0, ew, T, e0,
         nullptr, T, kT, kT, ACT_NONE, 1);
    const float *cbn = h->cbn, *c2 = h->c2;
    const int Dc = c.codebook_dim, nc = c.codebook_size;
    int64_t* sem = sp.sem;
    const long long sbs = sp.sem_bs;
    closure("quantizer.argmax", 2.0 * T * nc * Dc, dim3(T), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_vq, g, b, l, s, e0, Dc, Tlen, T, bs, cbn, c2, nc, sem, sbs);
    });
  }

  // ================= mel + ECAPA-TDNN latent + perceiver + FSQ =================
  {
    const int nf = c.n_fft / 2 + 1, nfft = c.n_fft, hop = c.hop_length;
    float *fr = B("frames"), *dft = B("dft"), *mag = B("mag"), *mel = B("mel");
    const int* Tmlen = len(LK_TM);
    {
      const float* ref = sp.ref;
      const long long rbs = sp.ref_bs;
      const int* nrs = len(LK_NREF);
      closure("mel.frames", 1.0 * nfft * Tm, dim3((Tm + 255) / 256, nfft), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
        hipLaunchKernelGGL(k_frames, g, b, l, s, ref, rbs, nrs, nfft, hop, fr, Tmlen, Tm, bs);
      });
    }
    conv("mel.dft", "mel.dft", "", 2 * nf, nfft, 1, 1, 0, fr, Tm, dft, nullptr, Tm, LK_TM, LK_TM, ACT_NONE, 1);
    closure("mel.magnitude", 4.0 * nf * Tm, dim3((Tm + 255) / 256, nf), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_mag, g, b, l, s, dft, nf, Tmlen, Tm, mag, bs);
    });
    conv("mel.filterbank", "mel.fb", "", c.num_mels, nf, 1, 1, 0, mag, Tm, mel, nullptr, Tm, LK_TM, LK_TM, ACT_NONE, 1);
    stage("mel", mel, c.num_mels, LK_TM, Tm);
    // ---- ECAPA-TDNN (ecapa_tdnn.py:186-197): bn(relu(conv(x))) fused as ReLU + affine in the conv epilogue
    const int C = c.ecapa_channels, W = C / 8;
    const std::string se = "speaker_encoder.speaker_encoder";
    float *ea = B("ec_a"), *eb = B("ec_b"), *ec = B("ec_c"), *ecat = B("ec_cat"), *elat = B("ec_lat"), *evec = B("ec_vec");
    // conv `pfx`(X + X2) -> ReLU -> BatchNorm `bn`
    auto crb = [&](const std::string& name, const std::string& pfx, const std::string& bn, int co, int ci, int k, int dil, int pad, const float* X,
                   const float* X2, float* Y) {
      ConvSpec s = spec(name, pfx + ".weight", pfx + ".bias", co, ci, k, dil, pad, X, Tm, Y, nullptr, Tm, LK_TM, LK_TM, ACT_RELU, 1);
      s.gamma = ent(h, "bnscale:" + bn); s.beta = ent(h, "bnshift:" + bn); s.X2 = X2;
      P.push_back(make_conv(s));
    };
    crb(se + ".layer1", se + ".layer1.conv", se + ".layer1.bn", C, c.num_mels, 5, 1, 2, mel, nullptr, ea);
    const float* xin = ea;
    for (int li = 2; li <= 4; ++li) {
      const std::string b = se + ".layer" + std::to_string(li) + ".se_res2block";
      const int dil = li;
      float* y0 = eb;      // after the first 1x1
      float* y1 = ec;      // Res2 output (cat of the 8 branches)
      crb(b + ".0", b + ".0.conv", b + ".0.bn", C, C, 1, 1, 0, xin, nullptr, y0);
      for (int j = 0; j < 7; ++j) {
        const std::string cj = b + ".1.convs." + std::to_string(j);
        // sp = conv(out_{j-1} + spx[j]) -> relu -> bn  (ecapa_tdnn.py:50-58); branch j reads slice j of y0, writes slice j of y1
        crb(cj, cj, b + ".1.bns." + std::to_string(j), W, W, 3, dil, dil, y0 + (size_t)j * W * Tm, j >= 1 ? y1 + (size_t)(j - 1) * W * Tm : nullptr,
            y1 + (size_t)j * W * Tm);
      }
      {
        const float* src = y0 + (size_t)7 * W * Tm;
        float* dst = y1 + (size_t)7 * W * Tm;
        closure(b + ".1.passthrough", 0.0, dim3((Tm + 255) / 256, W), 256, 0, [=](hipStream_t s, dim3 g, dim3 bl, size_t l) {
          hipLaunchKernelGGL(k_copy2d, g, bl, l, s, src, Tm, bs, dst, Tm, bs, W, Tmlen);
        });
      }
      crb(b + ".2", b + ".2.conv", b + ".2.bn", C, C, 1, 1, 0, y1, nullptr, y0);
      float *mean = evec, *s1 = evec + C, *s2 = evec + C + 128;
      closure(b + ".3.mean", 1.0 * C * Tm, dim3((C + 3) / 4), 256, 0, [=](hipStream_t s, dim3 g, dim3 bl, size_t l) {
        hipLaunchKernelGGL(k_rowmean, g, bl, l, s, y0, C, Tmlen, Tm, mean, bs);
      });
      // the two vector projections: one vector per row (k_gemv1: block y is the row)
      auto gemv = [&](const std::string& l, int co, int ci, const float* X, float* Y, int act) {
        ConvSpec s = spec(l, l + ".weight", l + ".bias", co, ci, 1, 1, 0, X, 1, Y, nullptr, 1, LK_ONE, LK_ONE, act, 1);
        s.want = CONV_GEMV;
        P.push_back(make_conv(s));
      };
      gemv(b + ".3.linear1", 128, C, mean, s1, ACT_RELU);
      gemv(b + ".3.linear2", C, 128, s1, s2, ACT_SIGMOID);
      float* outl = ecat + (size_t)(li - 2) * C * Tm;
      const float* xi = xin;
      closure(b + ".3.scale+res", 2.0 * C * Tm, dim3((Tm + 255) / 256, C), 256, 0, [=](hipStream_t s, dim3 g, dim3 bl, size_t l) {
        hipLaunchKernelGGL(k_se, g, bl, l, s, xi, y0, s2, outl, Tmlen, Tm, Tm, bs);
      });
      xin = outl;
    }
    conv(se + ".conv+relu", se + ".conv.weight", se + ".conv.bias", c.ecapa_out, 3 * C, 1, 1, 0, ecat, Tm, elat, nullptr, Tm, LK_TM, LK_TM, ACT_RELU, 1);
    stage("ecapa_latent", elat, c.ecapa_out, LK_TM, Tm);
    // ---- perceiver resampler (perceiver_encoder.py:297-350): ctx buffer = [latents | projected context] along time
    const std::string ps = "speaker_encoder.perceiver_sampler";
    const int Ld = c.spk_latent, Nt = c.spk_tokens, Tk = E.v[LK_TK], inner = c.perc_heads * 64, FI = c.perc_ff_inner;
    float *ctx = B("pctx"), *pq = B("pq"), *pkv = B("pkv"), *po = B("po"), *pff = B("pff"), *pg = B("pg"), *pout = B("pout");
    const int* Ntlen = len(LK_NT);
    {
      const float* lt = ent(h, "transpose:" + ps + ".latents");
      closure(ps + ".latents", 0.0, dim3((Nt + 255) / 256, Ld), 256, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
        hipLaunchKernelGGL(k_copy2d, g, b, l, s, lt, Nt, 0LL, ctx, Tk, bs, Ld, Ntlen);
      });
    }
    conv(ps + ".proj_context", ps + ".proj_context.weight", ps + ".proj_context.bias", Ld, c.ecapa_out, 1, 1, 0, elat, Tm, ctx + Nt, nullptr, Tk,
         LK_TM, LK_TM, ACT_NONE, 1);
    for (int i = 0; i < c.perc_depth; ++i) {
      const std::string a = ps + ".layers." + std::to_string(i) + ".0", f = ps + ".layers." + std::to_string(i) + ".1";
      conv(a + ".to_q", a + ".to_q.weight", "", inner, Ld, 1, 1, 0, ctx, Tk, pq, nullptr, Nt, LK_NT, LK_NT, ACT_NONE, 1);
      conv(a + ".to_kv", a + ".to_kv.weight", "", 2 * inner, Ld, 1, 1, 0, ctx, Tk, pkv, nullptr, Tk, LK_TK, LK_TK, ACT_NONE, 1);
      mha(a + ".attend", pq, Nt, pkv, Tk, pkv + (size_t)inner * Tk, Tk, po, Nt, c.perc_heads, LK_NT, LK_TK);
      conv(a + ".to_out+res", a + ".to_out.weight", "", Ld, inner, 1, 1, 0, po, Nt, ctx, ctx, Tk, LK_NT, LK_NT, ACT_NONE, 1);
      conv(f + ".0", f + ".0.weight", f + ".0.bias", 2 * FI, Ld, 1, 1, 0, ctx, Tk, pff, nullptr, Nt, LK_NT, LK_NT, ACT_NONE, 1);
      closure(f + ".geglu", 10.0 * FI * Nt, dim3(1, FI), 64 * ((Nt + 63) / 64), 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
        hipLaunchKernelGGL(k_geglu, g, b, l, s, pff, FI, Nt, Nt, pg, bs);
      });
      conv(f + ".2+res", f + ".2.weight", f + ".2.bias", Ld, FI, 1, 1, 0, pg, Nt, ctx, ctx, Tk, LK_NT, LK_NT, ACT_NONE, 1);
    }
    {
      const float* gm = ent(h, ps + ".norm.gamma");
      closure(ps + ".norm", 4.0 * Ld * Nt, dim3((Nt + 63) / 64), 64, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
        hipLaunchKernelGGL(k_rmsn, g, b, l, s, ctx, Ld, Nt, Tk, gm, pout, Nt, bs);
      });
    }
    stage("perceiver", pout, Ld, -Nt, Nt);
    FsqQP q;
    memset(&q, 0, sizeof(q));
    q.X = pout; q.W = ent(h, "speaker_encoder.quantizer.project_in.weight"); q.b = ent(h, "speaker_encoder.quantizer.project_in.bias");
    q.out = sp.glob; q.bounded = B("fsqb"); q.latent = Ld; q.stride = Nt; q.Ntok = Nt; q.nd = c.fsq_dims;
    q.bs = bs; q.obs = sp.glob_bs;
    for (int j = 0; j < 8; ++j) q.levels[j] = j < c.fsq_dims ? c.fsq_levels[j] : 1;
    closure("speaker_encoder.quantizer", 2.0 * Nt * Ld * c.fsq_dims, dim3((Nt + 63) / 64), 64, 0, [=](hipStream_t s, dim3 g, dim3 b, size_t l) {
      hipLaunchKernelGGL(k_fsq_quant, g, b, l, s, q);
    });
    stage("fsq_bounded", B("fsqb"), Nt, -c.fsq_dims, c.fsq_dims);
  }

  for (const Launch& L : P) {
    int rc = L.kind == 0 ? check_conv(L, "smi_enc_forward") : SMI_OK;
    if (rc) return rc;
    if (L.kind == 1) SMI_REQUIRE(L.lp.w && L.lp.bsh && L.cpt <= 32, "smi_enc_forward: LayerNorm %s: missing weights or too many channels", L.name.c_str());
  }
  return SMI_OK;
}

// smi_enc_forward's argument checks on one row's lengths
int enc_check_row(const smi_enc_cfg& c, const char* who, int n_samples, int n_ref, int max_samples, int max_ref) {
  SMI_REQUIRE(n_samples >= 400 && n_samples <= max_samples, "%s: n_samples=%d outside 400..%d", who, n_samples, max_samples);
  SMI_REQUIRE(n_ref > c.n_fft / 2 && n_ref <= max_ref, "%s: n_ref=%d outside %d..%d", who, n_ref, c.n_fft / 2 + 1, max_ref);
  const RowLens r = row_lens(c, n_samples, n_ref);
  const int T = r.v[LK_T0 + c.w2v_nconv - 1];
  SMI_REQUIRE(T >= 2, "%s: %d samples give %d frames", who, n_samples, T);
  SMI_REQUIRE(T <= kMaxKeys, "%s: %d frames exceed the attention kernel's %d-key score buffer", who, T, kMaxKeys);
  SMI_REQUIRE(r.v[LK_TK] <= kMaxKeys, "%s: %d speaker tokens + %d mel frames exceed the attention kernel's %d-key score buffer", who,
              c.spk_tokens, r.v[LK_TM], kMaxKeys);
  return SMI_OK;
}

int enc_run(const std::vector<Launch>& P, hipStream_t st) {
  for (const Launch& L : P) {
    int rc = run_launch(L, st);
    if (rc) return rc;
  }
  return SMI_OK;
}

// The launch list of B rows on workspace W (W.prog, .run_start, .stages, .host_lens); nothing runs.  A row's plan is the
// signature of its one-row list; consecutive rows with equal plans form a run: one launch sequence with the first row's plan and
// the extent (rows of the run, its longest row of every length kind).  A call of one row is that one-row list itself.
int enc_build(smi_enc* h, smi_enc::Ws& W, const char* who, const float* wav, long long wav_bs, const int32_t* ns, const float* ref,
              long long ref_bs, const int32_t* nref, int B, int64_t* sem, long long sem_bs, int32_t* glob, long long glob_bs, int32_t* n_frames) {
  const smi_enc_cfg& c = h->cfg;
  W.prog.clear(); W.run_start.clear(); W.stages.clear(); W.lastB = 0;
  SMI_REQUIRE(W.ws, "%s: no rows workspace (smi_enc_rows_reserve first)", who);
  SMI_REQUIRE(B >= 1 && B <= W.max_rows, "%s: B=%d outside the reserved 1..%d rows", who, B, W.max_rows);
  int rc;
  for (int b = 0; b < B; ++b)
    if ((rc = enc_check_row(c, who, ns[b], nref[b], W.max_samples, W.max_ref))) return rc;
  const int kT = LK_T0 + c.w2v_nconv - 1;
  std::vector<RowLens> own((size_t)B);
  std::vector<const std::vector<long long>*> sig((size_t)B, nullptr);
  if (h->sigs.size() > 1024) h->sigs.clear();   // (before the first lookup: the pointers below stay valid across insertions)
  for (int b = 0; b < B; ++b) {
    own[b] = row_lens(c, ns[b], nref[b]);
    if (B == 1) break;                          // (nothing to group: the list below is the row's own plan)
    const std::pair<int, int> key(ns[b], nref[b]);
    auto it = h->sigs.find(key);
    if (it == h->sigs.end()) {
      // the choices of that row's one-row list (pointers do not enter a signature)
      std::vector<Launch> one;
      const EncSpan sp{&h->solo, 0, 1, own[b], own[b], &own[b], wav, 0, ref, 0, sem, 0, glob, 0};
      if ((rc = enc_program(h, sp, one, nullptr))) return rc;
      it = h->sigs.emplace(key, plan_signature(one)).first;
    }
    sig[b] = &it->second;
  }
  W.stages.resize((size_t)B);
  W.host_lens.assign((size_t)LK_COUNT * W.max_rows, 0);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < LK_COUNT; ++k) W.host_lens[(size_t)k * W.max_rows + b] = own[b].v[k];
  const std::vector<int> runs = plan_runs(sig);
  std::vector<Launch> G;
  for (size_t i = 0; i + 1 < runs.size(); ++i) {
    const int r0 = runs[i], r1 = runs[i + 1];
    // (every length kind grows with its input, so the longest row of each kind is that of the longest wav / reference clip)
    const EncSpan sp{&W, r0, r1 - r0, row_lens(c, *std::max_element(ns + r0, ns + r1), *std::max_element(nref + r0, nref + r1)), own[r0], &own[r0],
                     wav + r0 * wav_bs, wav_bs, ref + r0 * ref_bs, ref_bs, sem + r0 * sem_bs, sem_bs, glob + r0 * glob_bs, glob_bs};
    G.clear();
    if ((rc = enc_program(h, sp, G, &W.stages[r0]))) { W.prog.clear(); return rc; }
    if (sig[r0] && plan_signature(G) != *sig[r0]) {
      W.prog.clear();
      smi_set_error("%s: the launch list of rows %d..%d does not carry the plan of a row of %d samples / %d reference samples", who, r0, r1 - 1,
                    ns[r0], nref[r0]);
      return SMI_EINVAL;
    }
    W.run_start.push_back(r0);
    W.prog.insert(W.prog.end(), G.begin(), G.end());
  }
  for (int b = 0; b < B; ++b) n_frames[b] = own[b].v[kT];
  W.lastB = B;
  return SMI_OK;
}

// smi_enc_forward's list: one row on the solo workspace
int enc_build_solo(smi_enc* h, const char* who, const float* wav_dev, int n_samples, const float* ref_dev, int n_ref, int64_t* sem_dev,
                   int32_t* glob_dev, int* n_frames) {
  const int32_t ns = n_samples, nr = n_ref;
  int32_t nf = 0;
  const int rc = enc_build(h, h->solo, who, wav_dev, 0, &ns, ref_dev, 0, &nr, 1, sem_dev, 0, glob_dev, 0, &nf);
  *n_frames = nf;
  return rc;
}

int enc_upload_lens(const smi_enc::Ws& W, hipStream_t st) {
  SMI_HIP(hipMemcpyAsync(W.lens_dev, W.host_lens.data(), W.host_lens.size() * 4, hipMemcpyHostToDevice, st));
  return SMI_OK;
}

// one debug view of row `row` of the list last built on W, copied out densely
int enc_stage(const smi_enc::Ws& W, const char* who, int row, const char* name, float* out_dev, size_t max_floats, int32_t* dims, void* stream) {
  SMI_REQUIRE(name && out_dev && dims, "%s: null argument", who);
  SMI_REQUIRE(row >= 0 && row < W.lastB && row < (int)W.stages.size(), "%s: row %d outside the last rows call (%d rows)", who, row, W.lastB);
  auto it = W.stages[row].find(name);
  SMI_REQUIRE(it != W.stages[row].end(), "%s: unknown stage '%s'", who, name);
  const smi_enc::Stage& s = it->second;
  SMI_REQUIRE((size_t)s.rows * s.cols <= max_floats, "%s: output buffer too small", who);
  SMI_HIP(hipMemcpy2DAsync(out_dev, (size_t)s.cols * 4, s.ptr, (size_t)s.stride * 4, (size_t)s.cols * 4, s.rows, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  dims[0] = s.rows; dims[1] = s.cols;
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_enc_forward(smi_enc* h, const float* wav_dev, int n_samples, const float* ref_dev, int n_ref, int64_t* sem_dev,
                    int32_t* glob_dev, int* n_frames, void* stream) {
  SMI_REQUIRE(h && wav_dev && ref_dev && sem_dev && glob_dev && n_frames, "smi_enc_forward: null argument");
  const smi_enc_cfg& c = h->cfg;
  smi_enc::Ws& S = h->solo;
  SMI_REQUIRE(n_samples >= 400 && n_samples <= c.max_samples, "smi_enc_forward: n_samples=%d outside 400..%d", n_samples, c.max_samples);
  SMI_REQUIRE(n_ref > c.n_fft / 2 && n_ref <= c.max_ref_samples, "smi_enc_forward: n_ref=%d outside %d..%d", n_ref, c.n_fft / 2 + 1,
              c.max_ref_samples);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  const std::pair<int, int> key(n_samples, n_ref);
  bool eager = !h->use_graph;
  if (!eager && h->graphs.find(key) == h->graphs.end()) {
    if (h->seen.size() > 4096) h->seen.clear();
    eager = h->seen[key]++ == 0;
  }
  if (eager) {
    h->prog_key = {-1, -1};
    if ((rc = enc_build_solo(h, "smi_enc_forward", wav_dev, n_samples, ref_dev, n_ref, sem_dev, glob_dev, n_frames))) return rc;
    if ((rc = enc_upload_lens(S, st))) return rc;
    if ((rc = enc_run(S.prog, st))) return rc;
    h->last_frames = *n_frames;
    return SMI_OK;
  }
  float *in_wav = S.at(0, "in_wav"), *in_ref = S.at(0, "in_ref");
  int64_t* out_sem = (int64_t*)S.at(0, "out_sem");
  int32_t* out_glob = (int32_t*)S.at(0, "out_glob");
  // the null stream cannot be captured: such callers' encodes run on the handle's own stream, fenced by events on both sides
  hipStream_t run = st ? st : h->gstream;
  if (!st) {
    SMI_HIP(hipEventRecord(h->gev0, st));
    SMI_HIP(hipStreamWaitEvent(run, h->gev0, 0));
  }
  SMI_HIP(hipMemcpyAsync(in_wav, wav_dev, (size_t)n_samples * 4, hipMemcpyDeviceToDevice, run));
  SMI_HIP(hipMemcpyAsync(in_ref, ref_dev, (size_t)n_ref * 4, hipMemcpyDeviceToDevice, run));
  auto it = h->graphs.find(key);
  if (it == h->graphs.end()) {
    if (h->graphs.size() >= 8) {   // keep the eight most recently used shapes
      auto old = h->graphs.begin();
      for (auto j = h->graphs.begin(); j != h->graphs.end(); ++j) if (j->second.used < old->second.used) old = j;
      SMI_HIP(hipStreamSynchronize(run));
      if (old->second.launched && old->second.last != run) SMI_HIP(hipStreamSynchronize(old->second.last));   // it may have last run on another caller's stream
      if (old->second.exec) (void)hipGraphExecDestroy(old->second.exec);
      h->graphs.erase(old);
    }
    int T = 0;
    if ((rc = enc_build_solo(h, "smi_enc_forward", in_wav, n_samples, in_ref, n_ref, out_sem, out_glob, &T))) return rc;
    smi_enc::Graph g;
    g.lens = S.host_lens; g.prog = S.prog; g.stages = S.stages; g.frames = T;
    SMI_HIP(hipMemcpyAsync(S.lens_dev, g.lens.data(), g.lens.size() * 4, hipMemcpyHostToDevice, run));
    SMI_HIP(hipStreamSynchronize(run));      // (the pageable source above must be read before g.lens moves into the map)
    SMI_HIP(hipStreamBeginCapture(run, hipStreamCaptureModeRelaxed));
    rc = enc_run(g.prog, run);
    hipGraph_t graph = nullptr;
    const hipError_t ec = hipStreamEndCapture(run, &graph);
    if (rc || ec != hipSuccess || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      if (!rc) { smi_set_error("smi_enc_forward: stream capture failed: %s", hipGetErrorString(ec)); rc = SMI_EHIP; }
      return rc;
    }
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { smi_set_error("smi_enc_forward: hipGraphInstantiate: %s", hipGetErrorString(ei)); return SMI_EHIP; }
    h->prog_key = key;
    it = h->graphs.emplace(key, std::move(g)).first;
  } else {
    if (h->prog_key != key) { S.prog = it->second.prog; h->prog_key = key; }
    S.stages = it->second.stages; S.lastB = 1;
    SMI_HIP(hipMemcpyAsync(S.lens_dev, it->second.lens.data(), it->second.lens.size() * 4, hipMemcpyHostToDevice, run));
  }
  it->second.used = ++h->tick;
  SMI_HIP(hipGraphLaunch(it->second.exec, run));
  it->second.last = run; it->second.launched = true;
  const int T = it->second.frames;
  SMI_HIP(hipMemcpyAsync(sem_dev, out_sem, (size_t)T * 8, hipMemcpyDeviceToDevice, run));
  SMI_HIP(hipMemcpyAsync(glob_dev, out_glob, (size_t)c.spk_tokens * 4, hipMemcpyDeviceToDevice, run));
  if (!st) {
    SMI_HIP(hipEventRecord(h->gev1, run));
    SMI_HIP(hipStreamWaitEvent(st, h->gev1, 0));
  }
  h->last_frames = T;
  *n_frames = T;
  return SMI_OK;
}

int smi_enc_rows_reserve(smi_enc* h, int max_rows, int max_row_samples, int max_row_ref_samples) {
  SMI_REQUIRE(h, "smi_enc_rows_reserve: null handle");
  const smi_enc_cfg& c = h->cfg;
  SMI_REQUIRE(max_rows >= 1 && max_rows <= 4096, "smi_enc_rows_reserve: max_rows=%d outside 1..4096", max_rows);
  SMI_REQUIRE(max_row_samples >= 400 && max_row_samples <= c.max_samples, "smi_enc_rows_reserve: max_row_samples=%d outside 400..%d",
              max_row_samples, c.max_samples);
  SMI_REQUIRE(max_row_ref_samples > c.n_fft / 2 && max_row_ref_samples <= c.max_ref_samples,
              "smi_enc_rows_reserve: max_row_ref_samples=%d outside %d..%d", max_row_ref_samples, c.n_fft / 2 + 1, c.max_ref_samples);
  smi_enc::Ws& R = h->rows;
  if (R.ws && R.max_rows == max_rows && R.max_samples == max_row_samples && R.max_ref == max_row_ref_samples) return SMI_OK;
  SMI_HIP(hipDeviceSynchronize());      // a rows call may still be reading the workspace that goes
  return ws_alloc(c, R, "smi_enc_rows_reserve", max_rows, max_row_samples, max_row_ref_samples);
}

int smi_enc_forward_rows(smi_enc* h, const float* wav_dev, long long wav_stride, const int32_t* n_samples_host, const float* ref_dev,
                         long long ref_stride, const int32_t* n_ref_host, int B, int64_t* sem_dev, long long sem_stride, int32_t* glob_dev,
                         int32_t* n_frames_host, void* stream) {
  SMI_REQUIRE(h && wav_dev && n_samples_host && ref_dev && n_ref_host && sem_dev && glob_dev && n_frames_host,
              "smi_enc_forward_rows: null argument");
  hipStream_t st = (hipStream_t)stream;
  int rc = enc_build(h, h->rows, "smi_enc_forward_rows", wav_dev, wav_stride, n_samples_host, ref_dev, ref_stride, n_ref_host, B, sem_dev, sem_stride,
                     glob_dev, h->cfg.spk_tokens, n_frames_host);
  if (rc) return rc;
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(wav_stride >= n_samples_host[b] && ref_stride >= n_ref_host[b] && sem_stride >= n_frames_host[b],
                "smi_enc_forward_rows: row %d (%d samples, %d reference samples, %d frames) exceeds a row stride", b, n_samples_host[b],
                n_ref_host[b], n_frames_host[b]);
  }
  if ((rc = enc_upload_lens(h->rows, st))) return rc;
  return enc_run(h->rows.prog, st);
}

int smi_enc_debug_stage(smi_enc* h, const char* name, float* out_dev, size_t max_floats, int32_t* dims, void* stream) {
  SMI_REQUIRE(h, "smi_enc_debug_stage: null argument");
  SMI_REQUIRE(h->last_frames > 0, "smi_enc_debug_stage: no forward has run");
  return enc_stage(h->solo, "smi_enc_debug_stage", 0, name, out_dev, max_floats, dims, stream);
}

int smi_enc_num_launches(smi_enc* h) { return h ? (int)h->solo.prog.size() : 0; }

int smi_enc_time_launch(smi_enc* h, int index, int iters, float* ms_avg, double* flops, char* name, int name_cap, void* stream) {
  SMI_REQUIRE(h && ms_avg && iters > 0, "smi_enc_time_launch: bad argument");
  SMI_REQUIRE(index >= 0 && index < (int)h->solo.prog.size(), "smi_enc_time_launch: index %d out of range", index);
  return time_launch(h->solo.prog[index], h->ev0, h->ev1, iters, ms_avg, flops, name, name_cap, (hipStream_t)stream);
}

}  // extern "C"

#ifdef SMI_DIAG   // ---- include/sparkmi_debug.h: the encoder's launch lists one launch at a time, exported by libsparkmi_diag.so only

namespace {

// Each entry below exists for the solo list (smi_enc_debug_*: the solo workspace, row 0) and for the rows list
// (smi_enc_rows_debug_*: the rows workspace); `who` is the calling entry's name.
int dbg_build(smi_enc* h, smi_enc::Ws& W, const char* who, const int32_t* ns, const int32_t* nref, int B, int32_t* n_frames, int* n_launches,
              hipStream_t st) {
  SMI_REQUIRE(W.ws, "%s: no rows workspace (smi_enc_rows_reserve first)", who);
  int rc = enc_build(h, W, who, W.at(0, "in_wav"), W.slab, ns, W.at(0, "in_ref"), W.slab, nref, B, (int64_t*)W.at(0, "out_sem"), W.slab / 2,
                     (int32_t*)W.at(0, "out_glob"), W.slab, n_frames);
  if (rc) return rc;
  if ((rc = enc_upload_lens(W, st))) return rc;
  SMI_HIP(hipStreamSynchronize(st));
  *n_launches = (int)W.prog.size();
  return SMI_OK;
}

int dbg_launch(const smi_enc::Ws& W, const char* who, int index, char* name, int cap, int32_t* info) {
  SMI_REQUIRE(info, "%s: null argument", who);
  SMI_REQUIRE(index >= 0 && index < (int)W.prog.size(), "%s: index %d out of range", who, index);
  const Launch& L = W.prog[index];
  if (name && cap > 0) { strncpy(name, L.name.c_str(), (size_t)cap - 1); name[cap - 1] = 0; }
  info[0] = L.kind; info[1] = (int32_t)L.grid.x; info[2] = (int32_t)L.grid.y; info[3] = (int32_t)L.grid.z;
  info[4] = L.blk;
  info[5] = (int32_t)L.lds;
  info[6] = L.kind == 1 ? dwln_form(L.cpt) : 0;
  info[7] = 0;
  return SMI_OK;
}

int dbg_io(const smi_enc::Ws& W, const char* who, int row, const char* buffer_name, int write, void* host_ptr, size_t offset_floats, size_t floats) {
  SMI_REQUIRE(buffer_name && host_ptr, "%s: null argument", who);
  SMI_REQUIRE(W.ws, "%s: no rows workspace (smi_enc_rows_reserve first)", who);
  SMI_REQUIRE(row >= 0 && row < W.max_rows, "%s: row %d outside the reserved 0..%d", who, row, W.max_rows - 1);
  auto it = W.floats.find(buffer_name);
  SMI_REQUIRE(it != W.floats.end(), "%s: unknown buffer '%s'", who, buffer_name);
  const size_t have = it->second;
  SMI_REQUIRE(offset_floats <= have && floats <= have - offset_floats, "%s: %zu floats at %zu outside '%s' (%zu floats a row)", who, floats,
              offset_floats, buffer_name, have);
  float* p = W.at(row, buffer_name) + offset_floats;
  SMI_HIP(hipDeviceSynchronize());
  if (write) SMI_HIP(hipMemcpy(p, host_ptr, floats * 4, hipMemcpyHostToDevice));
  else SMI_HIP(hipMemcpy(host_ptr, p, floats * 4, hipMemcpyDeviceToHost));
  return SMI_OK;
}

int dbg_run(const smi_enc::Ws& W, const char* who, int first, int last, hipStream_t st) {
  SMI_REQUIRE(first >= 0 && first <= last && last < (int)W.prog.size(), "%s: launches %d..%d outside 0..%d", who, first, last,
              (int)W.prog.size() - 1);
  for (int i = first; i <= last; ++i) {
    const int rc = run_launch(W.prog[i], st);
    if (rc) return rc;
  }
  SMI_HIP(hipStreamSynchronize(st));
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_enc_debug_build(smi_enc* h, int n_samples, int n_ref, int* n_frames, int* n_launches, void* stream) {
  SMI_REQUIRE(h && n_frames && n_launches, "smi_enc_debug_build: null argument");
  h->prog_key = {-1, -1};
  const int32_t ns = n_samples, nr = n_ref;
  int32_t nf = 0;
  const int rc = dbg_build(h, h->solo, "smi_enc_debug_build", &ns, &nr, 1, &nf, n_launches, (hipStream_t)stream);
  *n_frames = nf;
  return rc;
}

int smi_enc_debug_launch(smi_enc* h, int index, char* name, int cap, int32_t* info) {
  SMI_REQUIRE(h, "smi_enc_debug_launch: null argument");
  return dbg_launch(h->solo, "smi_enc_debug_launch", index, name, cap, info);
}

int smi_enc_debug_io(smi_enc* h, const char* buffer_name, int write, void* host_ptr, size_t offset_floats, size_t floats) {
  SMI_REQUIRE(h, "smi_enc_debug_io: null argument");
  return dbg_io(h->solo, "smi_enc_debug_io", 0, buffer_name, write, host_ptr, offset_floats, floats);
}

int smi_enc_debug_run(smi_enc* h, int first, int last, void* stream) {
  SMI_REQUIRE(h, "smi_enc_debug_run: null handle");
  return dbg_run(h->solo, "smi_enc_debug_run", first, last, (hipStream_t)stream);
}

int smi_enc_rows_debug_build(smi_enc* h, const int32_t* n_samples, const int32_t* n_ref, int B, int32_t* n_frames, int* n_launches,
                             int32_t* run_start, int run_cap, int* n_runs, void* stream) {
  SMI_REQUIRE(h && n_samples && n_ref && n_frames && n_launches && n_runs, "smi_enc_rows_debug_build: null argument");
  const int rc = dbg_build(h, h->rows, "smi_enc_rows_debug_build", n_samples, n_ref, B, n_frames, n_launches, (hipStream_t)stream);
  if (rc) return rc;
  return smi_enc_rows_debug_runs(h, run_start, run_cap, n_runs, n_launches);
}

int smi_enc_rows_debug_runs(smi_enc* h, int32_t* run_start, int run_cap, int* n_runs, int* n_launches) {
  SMI_REQUIRE(h && n_runs && n_launches, "smi_enc_rows_debug_runs: null argument");
  *n_runs = (int)h->rows.run_start.size();
  *n_launches = (int)h->rows.prog.size();
  for (int i = 0; run_start && i < run_cap && i < *n_runs; ++i) run_start[i] = h->rows.run_start[i];
  return SMI_OK;
}

int smi_enc_rows_debug_launch(smi_enc* h, int index, char* name, int cap, int32_t* info) {
  SMI_REQUIRE(h, "smi_enc_rows_debug_launch: null argument");
  return dbg_launch(h->rows, "smi_enc_rows_debug_launch", index, name, cap, info);
}

int smi_enc_rows_debug_io(smi_enc* h, int row, const char* buffer_name, int write, void* host_ptr, size_t offset_floats, size_t floats) {
  SMI_REQUIRE(h, "smi_enc_rows_debug_io: null argument");
  return dbg_io(h->rows, "smi_enc_rows_debug_io", row, buffer_name, write, host_ptr, offset_floats, floats);
}

int smi_enc_rows_debug_run(smi_enc* h, int first, int last, void* stream) {
  SMI_REQUIRE(h, "smi_enc_rows_debug_run: null handle");
  return dbg_run(h->rows, "smi_enc_rows_debug_run", first, last, (hipStream_t)stream);
}

int smi_enc_rows_debug_stage(smi_enc* h, int row, const char* name, float* out_dev, size_t max_floats, int32_t* dims, void* stream) {
  SMI_REQUIRE(h, "smi_enc_rows_debug_stage: null argument");
  return enc_stage(h->rows, "smi_enc_rows_debug_stage", row, name, out_dev, max_floats, dims, stream);
}

}  // extern "C"

#endif   // SMI_DIAG
