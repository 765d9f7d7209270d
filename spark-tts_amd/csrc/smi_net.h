// smi_net.h -- what the BiCodec vocoder (smi_voc.hip) and the prompt encoder (smi_enc.hip) name of the conv / LayerNorm / codebook
// layer they share: the kernels' parameter structs, the launch record and its builders, the arena entry and conv geometry helpers.
// The kernels themselves, the table of their instantiations and the builders' definitions are one translation unit, smi_net.hip:
// a kernel is compiled once, whoever launches it.  The types cross translation units, so they live in a named namespace; its
// hidden visibility keeps every name of it out of the library's dynamic symbol table.
#pragma once
#include "smi_common.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>

namespace smi_net __attribute__((visibility("hidden"))) {

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_TANH = 2, ACT_RELU = 3, ACT_SIGMOID = 4 };
enum { PACK_RAW = 0, PACK_CONV = 1, PACK_CONVT = 2, PACK_CONV_B = 3, PACK_CONVT_B = 4 };   // _B: two bf16 planes (hi, mid) for k_convb
constexpr int kMaxTaps = 8;     // taps per phase
constexpr int kMaxPhases = 8;   // ConvTranspose1d stride
constexpr int kChunk = 32;      // input channels staged per LDS chunk

struct ConvP {
  const float* X;       // [B][Cin][xstride]
  const float* X2;      // second input added to X while staging (same strides; Res2Net branch sum) or null
  const float* W;       // packed, phase-major
  const float* bias;    // [Cout] or null
  const float* bbias;   // [B][Cout] per-utterance bias or null
  const float* gamma;   // [Cout] layer scale or null
  const float* beta;    // [Cout] shift after gamma (BatchNorm in eval mode: y = gamma * act(conv) + beta) or null
  const float* R;       // residual [B][Cout][ystride] or null (may alias Y)
  const float* alpha;   // [Cout] Snake alpha for Ys or null
  float* Y;             // raw output or null
  float* Ys;            // snake(Y, alpha) or null
  const int* lens;      // [B] valid INPUT lengths
  const int* olens;     // [B] valid OUTPUT positions per phase when they differ from lens (strided conv), or null
  int Cin, CinP, Cout, S, act;
  int xstride, ystride;
  long long xb, yb;     // batch strides (floats)
  int halo_l, xw;       // left halo, staged row width (floats)
  int istr;             // input stride of a strided Conv1d (1 otherwise): output q reads x[q * istr + tap]
  float out_scale;
  int fast_sin;         // Snake with the hardware sine (layers on the bf16-split pipe)
  int ntaps[kMaxPhases];
  int off[kMaxPhases][kMaxTaps];
  long long wphase[kMaxPhases];  // float offset of each phase's weights
};

__device__ __forceinline__ float gelu_f(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

// one fused ResidualUnit (k_resunit, smi_net.hip)
struct ResP {
  const float* Xs;      // snake(U, alpha0): [B][C][stride]
  const float* U;       // residual (raw), same layout
  const float* W7;      // conv7 weights, bf16 planes (PACK_CONV_B)
  const float* b7;
  const float* alpha2;  // Snake between the convs
  const float* W1;      // 1x1 weights, bf16 planes
  const float* b1;
  const float* alpha_next;   // Snake of the NEXT consumer (Ys) or null
  float* Y;             // raw output (may alias U) or null
  float* Ys;            // snake(Y, alpha_next) or null
  const int* lens;
  int C, stride;
  long long bs;
  int halo_l, xw;
  int off[kMaxTaps];
  int fast_sin;
};

// depthwise conv7 (optional) + LayerNorm / AdaLayerNorm over channels, eps 1e-6 (vocos.py:65-110)
struct LnP {
  const float* X;      // [B][C][stride]
  float* Y;
  const float* dww;    // [C][7] or null
  const float* dwb;    // [C]
  const float* w;      // LN weight [C] (plain) or null
  const float* bsh;    // LN bias [C]
  const float* ada;    // AdaLN: [B][ada_stride] with scale at +0, shift at +C; or null
  const int* lens;
  int C, stride, ada_stride;
  long long bs;
  int triple;          // 1: write 3x (SamplingBlock ratio 1 after final_layer_norm)
  float eps;           // 1e-6 (vocos), 1e-5 (wav2vec2)
  int gelu;            // 1: GELU(erf) after the affine (wav2vec2 feature-encoder layers)
};

// FSQ index -> level codes -> Linear(nd -> latent) (k_fsq, smi_net.hip)
struct FsqP {
  const int32_t* glob;  // [B][Ntok]
  const float* W1;      // [latent][nd]
  const float* b1;      // [latent]
  float* out;           // [B][latent*Ntok]
  int Ntok, latent, nd;
  int levels[8];
};

// ------------------------------------------------------------------------------------------
// arena description
// ------------------------------------------------------------------------------------------
struct Entry {
  std::string name;   // reference state_dict key (after remove_weight_norm); "cat:a|b|c" = rows concatenated
  int kind;           // PACK_*
  int Cout, Cin, K;   // logical dims (K taps)
  int S, pad;         // ConvTranspose1d stride / padding
  size_t offset, bytes;
};

struct ConvGeom {
  int S;
  int ntaps[kMaxPhases];
  int off[kMaxPhases][kMaxTaps];
  int tapk[kMaxPhases][kMaxTaps];   // kernel index j of each (phase, tap)
  long long wphase[kMaxPhases];
  int halo_l, halo_r;
  long long floats;
};

inline int pad8(int c) { return (c + 7) / 8 * 8; }
inline int pad32(int c) { return (c + 31) / 32 * 32; }

// Conv1d (S = 1): tap j reads x[t + j*dil - pad].  ConvTranspose1d (stride S, padding pad):
// out[q*S + r] += W[ci][co][j] * x[ci][(q*S + r + pad - j)/S] for j == (r + pad) mod S.
ConvGeom conv_geom(int Cout, int Cin, int K, int dil, int pad, int S, bool bf = false);

// ------------------------------------------------------------------------------------------
// The kernel form of a conv launch: which instantiation of k_conv / k_convb / k_convbT / k_conv_c1 / k_gemv1 runs it.
// kConvForms (smi_net.hip) is the ONE list of instantiations; make_conv() is the ONE place where a layer, a plan shape and, in
// the diagnostics build, the SPARKMI_* A/B switches become an index into it.  run_launch() dispatches on that index, and the
// diagnostics entry points (include/sparkmi_debug.h) enumerate the same table and copy the same record, so the list of forms a
// test covers and the launches cannot diverge.
// ------------------------------------------------------------------------------------------
enum { CONV_K_CONV = 0, CONV_K_CONVB = 1, CONV_K_CONVBT = 2, CONV_K_C1 = 3, CONV_K_GEMV = 4 };
struct ConvForm {
  int kernel;   // CONV_K_*
  int qb;       // 32-column time sub-tiles per wave
  int ks;       // waves split the input channels of one output tile
  int chg;      // a staged chunk holds 32 * chg input channels
  int nc;       // the staged row is up to 64 * nc columns wide
  int nwv;      // waves per block
  int wpf;      // one-tap layers on a small grid: weights requested one chunk ahead
  int wall;     // several taps on a small grid: all taps' weights of a chunk requested together
  int tph;      // k_convbT: output phases per block (k_conv_c1: its taps)
};
inline bool operator==(const ConvForm& a, const ConvForm& b) {
  return a.kernel == b.kernel && a.qb == b.qb && a.ks == b.ks && a.chg == b.chg && a.nc == b.nc && a.nwv == b.nwv && a.wpf == b.wpf &&
         a.wall == b.wall && a.tph == b.tph;
}

// the table of instantiations the library carries (kConvForms, smi_net.hip), in the enumeration order of smi_conv_form_get
int conv_form_count();
const ConvForm& conv_form_at(int index);
int conv_form_index(const ConvForm& f);   // -1: no such instantiation

// What make_conv() chose for a conv launch from its PLAN shape.  plan_signature() compares the whole record, so a choice added
// here separates rows without further ado; in return the record holds ints only, each a function of the layer and the plan
// shape and never of the extent (the grid's x and z and plan_blocks stand in the Launch).
struct ConvPlan {
  int form;                     // index in kConvForms (-1: no instantiation; check_conv refuses the launch)
  int qb, ks, chg, nwv, tph;    // the MFMA tile choices; a gemv / c1 launch keeps those of its layer (run boundaries depend on them)
  int xw;                       // staged row width (= cp.xw)
  int tiles_y;                  // grid.y of an MFMA form (0: gemv and c1 size their grids from the extent alone)
  int small;                    // an MFMA form planned on at most 512 blocks (WPF and WALL depend on it)
};

struct Launch {
  int kind;          // 0 conv, 1 dwln, 2 codebook, 3 fsq, 4 zero-tail, 5 fused ResidualUnit, 9 closure (fn)
  std::function<void(hipStream_t)> fn;
  std::string name;
  double flops;
  dim3 grid; size_t lds;
  int blk = 0;       // kinds 0 and 9: threads per block (with grid and lds: what the launch runs with and the diagnostics report)
  ConvP cp; ConvPlan plan;     // kind 0, as make_conv() left them
  long long plan_blocks = 0;   // kind 0: blocks of the grid the plan was chosen for (with a PlanShape: not the launch's own grid)
  ResP rp; int res_nwv = 0;   // kind 5: a fused ResidualUnit (k_resunit) with res_nwv waves per block
  LnP lp; int cpt;
  // small kernels keep their args here
  const int64_t* sem; int semstride; const float* cb; int D, cbsize; float* Z; int zstride; long long zb;
  FsqP fp; int B;
  float* wav; int wstride, hop, tmaxhop;
  const int* lens;
};

// the k_dwln instantiation (channels per thread) that covers a layer of ceil(C / 32) channels per thread
inline int dwln_form(int cpt) { return cpt <= 2 ? 2 : (cpt <= 4 ? 4 : (cpt <= 12 ? 12 : (cpt <= 16 ? 16 : 32))); }

int run_launch(const Launch& L, hipStream_t st);

// The shape a launch plan is chosen for where that is not the call's own (smi_voc_forward_rows): ONE row of `frames` frames, in a
// call whose grids cover rows of up to `ext_frames` frames.  A layer that works at Lmax = up * ext_frames positions plans for
// up * frames (the per-utterance vector projections, Lmax = 1, for 1).  Where a layer's length is no multiple of a frame count (the
// prompt encoder: the strided convs' output lengths, mel frames, perceiver keys) the builder names the plan row's length of that
// very layer in plan_len, and nothing is derived.
struct PlanShape {
  int frames, ext_frames;
  int plan_len = 0;     // > 0: the plan row's length at this launch, as given
  int len(int Lmax) const { return plan_len > 0 ? plan_len : (Lmax % ext_frames == 0 ? Lmax / ext_frames * frames : Lmax); }
};

// One conv launch, field by field.  Strides are in floats; Lmax = padded OUTPUT positions per phase (the input length of a
// stride-1 or transposed conv).  The call shape (B, Lmax) plays two roles: the PLAN shape picks tile width, channel split, wave
// count, chunk size and kernel form -- the summation order -- and the EXTENT sizes the grid.  With `ps` the plan is that of ps's
// one row and only the extent comes from (B, Lmax): blocks beyond a row's own length exit, so every row carries the bits of its
// plan shape.
enum { CONV_MFMA = 0, CONV_GEMV = 1, CONV_C1 = 2 };
struct ConvSpec {
  std::string name;
  int Cout = 0, Cin = 0, K = 1, dil = 1, S = 1, pad = 0, istr = 1;   // S > 1: ConvTranspose1d; istr > 1: strided Conv1d
  bool bf = false;        // the weights are two bf16 planes (PACK_CONV_B / PACK_CONVT_B): the layer runs on k_convb / k_convbT
  const float* W = nullptr; const float* bias = nullptr;
  const float* X = nullptr; const float* X2 = nullptr; int xstride = 0; long long xb = 0;
  float* Y = nullptr; float* Ys = nullptr; const float* alpha = nullptr; const float* R = nullptr; int ystride = 0; long long yb = 0;
  const int* lens = nullptr; const int* olens = nullptr; int B = 1, Lmax = 1, act = ACT_NONE;
  const float* bbias = nullptr; const float* gamma = nullptr; const float* beta = nullptr; float out_scale = 1.0f;
  int want = CONV_MFMA;   // CONV_GEMV: one vector per utterance (k_gemv1); CONV_C1: k_conv_c1 where the layer qualifies, else as CONV_MFMA
  const PlanShape* ps = nullptr;
};
// The launch as it runs: form, grid, block, LDS, xw and plan_blocks are final; nobody assigns a field of it afterwards.
Launch make_conv(const ConvSpec& s);
// What a conv launch must satisfy before it runs: weights, a kernel form, the LDS limit, the staged width, k_convbT's epilogue.
int check_conv(const Launch& L, const char* who);

// Every choice a launch list makes from its plan shape, launch by launch: two rows may share a launch sequence when these agree.
std::vector<long long> plan_signature(const std::vector<Launch>& P);

// Run boundaries of a call's rows: consecutive rows with equal plan signatures form a run.  {first row of every run ..., rows}.
inline std::vector<int> plan_runs(const std::vector<const std::vector<long long>*>& sig) {
  std::vector<int> runs;
  for (size_t r = 0; r < sig.size(); ++r)
    if (r == 0 || *sig[r] != *sig[runs.back()]) runs.push_back((int)r);
  runs.push_back((int)sig.size());
  return runs;
}

// One launch timed alone: once to warm, then `iters` times between two events (smi_voc_time_launch, smi_enc_time_launch).
int time_launch(const Launch& L, hipEvent_t ev0, hipEvent_t ev1, int iters, float* ms_avg, double* flops, char* name, int name_cap,
                hipStream_t st);

}  // namespace smi_net
