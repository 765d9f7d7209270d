// smi_voc.hip -- BiCodec vocoder (detokenize path) for gfx950 (MI355X).
//
// Stands behind BiCodec.detokenize (sparktts/models/bicodec.py:171-189):
//   quantizer.detokenize        sparktts/modules/vq/factorized_vector_quantize.py:154-167
//   speaker_encoder.detokenize  sparktts/modules/speaker/speaker_encoder.py:107-112,
//                               fsq/residual_fsq.py:112-199, fsq/finite_scalar_quantization.py:143-162
//   prenet (Decoder)            sparktts/modules/encoder_decoder/feat_decoder.py:78-94,
//                               blocks/vocos.py:65-110,324-335, blocks/samper.py:79-100 (ratio 1 => 3x)
//   decoder (WaveGenerator)     sparktts/modules/encoder_decoder/wave_generator.py:29-88,
//                               blocks/layers.py:33-67 (snake, ResidualUnit)
//
// Every dense contraction (Linear, Conv1d incl. dilated, ConvTranspose1d as polyphase taps) runs
// through ONE implicit-GEMM kernel on the exact-fp32 matrix pipe (v_mfma_f32_32x32x2_f32: the
// reference computes in fp32 and the parity bar is 1e-3 on the waveform).  Activations are
// [B][C][T] fp32 with time contiguous; input tiles (+halo) are staged through LDS once per
// 32-channel chunk and re-read per tap; weights are pre-packed in MFMA A-operand order so each
// lane streams float4s.  Elementwise work is fused into the producing kernel's epilogue: bias,
// per-utterance bias (d-vector), layer-scale, residual add, GELU / tanh, and the *next* layer's
// Snake activation (written as a second output), so no standalone elementwise kernel exists.
// Ragged batches: every kernel masks loads beyond the row's own length, so each row equals an
// un-padded B=1 run of that row.
#include "smi_net.h"
#include <algorithm>
#include <map>

using namespace smi_net;

namespace {

struct VocLayout {
  std::vector<Entry> e;
  size_t total;
};

bool voc_cfg_ok(const smi_voc_cfg* c) {
  if (!c) return false;
  if (c->vq_input_dim <= 0 || c->codebook_size <= 0 || c->codebook_dim <= 0) return false;
  if (c->fsq_dims < 1 || c->fsq_dims > 8 || c->spk_token_num < 1 || c->spk_latent_dim < 1) return false;
  if (c->pre_dim < 1 || c->pre_dim > 512 || c->pre_layers < 1 || c->pre_num_down < 0 || c->pre_num_down > 4) return false;
  if (c->pre_out_channels != c->dec_in || c->spk_out_dim != c->dec_in || c->pre_input_channels != c->vq_input_dim) return false;
  if (c->pre_cond_dim != c->spk_out_dim) return false;
  if (c->dec_nblocks < 1 || c->dec_nblocks > 8 || c->dec_channels >> c->dec_nblocks < 1) return false;
  for (int i = 0; i < c->dec_nblocks; ++i) {
    const int k = c->dec_ksizes[i], s = c->dec_rates[i];
    if (s < 1 || s > kMaxPhases || k < s || (k - s) % 2 || (k + s - 1) / s > kMaxTaps) return false;
  }
  if (c->max_batch < 1 || c->max_frames < 1) return false;
  return true;
}

VocLayout voc_layout(const smi_voc_cfg* c) {
  VocLayout L;
  size_t o = 0;
  auto add = [&](const std::string& name, int kind, int Cout, int Cin, int K, int S, int pad, size_t floats) {
    Entry e{name, kind, Cout, Cin, K, S, pad, o, floats * 4};
    L.e.push_back(e);
    o += smi_align_up(floats * 4, 256);
  };
  auto raw = [&](const std::string& name, size_t n) { add(name, PACK_RAW, 0, 0, 0, 1, 0, n); };
  // conv: layers of the dense stack -- on the bf16-split matrix pipe (k_convb, two bf16 weight planes) unless the handle is
  // created with exact_fp32, or the layer is too thin to fill a 16-channel step / 32-row tile; convf: always exact fp32
  // (the per-utterance GEMVs read the fp32 packing; the 8-channel codebook projection; the one-channel output conv)
  auto convf = [&](const std::string& name, int Cout, int Cin, int K) {
    add(name, PACK_CONV, Cout, Cin, K, 1, 0, (size_t)conv_geom(Cout, Cin, K, 1, 0, 1).floats);
  };
  auto use_bf = [&](int Cout, int Cin) { return !c->exact_fp32 && Cin >= 32 && Cout >= 32; };
  auto conv = [&](const std::string& name, int Cout, int Cin, int K) {
    const bool bf = use_bf(Cout, Cin);
    add(name, bf ? PACK_CONV_B : PACK_CONV, Cout, Cin, K, 1, 0, (size_t)conv_geom(Cout, Cin, K, 1, 0, 1, bf).floats);
  };
  const int D = c->pre_dim, I = c->pre_inter, Cc = c->pre_cond_dim;
  raw("quantizer.codebook.weight", (size_t)c->codebook_size * c->codebook_dim);
  convf("quantizer.out_project.weight", c->vq_input_dim, c->codebook_dim, 1);
  raw("quantizer.out_project.bias", c->vq_input_dim);
  raw("speaker_encoder.quantizer.project_out.weight", (size_t)c->spk_latent_dim * c->fsq_dims);
  raw("speaker_encoder.quantizer.project_out.bias", c->spk_latent_dim);
  convf("speaker_encoder.project.weight", c->spk_out_dim, c->spk_latent_dim * c->spk_token_num, 1);
  raw("speaker_encoder.project.bias", c->spk_out_dim);
  conv("prenet.linear_pre.weight", D, c->pre_input_channels, 1);
  raw("prenet.linear_pre.bias", D);
  std::string adaw = "cat:", adab = "cat:";
  auto vocos = [&](const std::string& p, int nl, bool ada) {
    conv(p + ".embed.weight", D, D, 7);
    raw(p + ".embed.bias", D);
    auto norm = [&](const std::string& n) {
      if (ada) {
        adaw += (adaw.size() > 4 ? "|" : "") + n + ".scale.weight|" + n + ".shift.weight";
        adab += (adab.size() > 4 ? "|" : "") + n + ".scale.bias|" + n + ".shift.bias";
      } else {
        raw(n + ".weight", D);
        raw(n + ".bias", D);
      }
    };
    norm(p + ".norm");
    for (int j = 0; j < nl; ++j) {
      const std::string b = p + ".convnext." + std::to_string(j);
      raw(b + ".dwconv.weight", (size_t)D * 7);
      raw(b + ".dwconv.bias", D);
      norm(b + ".norm");
      conv(b + ".pwconv1.weight", I, D, 1);
      raw(b + ".pwconv1.bias", I);
      conv(b + ".pwconv2.weight", D, I, 1);
      raw(b + ".pwconv2.bias", D);
      raw(b + ".gamma", D);
    }
    raw(p + ".final_layer_norm.weight", D);
    raw(p + ".final_layer_norm.bias", D);
  };
  for (int i = 0; i < c->pre_num_down; ++i) vocos("prenet.downsample." + std::to_string(i) + ".1", 2, false);
  vocos("prenet.vocos_backbone", c->pre_layers, true);
  const int nada = 1 + c->pre_layers;
  convf(adaw, nada * 2 * D, Cc, 1);
  raw(adab, (size_t)nada * 2 * D);
  conv("prenet.linear.weight", c->pre_out_channels, D, 1);
  raw("prenet.linear.bias", c->pre_out_channels);
  int ch = c->dec_channels;
  conv("decoder.model.0.weight", ch, c->dec_in, 7);
  raw("decoder.model.0.bias", ch);
  for (int i = 0; i < c->dec_nblocks; ++i) {
    const int cin = ch >> i, cout = ch >> (i + 1), k = c->dec_ksizes[i], s = c->dec_rates[i];
    const std::string b = "decoder.model." + std::to_string(i + 1) + ".block";
    raw(b + ".0.alpha", cin);
    add(b + ".1.weight", use_bf(cout, cin) ? PACK_CONVT_B : PACK_CONVT, cout, cin, k, s, (k - s) / 2,
        (size_t)conv_geom(cout, cin, k, 1, (k - s) / 2, s, use_bf(cout, cin)).floats);
    raw(b + ".1.bias", cout);
    for (int r = 0; r < 3; ++r) {
      const std::string u = b + "." + std::to_string(r + 2) + ".block";
      raw(u + ".0.alpha", cout);
      conv(u + ".1.weight", cout, cout, 7);
      raw(u + ".1.bias", cout);
      raw(u + ".2.alpha", cout);
      conv(u + ".3.weight", cout, cout, 1);
      raw(u + ".3.bias", cout);
    }
  }
  const int clast = ch >> c->dec_nblocks;
  raw("decoder.model." + std::to_string(c->dec_nblocks + 1) + ".alpha", clast);
  convf("decoder.model." + std::to_string(c->dec_nblocks + 2) + ".weight", 1, clast, 7);
  raw("decoder.model." + std::to_string(c->dec_nblocks + 2) + ".bias", 1);
  L.total = o;
  return L;
}

}  // namespace

struct smi_voc {
  smi_voc_cfg cfg;
  VocLayout lay;
  const unsigned char* arena;
  DevBuf<float> buf[4];   // activation ping-pong buffers [max_batch][maxC x maxL]
  size_t buf_floats;      // per batch item
  DevBuf<float> small;    // d-vector path + AdaLN params
  DevBuf<int> lens_dev;   // [8][max_batch] valid lengths per resolution
  DevBuf<float> dbg[8]; size_t dbg_floats[8]; int debug;
  std::vector<Launch> prog;
  std::vector<int32_t> host_lens;   // staging for the async H2D copy (must outlive the call)
  int lastB, lastT;
  hipEvent_t ev0, ev1;
};

namespace {

// Where a group of launches finds its packed weights: a table of entries (the vocoder's arena, or one block's -- smi_voc_block_*)
struct WSrc {
  const std::vector<Entry>* e;
  const unsigned char* arena;
  const float* get(const std::string& name) const {
    for (const Entry& x : *e)
      if (x.name == name) return (const float*)(arena + x.offset);
    return nullptr;
  }
  bool is_bf(const std::string& name) const {
    for (const Entry& x : *e)
      if (x.name == name) return x.kind == PACK_CONV_B || x.kind == PACK_CONVT_B;
    return false;
  }
};
WSrc wsrc(const smi_voc* h) { return WSrc{&h->lay.e, h->arena}; }
const float* ent(const smi_voc* h, const std::string& name) { return wsrc(h).get(name); }

// The spec of a layer on [C][L] activations: weights and bias by arena name, input and output with row stride L and batch stride
// bs, B rows of at most L positions.  The caller names the layer's shape and its operands (and any stride that differs).
ConvSpec layer(const WSrc& w, const std::string& name, const std::string& wname, const std::string& bname, int L, long long bs,
               const int* lens, int B, const PlanShape* ps) {
  ConvSpec s;
  s.name = name; s.W = w.get(wname); s.bias = w.get(bname); s.bf = w.is_bf(wname);
  s.xstride = s.ystride = L; s.xb = s.yb = bs; s.lens = lens; s.B = B; s.Lmax = L; s.ps = ps;
  return s;
}

// ---- launch builders shared by smi_voc_forward and the one-block entry points (smi_voc_block_run): the same kernels,
//      the same launch geometry, the same fusions

// ResidualUnit (blocks/layers.py:51-67): y = x + conv1(snake(conv7_dil(snake(x)))).  US holds snake(U, <u>.0.alpha) -- the
// producer's second output; conv7's epilogue applies the unit's second Snake (-> A); the 1x1 adds the residual U and writes
// the new U to `rawout` (may be null) and, if `want_us`, snake(new U, next_alpha) over US (in place: the 7-tap conv has finished
// with it).  The fused form (k_resunit, below) cannot write over US -- a block's neighbours still read their halo columns from it --
// and leaves the Snake'd output in A, which it does not otherwise need.  Returns the buffer that holds it (null: none asked for).
float* add_res_unit(std::vector<Launch>& P, const WSrc& w, const std::string& u, int C, int dil, const float* U, float* US,
                    float* A, float* rawout, bool want_us, const float* next_alpha, int L, long long bs, const int* lens, int B,
                    const PlanShape* ps = nullptr) {
  float* US_out = want_us ? US : nullptr;
  ConvSpec s7 = layer(w, u + ".conv7", u + ".1.weight", u + ".1.bias", L, bs, lens, B, ps);
  s7.Cout = s7.Cin = C; s7.K = 7; s7.dil = dil; s7.pad = 3 * dil; s7.X = US; s7.Ys = A; s7.alpha = w.get(u + ".2.alpha");
  ConvSpec s1 = layer(w, u + ".conv1+res", u + ".3.weight", u + ".3.bias", L, bs, lens, B, ps);
  s1.Cout = s1.Cin = C; s1.X = A; s1.Y = rawout; s1.Ys = US_out; s1.alpha = next_alpha; s1.R = U;
  const Launch c7 = make_conv(s7), c1 = make_conv(s1);
  // C = 96 / 192 on the bf16-split pipe with one output tile per wave (not the channel-split mode of short sequences): the two
  // launches become one k_resunit (SPARKMI_RESFUSE=0: two launches, A/B).  The choice depends on the layer and on whether the
  // grid fills the chip, as every launch plan does -- never on a row's neighbours.
  const char* e = smi_env("SPARKMI_RESFUSE");
  if ((C == 96 || C == 192) && s7.bf && s1.bf && !c7.plan.ks && !c1.plan.ks && s7.W && s1.W && s7.bias && s1.bias && s7.alpha &&
      c7.plan.xw <= 128 && !(e && e[0] == '0')) {
    Launch F; F.kind = 5; F.name = u + ".conv7+conv1+res"; F.flops = c7.flops + c1.flops; F.res_nwv = C / 32;
    ResP& r = F.rp; memset(&r, 0, sizeof(r));
    r.Xs = US; r.U = U; r.W7 = c7.cp.W; r.b7 = c7.cp.bias; r.alpha2 = c7.cp.alpha; r.W1 = c1.cp.W; r.b1 = c1.cp.bias;
    r.alpha_next = want_us ? next_alpha : nullptr; r.Y = rawout; r.Ys = want_us ? A : nullptr; r.lens = lens; r.C = C; r.stride = L; r.bs = bs;
    r.halo_l = c7.cp.halo_l; r.xw = c7.cp.xw; r.fast_sin = c7.cp.fast_sin;
    for (int i = 0; i < 7; ++i) r.off[i] = c7.cp.off[0][i];
    F.grid = dim3((L + 63) / 64, 1, B);
    const size_t stage = (size_t)2 * 6 * r.xw * 16, image = (size_t)2 * (C / 8) * 64 * 16;
    F.lds = stage > image ? stage : image;
    P.push_back(F);
    return F.rp.Ys;
  }
  P.push_back(c7);
  P.push_back(c1);
  return US_out;
}

// DecoderBlock (encoder_decoder/wave_generator.py:29-53) on s_in = snake(x, <b>.0.alpha) (left by the producer):
// ConvTranspose1d (polyphase) -> U raw, US = snake(U, unit 2's first alpha); three ResidualUnits (dilation 1, 3, 9).
// The last unit writes its raw output to `raw_final` (may be null) and snake(., next_alpha) (next_alpha may be null) to US or A:
// the function returns which (a fused unit flips the two; see add_res_unit).
float* add_dec_block(std::vector<Launch>& P, const WSrc& w, const std::string& b, int cin, int cout, int k, int s, const float* s_in,
                   int Lin, long long bs_in, float* U, float* US, float* A, float* raw_final, const float* next_alpha, long long bs,
                   const int* lens_in, const int* lens_out, int B, const PlanShape* ps = nullptr) {
  const int Lout = Lin * s;
  ConvSpec t = layer(w, b + ".convT", b + ".1.weight", b + ".1.bias", Lin, bs_in, lens_in, B, ps);
  t.Cout = cout; t.Cin = cin; t.K = k; t.S = s; t.pad = (k - s) / 2; t.X = s_in; t.Y = U; t.Ys = US; t.alpha = w.get(b + ".2.block.0.alpha");
  t.ystride = Lout; t.yb = bs;
  P.push_back(make_conv(t));
  for (int r = 0; r < 3; ++r) {
    const std::string u = b + "." + std::to_string(r + 2) + ".block";
    const int dil = r == 0 ? 1 : (r == 1 ? 3 : 9);
    const bool last = r == 2;
    const float* na = last ? next_alpha : w.get(b + "." + std::to_string(r + 3) + ".block.0.alpha");
    float* out = add_res_unit(P, w, u, cout, dil, U, US, A, last ? raw_final : U, !(last && !next_alpha), na, Lout, bs, lens_out, B, ps);
    if (out && out != US) { A = US; US = out; }   // the Snake'd stream now lives in the other buffer; the old one is the next unit's scratch
  }
  return US;
}

// LayerNorm / AdaLayerNorm over channels, optionally behind the depthwise conv7 of a ConvNeXt block (k_dwln)
void add_lnorm(std::vector<Launch>& P, const WSrc& w, const std::string& name, const std::string& pfx, const float* ada, int ada_stride,
               const float* dww, const float* dwb, const float* X, float* Y, int triple, int D, int T, long long bs, const int* lens, int B) {
  Launch L; L.kind = 1; L.name = name; L.flops = (dww ? 14.0 : 0.0) * D * T * B + 8.0 * D * T * B;
  LnP& p = L.lp; memset(&p, 0, sizeof(p));
  p.X = X; p.Y = Y; p.dww = dww; p.dwb = dwb; p.lens = lens; p.C = D; p.stride = T; p.bs = bs; p.triple = triple;
  p.eps = 1e-6f;
  if (ada) { p.ada = ada; p.ada_stride = ada_stride; }
  else { p.w = w.get(pfx + ".weight"); p.bsh = w.get(pfx + ".bias"); }
  L.cpt = (D + 31) / 32; L.grid = dim3((T + 7) / 8, B);
  P.push_back(L);
}

// ConvNeXtBlock (blocks/vocos.py:26-62): x += gamma * pwconv2(GELU(pwconv1(norm(dwconv7(x))))); n, m: scratch
void add_convnext(std::vector<Launch>& P, const WSrc& w, const std::string& b, int D, int I, float* x, float* n, float* m,
                  const float* ada, int ada_stride, int T, long long bs, const int* lens, int B, const PlanShape* ps = nullptr) {
  add_lnorm(P, w, b + ".dwconv+norm", b + ".norm", ada, ada_stride, w.get(b + ".dwconv.weight"), w.get(b + ".dwconv.bias"), x, n, 0, D, T, bs, lens, B);
  ConvSpec p1 = layer(w, b + ".pwconv1", b + ".pwconv1.weight", b + ".pwconv1.bias", T, bs, lens, B, ps);
  p1.Cout = I; p1.Cin = D; p1.X = n; p1.Y = m; p1.act = ACT_GELU;
  P.push_back(make_conv(p1));
  ConvSpec p2 = layer(w, b + ".pwconv2", b + ".pwconv2.weight", b + ".pwconv2.bias", T, bs, lens, B, ps);
  p2.Cout = D; p2.Cin = I; p2.X = m; p2.Y = x; p2.R = x; p2.gamma = w.get(b + ".gamma");
  P.push_back(make_conv(p2));
}

// every conv launch of a list against check_conv (smi_net.h)
int check_launches(const std::vector<Launch>& P, const char* who) {
  int rc = SMI_OK;
  for (size_t i = 0; i < P.size() && rc == SMI_OK; ++i)
    if (P[i].kind == 0) rc = check_conv(P[i], who);
  return rc;
}

// ---- one reference block as its own little arena (smi_voc_block_*: op-level tests on the reference's layer classes)
bool block_cfg_ok(const smi_voc_block_cfg* c) {
  if (!c) return false;
  switch (c->kind) {
    case SMI_VOC_BLOCK_RESUNIT: return c->C >= 1 && c->C <= 4096 && (c->dil == 1 || c->dil == 3 || c->dil == 9);
    case SMI_VOC_BLOCK_DECBLOCK:
      return c->C >= 1 && c->Cout >= 1 && c->C <= 4096 && c->Cout <= 4096 && c->S >= 1 && c->S <= kMaxPhases && c->K >= c->S &&
             (c->K - c->S) % 2 == 0 && (c->K + c->S - 1) / c->S <= kMaxTaps;
    case SMI_VOC_BLOCK_CONVNEXT: return c->C >= 1 && c->C <= 512 && c->I >= 1 && c->I <= 8192 && c->cond_dim >= 0 && c->cond_dim <= 4096;
  }
  return false;
}

VocLayout block_layout(const smi_voc_block_cfg* c) {
  VocLayout L;
  size_t o = 0;
  auto add = [&](const std::string& name, int kind, int Cout, int Cin, int K, int S, int pad, size_t floats) {
    Entry e{name, kind, Cout, Cin, K, S, pad, o, floats * 4};
    L.e.push_back(e);
    o += smi_align_up(floats * 4, 256);
  };
  auto raw = [&](const std::string& name, size_t n) { add(name, PACK_RAW, 0, 0, 0, 1, 0, n); };
  auto use_bf = [&](int Cout, int Cin) { return !c->exact_fp32 && Cin >= 32 && Cout >= 32; };   // the vocoder's own rule (voc_layout)
  auto conv = [&](const std::string& name, int Cout, int Cin, int K) {
    const bool bf = use_bf(Cout, Cin);
    add(name, bf ? PACK_CONV_B : PACK_CONV, Cout, Cin, K, 1, 0, (size_t)conv_geom(Cout, Cin, K, 1, 0, 1, bf).floats);
  };
  auto unit = [&](const std::string& u, int C) {
    raw(u + ".0.alpha", C);
    conv(u + ".1.weight", C, C, 7);
    raw(u + ".1.bias", C);
    raw(u + ".2.alpha", C);
    conv(u + ".3.weight", C, C, 1);
    raw(u + ".3.bias", C);
  };
  if (c->kind == SMI_VOC_BLOCK_RESUNIT) {
    unit("L.block", c->C);
  } else if (c->kind == SMI_VOC_BLOCK_DECBLOCK) {
    raw("L.block.0.alpha", c->C);
    const bool bf = use_bf(c->Cout, c->C);
    add("L.block.1.weight", bf ? PACK_CONVT_B : PACK_CONVT, c->Cout, c->C, c->K, c->S, (c->K - c->S) / 2,
        (size_t)conv_geom(c->Cout, c->C, c->K, 1, (c->K - c->S) / 2, c->S, bf).floats);
    raw("L.block.1.bias", c->Cout);
    for (int r = 0; r < 3; ++r) unit("L.block." + std::to_string(r + 2) + ".block", c->Cout);
  } else {
    const int D = c->C;
    raw("L.dwconv.weight", (size_t)D * 7);
    raw("L.dwconv.bias", D);
    if (c->cond_dim > 0) {
      add("cat:L.norm.scale.weight|L.norm.shift.weight", PACK_CONV, 2 * D, c->cond_dim, 1, 1, 0, (size_t)conv_geom(2 * D, c->cond_dim, 1, 1, 0, 1).floats);
      raw("cat:L.norm.scale.bias|L.norm.shift.bias", (size_t)2 * D);
    } else {
      raw("L.norm.weight", D);
      raw("L.norm.bias", D);
    }
    conv("L.pwconv1.weight", c->I, D, 1);
    raw("L.pwconv1.bias", c->I);
    conv("L.pwconv2.weight", D, c->I, 1);
    raw("L.pwconv2.bias", D);
    raw("L.gamma", D);
  }
  L.total = o;
  return L;
}

// The launch list of one block on the working buffers of smi_voc_block_run: [0] input / x, [1] snake(input) / n, [2] U or m,
// [3] US, [4] A; lens = {lens_in[64], lens_out[64], ones[64]}.  Returns the buffer that holds the block's output.  Host only
// (smi_voc_block_plan builds the same list on placeholder pointers to report its kernel forms).
float* block_program(std::vector<Launch>& P, const smi_voc_block_cfg& c, const WSrc& w, float* const buf[5], float* ada, const float* cond_dev,
                     const int* lens, long long bs, int B, int L) {
  const int* lens_in = lens; const int* lens_out = lens + 64; const int* len1 = lens + 128;
  if (c.kind == SMI_VOC_BLOCK_RESUNIT) {
    add_res_unit(P, w, "L.block", c.C, c.dil, buf[0], buf[1], buf[4], buf[2], false, nullptr, L, bs, lens_in, B);
    return buf[2];
  }
  if (c.kind == SMI_VOC_BLOCK_DECBLOCK) {
    add_dec_block(P, w, "L.block", c.C, c.Cout, c.K, c.S, buf[1], L, bs, buf[2], buf[3], buf[4], buf[0], nullptr, bs, lens_in, lens_out, B);
    return buf[0];
  }
  if (c.cond_dim > 0) {   // all scale / shift projections of the condition in one GEMV (vocos.py:105-108), as smi_voc_forward does
    ConvSpec a = layer(w, "adaln_params", "cat:L.norm.scale.weight|L.norm.shift.weight", "cat:L.norm.scale.bias|L.norm.shift.bias", 1, 0, len1, B, nullptr);
    a.Cout = 2 * c.C; a.Cin = c.cond_dim; a.X = cond_dev; a.xb = c.cond_dim; a.Y = ada; a.yb = 2 * c.C; a.want = CONV_GEMV;
    P.push_back(make_conv(a));
  }
  add_convnext(P, w, "L", c.C, c.I, buf[0], buf[1], buf[2], c.cond_dim > 0 ? ada : nullptr, 2 * c.C, L, bs, lens_in, B);
  return buf[0];
}

int layout_entry(const VocLayout& L, int index, char* name, int name_cap, size_t* offset, size_t* bytes, int32_t* info, const char* who) {
  SMI_REQUIRE(index >= 0 && index < (int)L.e.size(), "%s: index %d out of range", who, index);
  const Entry& e = L.e[index];
  SMI_REQUIRE(name && name_cap > (int)e.name.size(), "%s: name buffer too small (%zu needed)", who, e.name.size() + 1);
  strcpy(name, e.name.c_str());
  if (offset) *offset = e.offset;
  if (bytes) *bytes = e.bytes;
  if (info) { info[0] = e.kind; info[1] = e.Cout; info[2] = e.Cin; info[3] = e.K; info[4] = e.S; info[5] = e.pad; }
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_voc_arena_count(const smi_voc_cfg* cfg) {
  if (!voc_cfg_ok(cfg)) return 0;
  return (int)voc_layout(cfg).e.size();
}

size_t smi_voc_arena_bytes(const smi_voc_cfg* cfg) {
  if (!voc_cfg_ok(cfg)) return 0;
  return voc_layout(cfg).total;
}

int smi_voc_arena_entry(const smi_voc_cfg* cfg, int index, char* name, int name_cap, size_t* offset, size_t* bytes,
                        int32_t* info) {
  SMI_REQUIRE(voc_cfg_ok(cfg), "smi_voc_arena_entry: config outside the kernel contract");
  return layout_entry(voc_layout(cfg), index, name, name_cap, offset, bytes, info, "smi_voc_arena_entry");
}

int smi_voc_create(const smi_voc_cfg* cfg, const void* arena_dev, size_t arena_bytes, smi_voc** out) {
  SMI_REQUIRE(out, "smi_voc_create: out is null");
  *out = nullptr;
  SMI_REQUIRE(voc_cfg_ok(cfg), "smi_voc_create: config outside the kernel contract");
  VocLayout lay = voc_layout(cfg);
  SMI_REQUIRE(arena_dev && arena_bytes >= lay.total, "smi_voc_create: arena too small (%zu < %zu)", arena_bytes, lay.total);
  SMI_REQUIRE(((uintptr_t)arena_dev & 255) == 0, "smi_voc_create: arena must be 256-byte aligned");
  smi_voc* h = new smi_voc();
  h->cfg = *cfg; h->lay = lay; h->arena = (const unsigned char*)arena_dev;
  const char* dbg = smi_env("SPARKMI_VOC_DEBUG");
  h->debug = dbg && dbg[0] == '1';
  // largest activation: channels x length over all stages
  size_t mx = (size_t)cfg->vq_input_dim * cfg->max_frames;
  mx = std::max(mx, (size_t)cfg->pre_inter * cfg->max_frames);
  mx = std::max(mx, (size_t)cfg->dec_channels * cfg->max_frames);
  size_t len = cfg->max_frames;
  for (int i = 0; i < cfg->dec_nblocks; ++i) {
    len *= cfg->dec_rates[i];
    mx = std::max(mx, (size_t)(cfg->dec_channels >> (i + 1)) * len);
  }
  h->buf_floats = smi_align_up(mx, 64);
  const size_t small_floats = (size_t)cfg->max_batch *
      ((size_t)cfg->spk_latent_dim * cfg->spk_token_num + cfg->spk_out_dim + (size_t)(1 + cfg->pre_layers) * 2 * cfg->pre_dim + 64);
  int rc = SMI_OK;
  for (int i = 0; i < 4 && !rc; ++i) rc = h->buf[i].alloc(h->buf_floats * cfg->max_batch * 4, "vocoder activation buffer");
  if (!rc) rc = h->small.alloc(small_floats * 4, "vocoder small");
  if (!rc) rc = h->lens_dev.alloc(8 * cfg->max_batch * 4 + 64, "vocoder lens_dev");
  for (int i = 0; i < 8 && !rc && h->debug; ++i) {
    h->dbg_floats[i] = h->buf_floats * cfg->max_batch;
    rc = h->dbg[i].alloc(h->dbg_floats[i] * 4, "vocoder debug buffer");
  }
  if (!rc && (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)) {
    smi_set_error("smi_voc_create: hipEventCreate failed");
    rc = SMI_ENOMEM;
  }
  if (rc) {
    smi_voc_destroy(h);
    return SMI_ENOMEM;
  }
  *out = h;
  return SMI_OK;
}

int smi_voc_destroy(smi_voc* h) {
  if (!h) return SMI_OK;
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  delete h;
  return SMI_OK;
}

}  // extern "C"

namespace {

// The launch list of one forward over rows row0 .. row0 + B of a call (their lengths sit in h->lens_dev): T is the extent -- the
// longest of these rows, and the row stride of the working buffers; semstride / wavstride are the row strides of the CALLER's
// sem_dev / wav_dev, which sem_dev / glob_dev / wav_dev point into at row0.  ps null: the plan shape is (B, T) (smi_voc_forward);
// else the plan is ps's one row (smi_voc_forward_rows).
int voc_program(smi_voc* h, std::vector<Launch>& P, const int64_t* sem_dev, int semstride, const int32_t* glob_dev, int B, int T,
                float* wav_dev, long long wavstride, int row0, const PlanShape* ps) {
  const smi_voc_cfg& c = h->cfg;
  auto lens_at = [&](int s) { return (const int*)(h->lens_dev + (size_t)s * c.max_batch + row0); };
  const int* len1 = lens_at(7);
  const int* len0 = lens_at(0);

  const long long bs = (long long)h->buf_floats;
  float* bufs[4] = {h->buf[0], h->buf[1], h->buf[2], h->buf[3]};
  // a buffer that none of the listed live activations occupies
  auto other = [&](std::initializer_list<const float*> used) -> float* {
    for (float* f : bufs) {
      bool u = false;
      for (const float* q : used) u |= (q == f);
      if (!u) return f;
    }
    return nullptr;
  };
  const int D = c.pre_dim, I = c.pre_inter;
  const int nada = 1 + c.pre_layers;
  // small scratch: [lat: B x (latent*Ntok)] [dvec: B x out] [ada: B x nada*2*D]
  const int latn = c.spk_latent_dim * c.spk_token_num;
  float* lat = h->small;
  float* dvec = lat + (size_t)c.max_batch * latn;
  float* ada = dvec + (size_t)c.max_batch * c.spk_out_dim;
  const int ada_stride = nada * 2 * D;

  // --- d-vector: FSQ codes -> latent -> project (speaker_encoder.py:107-112)
  {
    Launch L; L.kind = 3; L.name = "fsq_latent"; L.flops = 2.0 * B * latn * c.fsq_dims; L.B = B;
    L.fp.glob = glob_dev; L.fp.W1 = ent(h, "speaker_encoder.quantizer.project_out.weight");
    L.fp.b1 = ent(h, "speaker_encoder.quantizer.project_out.bias"); L.fp.out = lat;
    L.fp.Ntok = c.spk_token_num; L.fp.latent = c.spk_latent_dim; L.fp.nd = c.fsq_dims;
    for (int j = 0; j < 8; ++j) L.fp.levels[j] = j < c.fsq_dims ? c.fsq_levels[j] : 1;
    P.push_back(L);
  }
  const WSrc ws = wsrc(h);
  // a per-utterance vector projection (k_gemv1): x [B][Cin] at batch stride xb -> y [B][Cout]
  auto gemv = [&](const std::string& name, const std::string& wname, const std::string& bname, int Cout, int Cin, const float* X, long long xb,
                  float* Y) {
    ConvSpec s = layer(ws, name, wname, bname, 1, 0, len1, B, ps);
    s.Cout = Cout; s.Cin = Cin; s.X = X; s.xb = xb; s.Y = Y; s.yb = Cout; s.want = CONV_GEMV;
    P.push_back(make_conv(s));
  };
  gemv("spk_project", "speaker_encoder.project.weight", "speaker_encoder.project.bias", c.spk_out_dim, latn, lat, latn, dvec);
  // all AdaLayerNorm scale/shift projections of the condition in one GEMM (vocos.py:105-108)
  {
    std::string wn, bn;
    for (const Entry& e : h->lay.e) {
      if (e.name.rfind("cat:", 0) == 0 && e.kind == PACK_CONV) wn = e.name;
      if (e.name.rfind("cat:", 0) == 0 && e.kind == PACK_RAW) bn = e.name;
    }
    gemv("adaln_params", wn, bn, ada_stride, c.pre_cond_dim, dvec, c.spk_out_dim, ada);
  }
  // a stride-1 layer on the call's [C][T] activations
  auto conv = [&](const std::string& name, const std::string& pfx, int Cout, int Cin, int K, const float* X, float* Y) {
    ConvSpec s = layer(ws, name, pfx + ".weight", pfx + ".bias", T, bs, len0, B, ps);
    s.Cout = Cout; s.Cin = Cin; s.K = K; s.pad = K / 2; s.X = X; s.Y = Y;
    return s;
  };
  // --- semantic tokens -> codebook rows -> out_project (factorized_vector_quantize.py:154-167)
  float* zc = bufs[0];
  {
    Launch L; L.kind = 2; L.name = "codebook"; L.flops = 0;
    L.sem = sem_dev; L.semstride = semstride; L.cb = ent(h, "quantizer.codebook.weight"); L.D = c.codebook_dim; L.cbsize = c.codebook_size;
    L.lens = len0; L.Z = zc; L.zstride = T; L.zb = bs; L.grid = dim3((T + 127) / 128, B);
    P.push_back(L);
  }
  float* zq = other({zc});
  // a debug build runs the layer a second time into its stage buffer
  auto push = [&](ConvSpec s, float* dbg) {
    P.push_back(make_conv(s));
    if (h->debug) { s.Y = dbg; s.name += "(dbg)"; P.push_back(make_conv(s)); }
  };
  push(conv("vq_out_project", "quantizer.out_project", c.vq_input_dim, c.codebook_dim, 1, zc, zq), h->dbg[0]);
  // --- prenet (feat_decoder.py:78-94)
  float* cur = other({zq});
  ConvSpec pre = conv("prenet.linear_pre", "prenet.linear_pre", D, c.pre_input_channels, 1, zq, cur);
  pre.out_scale = c.pre_num_down > 0 ? 3.0f : 1.0f;   // first SamplingBlock(ratio 1): 3x
  P.push_back(make_conv(pre));
  int ada_idx = 0;
  auto lnorm = [&](const std::string& name, const std::string& pfx, bool ada_norm, const float* X, float* Y, int triple) {
    const float* ap = ada_norm ? ada + (size_t)(ada_idx++) * 2 * D : nullptr;
    add_lnorm(P, ws, name, pfx, ap, ada_stride, nullptr, nullptr, X, Y, triple, D, T, bs, len0, B);
  };
  // embed conv7 -> norm -> nl x ConvNeXt -> final LN (vocos.py:324-335); consumes cur, leaves result in cur
  auto vocos = [&](const std::string& p, int nl, bool ada_norm, int triple_out) {
    float* n = other({cur});          // conv / norm output
    P.push_back(make_conv(conv(p + ".embed", p + ".embed", D, D, 7, cur, n)));
    float* x = other({n});            // residual stream (cur is dead once embed has run)
    lnorm(p + ".norm", p + ".norm", ada_norm, n, x, 0);
    float* m = other({x, n});         // MLP hidden
    for (int j = 0; j < nl; ++j) {
      const float* ap = ada_norm ? ada + (size_t)(ada_idx++) * 2 * D : nullptr;
      add_convnext(P, ws, p + ".convnext." + std::to_string(j), D, I, x, n, m, ap, ada_stride, T, bs, len0, B, ps);
    }
    lnorm(p + ".final_layer_norm", p + ".final_layer_norm", false, x, n, triple_out);
    cur = n;
  };
  for (int i = 0; i < c.pre_num_down; ++i)
    vocos("prenet.downsample." + std::to_string(i) + ".1", 2, false, (i + 1 < c.pre_num_down) ? 1 : 0);
  vocos("prenet.vocos_backbone", c.pre_layers, c.pre_cond_dim > 0, 0);
  SMI_REQUIRE(!c.pre_tanh_final, "smi_voc: use_tanh_at_final is not supported");
  // prenet.linear, then + d_vector per utterance (bicodec.py:185-186)
  float* x0 = other({cur});
  ConvSpec lin = conv("prenet.linear+d", "prenet.linear", c.pre_out_channels, D, 1, cur, x0);
  lin.bbias = dvec;
  push(lin, h->dbg[1]);
  // --- WaveGenerator (wave_generator.py:56-88)
  int ch = c.dec_channels;
  int Lcur = T;
  float* s_in = other({x0});   // snake'd input of the next ConvTranspose
  {
    ConvSpec in = conv("decoder.conv_in", "decoder.model.0", ch, c.dec_in, 7, x0, h->debug ? (float*)h->dbg[2] : nullptr);
    in.Ys = s_in; in.alpha = ent(h, "decoder.model.1.block.0.alpha");
    P.push_back(make_conv(in));
  }
  for (int i = 0; i < c.dec_nblocks; ++i) {
    const int cin = ch >> i, cout = ch >> (i + 1), k = c.dec_ksizes[i], s = c.dec_rates[i];
    const std::string b = "decoder.model." + std::to_string(i + 1) + ".block";
    const int Lout = Lcur * s;
    float* U = other({s_in});
    float* US = other({s_in, U});
    float* A = other({s_in, U, US});
    // Snake (already applied by the producer) -> ConvTranspose1d -> three ResidualUnits; the last unit's second output is the
    // NEXT consumer's Snake of the block's result (the next block's, or the output conv's)
    const std::string next_alpha = i + 1 < c.dec_nblocks ? "decoder.model." + std::to_string(i + 2) + ".block.0.alpha"
                                                         : "decoder.model." + std::to_string(c.dec_nblocks + 1) + ".alpha";
    s_in = add_dec_block(P, ws, b, cin, cout, k, s, s_in, Lcur, bs, U, US, A, h->debug ? h->dbg[3 + i] : nullptr, ent(h, next_alpha), bs,
                         lens_at(i), lens_at(i + 1), B, ps);
    Lcur = Lout;
  }
  const int clast = ch >> c.dec_nblocks;
  const int hop = Lcur / T;
  {
    const std::string n = "decoder.model." + std::to_string(c.dec_nblocks + 2);
    // final conv7 -> tanh, written straight into the caller's waveform buffer [B][wavstride]; C -> 1: the one-channel kernel
    ConvSpec o = layer(ws, "decoder.conv_out+tanh", n + ".weight", n + ".bias", Lcur, bs, lens_at(c.dec_nblocks), B, ps);
    o.Cout = 1; o.Cin = clast; o.K = 7; o.pad = 3; o.X = s_in; o.Y = wav_dev; o.yb = wavstride; o.act = ACT_TANH; o.want = CONV_C1;
    P.push_back(make_conv(o));
    Launch Z; Z.kind = 4; Z.name = "zero_tail"; Z.flops = 0; Z.wav = wav_dev; Z.wstride = (int)wavstride; Z.lens = len0; Z.hop = hop;
    Z.grid = dim3((unsigned)((wavstride + 255) / 256), B);
    P.push_back(Z);
  }
  return SMI_OK;
}

// The call's shape checks and h->host_lens, the valid lengths at every resolution: [s][b] = lens[b] * prod(rates[0..s)), and
// [7][b] = 1, the length-1 "sequences" of the d-vector GEMVs.
int voc_host_lens(smi_voc* h, const char* who, const int32_t* lens_host, int B, int T) {
  const smi_voc_cfg& c = h->cfg;
  SMI_REQUIRE(B >= 1 && B <= c.max_batch, "%s: B=%d outside 1..%d", who, B, c.max_batch);
  SMI_REQUIRE(T >= 1 && T <= c.max_frames, "%s: T_max=%d outside 1..%d", who, T, c.max_frames);
  std::vector<int32_t>& hl = h->host_lens;
  hl.assign((size_t)8 * c.max_batch, 0);
  for (int b = 0; b < B; ++b) {
    SMI_REQUIRE(lens_host[b] >= 1 && lens_host[b] <= T, "%s: lens[%d]=%d outside 1..%d", who, b, lens_host[b], T);
    int up = 1;
    for (int s = 0; s <= c.dec_nblocks; ++s) {
      hl[(size_t)s * c.max_batch + b] = lens_host[b] * up;
      if (s < c.dec_nblocks) up *= c.dec_rates[s];
    }
    hl[(size_t)7 * c.max_batch + b] = 1;
  }
  return SMI_OK;
}

}  // namespace

extern "C" {

int smi_voc_forward(smi_voc* h, const int64_t* sem_dev, const int32_t* lens_host, const int32_t* glob_dev, int B, int T,
                    float* wav_dev, void* stream) {
  SMI_REQUIRE(h && sem_dev && lens_host && glob_dev && wav_dev, "smi_voc_forward: null argument");
  const smi_voc_cfg& c = h->cfg;
  hipStream_t st = (hipStream_t)stream;
  int rc = voc_host_lens(h, "smi_voc_forward", lens_host, B, T);
  if (rc) return rc;
  const std::vector<int32_t>& hl = h->host_lens;
  SMI_HIP(hipMemcpyAsync(h->lens_dev, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, st));
  std::vector<Launch>& P = h->prog;
  P.clear();
  long long hop = 1;
  for (int i = 0; i < c.dec_nblocks; ++i) hop *= c.dec_rates[i];
  rc = voc_program(h, P, sem_dev, T, glob_dev, B, T, wav_dev, hop * T, 0, nullptr);
  if (rc) return rc;
  if ((rc = check_launches(P, "smi_voc_forward"))) return rc;
  for (const Launch& L : P)
    if ((rc = run_launch(L, st))) return rc;
  h->lastB = B; h->lastT = T;
  return SMI_OK;
}

// A ragged batch whose rows carry their solo bits (include/sparkmi.h).  A row's plan is the launch list smi_voc_forward builds for
// that row alone, (1, lens[b]); consecutive rows with equal plans (plan_signature) run as one launch sequence with that plan and
// the extent (rows of the run, its longest row).  The launch list is rebuilt per call, as smi_voc_forward's is.
int smi_voc_forward_rows(smi_voc* h, const int64_t* sem_dev, const int32_t* lens_host, const int32_t* glob_dev, int B, int T,
                         float* wav_dev, void* stream) {
  SMI_REQUIRE(h && sem_dev && lens_host && glob_dev && wav_dev, "smi_voc_forward_rows: null argument");
  const smi_voc_cfg& c = h->cfg;
  hipStream_t st = (hipStream_t)stream;
  int rc = voc_host_lens(h, "smi_voc_forward_rows", lens_host, B, T);
  if (rc) return rc;
  const std::vector<int32_t>& hl = h->host_lens;
  long long hop = 1;
  for (int i = 0; i < c.dec_nblocks; ++i) hop *= c.dec_rates[i];
  // the plan of every distinct length: the choices of that row's own smi_voc_forward (pointers do not enter a signature)
  std::map<int, std::vector<long long>> plans;
  std::vector<const std::vector<long long>*> sig((size_t)B);
  for (int b = 0; b < B; ++b) {
    auto it = plans.find(lens_host[b]);
    if (it == plans.end()) {
      std::vector<Launch> solo;
      if ((rc = voc_program(h, solo, sem_dev, lens_host[b], glob_dev, 1, lens_host[b], wav_dev, hop * lens_host[b], 0, nullptr))) return rc;
      it = plans.emplace(lens_host[b], plan_signature(solo)).first;
    }
    sig[b] = &it->second;
  }
  const std::vector<int> runs = plan_runs(sig);
  std::vector<Launch>& P = h->prog;
  P.clear();
  std::vector<Launch> G;
  for (size_t i = 0; i + 1 < runs.size(); ++i) {
    const int r0 = runs[i], r1 = runs[i + 1];
    const int Tg = *std::max_element(lens_host + r0, lens_host + r1);
    const PlanShape ps{lens_host[r0], Tg};
    G.clear();
    if ((rc = voc_program(h, G, sem_dev + (size_t)r0 * T, T, glob_dev + (size_t)r0 * c.spk_token_num, r1 - r0, Tg,
                          wav_dev + (size_t)r0 * hop * T, hop * T, r0, &ps))) return rc;
    if (plan_signature(G) != *sig[r0]) {
      smi_set_error("smi_voc_forward_rows: the launch list of rows %d..%d does not carry the plan of a %d-frame row", r0, r1 - 1, lens_host[r0]);
      return SMI_EINVAL;
    }
    P.insert(P.end(), G.begin(), G.end());
  }
  if ((rc = check_launches(P, "smi_voc_forward_rows"))) return rc;
  SMI_HIP(hipMemcpyAsync(h->lens_dev, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, st));
  for (const Launch& L : P)
    if ((rc = run_launch(L, st))) return rc;
  h->lastB = B; h->lastT = T;
  return SMI_OK;
}

int smi_voc_debug_stage(smi_voc* h, int stage, float* out_dev, size_t max_floats, size_t* n_floats, void* stream) {
  SMI_REQUIRE(h && out_dev && n_floats, "smi_voc_debug_stage: null argument");
  SMI_REQUIRE(h->lastB > 0, "smi_voc_debug_stage: no forward has run");
  const smi_voc_cfg& c = h->cfg;
  const float* src = nullptr;
  size_t n = 0;
  if (stage == -1) {   // d-vector [B][out_dim]
    src = h->small + (size_t)c.max_batch * c.spk_latent_dim * c.spk_token_num;
    n = (size_t)h->lastB * c.spk_out_dim;
  } else {
    SMI_REQUIRE(h->debug, "smi_voc_debug_stage: create the handle with SPARKMI_VOC_DEBUG=1");
    SMI_REQUIRE(stage >= 0 && stage < 3 + c.dec_nblocks, "smi_voc_debug_stage: stage %d out of range", stage);
    src = h->dbg[stage];
    n = h->buf_floats * h->lastB;   // rows are [C][stride] inside each batch slot
  }
  SMI_REQUIRE(n <= max_floats, "smi_voc_debug_stage: output buffer too small (%zu > %zu)", n, max_floats);
  SMI_HIP(hipMemcpyAsync(out_dev, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  *n_floats = n;
  return SMI_OK;
}

int smi_voc_num_launches(smi_voc* h) { return h ? (int)h->prog.size() : 0; }

int smi_voc_time_launch(smi_voc* h, int index, int iters, float* ms_avg, double* flops, char* name, int name_cap, void* stream) {
  SMI_REQUIRE(h && ms_avg && iters > 0, "smi_voc_time_launch: bad argument");
  SMI_REQUIRE(index >= 0 && index < (int)h->prog.size(), "smi_voc_time_launch: index %d out of range", index);
  return time_launch(h->prog[index], h->ev0, h->ev1, iters, ms_avg, flops, name, name_cap, (hipStream_t)stream);
}

// ---- one block of the vocoder on caller tensors (op-level tests; include/sparkmi.h)
int smi_voc_block_arena_count(const smi_voc_block_cfg* cfg) { return block_cfg_ok(cfg) ? (int)block_layout(cfg).e.size() : 0; }
size_t smi_voc_block_arena_bytes(const smi_voc_block_cfg* cfg) { return block_cfg_ok(cfg) ? block_layout(cfg).total : 0; }
int smi_voc_block_arena_entry(const smi_voc_block_cfg* cfg, int index, char* name, int name_cap, size_t* offset, size_t* bytes, int32_t* info) {
  SMI_REQUIRE(block_cfg_ok(cfg), "smi_voc_block_arena_entry: config outside the kernel contract");
  return layout_entry(block_layout(cfg), index, name, name_cap, offset, bytes, info, "smi_voc_block_arena_entry");
}

int smi_voc_block_run(const smi_voc_block_cfg* cfg, const void* arena_dev, size_t arena_bytes, const float* x_dev, const float* xs_dev,
                      const float* cond_dev, const int32_t* lens_host, int B, int L, float* y_dev, void* stream) {
  SMI_REQUIRE(block_cfg_ok(cfg), "smi_voc_block_run: config outside the kernel contract");
  const smi_voc_block_cfg& c = *cfg;
  VocLayout lay = block_layout(cfg);
  SMI_REQUIRE(arena_dev && arena_bytes >= lay.total, "smi_voc_block_run: arena too small (%zu < %zu)", arena_bytes, lay.total);
  SMI_REQUIRE(((uintptr_t)arena_dev & 255) == 0, "smi_voc_block_run: arena must be 256-byte aligned");
  SMI_REQUIRE(y_dev && B >= 1 && B <= 64 && L >= 1 && L <= (1 << 20), "smi_voc_block_run: bad B / L / output");
  SMI_REQUIRE(c.kind == SMI_VOC_BLOCK_DECBLOCK ? xs_dev != nullptr : x_dev != nullptr, "smi_voc_block_run: input tensor is null");
  SMI_REQUIRE(c.kind != SMI_VOC_BLOCK_RESUNIT || xs_dev, "smi_voc_block_run: a ResidualUnit needs x and snake(x)");
  SMI_REQUIRE(c.kind != SMI_VOC_BLOCK_CONVNEXT || c.cond_dim == 0 || cond_dev, "smi_voc_block_run: AdaLayerNorm needs the condition vector");
  hipStream_t st = (hipStream_t)stream;
  const WSrc w{&lay.e, (const unsigned char*)arena_dev};
  const int Lout = c.kind == SMI_VOC_BLOCK_DECBLOCK ? L * c.S : L;
  const int Cin = c.C, Cres = c.kind == SMI_VOC_BLOCK_DECBLOCK ? c.Cout : c.C;
  const int Cmax = std::max(std::max(Cin, Cres), c.kind == SMI_VOC_BLOCK_CONVNEXT ? c.I : 1);
  const long long bs = (long long)smi_align_up((size_t)Cmax * Lout, 64);   // one batch stride for every working buffer, as in the vocoder
  // working buffers: [0] input / x, [1] snake(input) / n, [2] U or m, [3] US, [4] A ; ints: lens_in, lens_out, ones ; ada
  DevBuf<float> own[5], ada;
  DevBuf<int> lens;
  int rc = SMI_OK;
  for (int i = 0; i < 5 && !rc; ++i) rc = own[i].alloc((size_t)bs * B * 4, "smi_voc_block_run: working buffer");
  if (rc || (rc = ada.alloc((size_t)B * 2 * c.C * 4 + 256, "smi_voc_block_run: ada")) || (rc = lens.alloc((size_t)3 * 64 * 4, "smi_voc_block_run: lens"))) return rc;
  float* const buf[5] = {own[0], own[1], own[2], own[3], own[4]};
  std::vector<int32_t> hl((size_t)3 * 64, 0);
  for (int b = 0; b < B; ++b) {
    const int n = lens_host ? lens_host[b] : L;
    SMI_REQUIRE(n >= 1 && n <= L, "smi_voc_block_run: lens[%d]=%d outside 1..%d", b, n, L);
    hl[b] = n; hl[64 + b] = n * (Lout / L); hl[128 + b] = 1;
  }
  // from here every way out passes the synchronise at the end: the stream is done with the buffers before they go
  auto fail = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == SMI_OK) { smi_set_error("smi_voc_block_run: %s: %s", what, hipGetErrorString(e)); rc = SMI_EHIP; } };
  fail(hipMemcpyAsync(lens, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, st), "lens upload");
  for (int i = 0; i < 5; ++i) fail(hipMemsetAsync(buf[i], 0, (size_t)bs * B * 4, st), "memset");
  auto copy_in = [&](float* dst, const float* src, int C, int len) {   // contiguous [B][C][len] -> working layout
    fail(hipMemcpy2DAsync(dst, (size_t)bs * 4, src, (size_t)C * len * 4, (size_t)C * len * 4, (size_t)B, hipMemcpyDeviceToDevice, st), "copy in");
  };
  std::vector<Launch> P;
  if (c.kind == SMI_VOC_BLOCK_RESUNIT) {
    copy_in(buf[0], x_dev, c.C, L);
    copy_in(buf[1], xs_dev, c.C, L);
  } else if (c.kind == SMI_VOC_BLOCK_DECBLOCK) {
    copy_in(buf[1], xs_dev, c.C, L);
  } else {
    copy_in(buf[0], x_dev, c.C, L);
  }
  float* result = block_program(P, c, w, buf, ada, cond_dev, lens, bs, B, L);
  if (rc == SMI_OK) rc = check_launches(P, "smi_voc_block_run");
  for (size_t i = 0; i < P.size() && rc == SMI_OK; ++i) rc = run_launch(P[i], st);
  if (rc == SMI_OK)
    fail(hipMemcpy2DAsync(y_dev, (size_t)Cres * Lout * 4, result, (size_t)bs * 4, (size_t)Cres * Lout * 4, (size_t)B, hipMemcpyDeviceToDevice, st), "copy out");
  fail(hipStreamSynchronize(st), "synchronize");
  return rc;
}

}  // extern "C"

#ifdef SMI_DIAG   // ---- include/sparkmi_debug.h: the conv kernel forms, exported by libsparkmi_diag.so only
namespace {

smi_conv_form form_record(const ConvForm& f) { return smi_conv_form{f.kernel, f.qb, f.ks, f.chg, f.nc, f.nwv, f.wpf, f.wall, f.tph}; }

int conv_case_lout(const smi_conv_case& c, int n) {   // output positions of a row of n input positions
  if (c.S > 1) return n * c.S;
  if (c.istr > 1) return n < (c.K - 1) * c.dil + 1 ? 0 : (n - (c.K - 1) * c.dil - 1) / c.istr + 1;
  return n;
}

// one conv launch for a case, through make_conv() and check_conv() as the launch lists' are
int conv_case_launch(const smi_conv_case* cp, const smi_conv_operands& io, const int* lens, const int* olens, Launch& L, const char* who) {
  SMI_REQUIRE(cp, "%s: case is null", who);
  const smi_conv_case& c = *cp;
  SMI_REQUIRE(c.Cout >= 1 && c.Cout <= 8192 && c.Cin >= 1 && c.Cin <= 8192 && c.B >= 1 && c.B <= 4096 && c.L >= 1 && c.L <= (1 << 20),
              "%s: Cout / Cin / B / L out of range", who);
  SMI_REQUIRE(c.dil >= 1 && c.K >= 1 && c.S >= 1 && c.S <= kMaxPhases && c.istr >= 1, "%s: bad K / dil / S / istr", who);
  SMI_REQUIRE(c.act == ACT_NONE || c.act == ACT_GELU || c.act == ACT_TANH || c.act == ACT_RELU || (c.gemv && c.act == ACT_SIGMOID), "%s: bad act", who);
  if (c.S > 1) {
    SMI_REQUIRE(c.istr == 1 && c.dil == 1 && c.K >= c.S && (c.K - c.S) % 2 == 0 && c.pad == (c.K - c.S) / 2 && (c.K + c.S - 1) / c.S <= kMaxTaps,
                "%s: a transposed conv needs istr = dil = 1, K >= S, (K - S) even, pad = (K - S) / 2, at most %d taps per phase", who, kMaxTaps);
  } else {
    SMI_REQUIRE(c.K <= kMaxTaps, "%s: at most %d taps", who, kMaxTaps);
    if (c.istr == 1) SMI_REQUIRE(2 * c.pad == c.dil * (c.K - 1), "%s: a stride-1 conv keeps its length: 2 * pad = dil * (K - 1)", who);
    else SMI_REQUIRE(c.pad == 0 && !c.bf, "%s: a strided conv has pad = 0 and runs on the exact pipe (k_convb stages with unit stride)", who);
  }
  SMI_REQUIRE(!(c.gemv && c.c1), "%s: gemv and c1 exclude each other", who);
  SMI_REQUIRE(c.plan_frames == 0 || (c.plan_frames >= 1 && c.plan_ext_frames == c.L && c.plan_frames <= c.L && !c.gemv && !c.c1 && c.istr == 1),
              "%s: a plan shape is one row of 1..L frames with plan_ext_frames = L (unit input stride)", who);
  const int lout = conv_case_lout(c, c.L);
  SMI_REQUIRE(lout >= 1, "%s: L = %d gives no output", who, c.L);
  const PlanShape ps{c.plan_frames, c.plan_ext_frames};
  SMI_REQUIRE(io.out_scale == 1.0f || io.out_scale == 3.0f, "%s: out_scale is 1 or 3", who);
  SMI_REQUIRE(!(c.bf && io.X2), "%s: the bf16-split kernels stage X only (no second input)", who);
  ConvSpec s;
  s.name = "conv"; s.Cout = c.Cout; s.Cin = c.Cin; s.K = c.K; s.dil = c.dil; s.S = c.S; s.pad = c.pad; s.istr = c.istr; s.bf = c.bf != 0;
  s.W = io.W; s.bias = io.bias; s.X = io.X; s.X2 = io.X2; s.xstride = c.L; s.xb = (long long)c.Cin * c.L;
  s.Y = io.Y; s.Ys = io.Ys; s.alpha = io.alpha; s.R = io.R ? io.R : (c.has_R ? io.X : nullptr); s.ystride = lout; s.yb = (long long)c.Cout * lout;
  s.lens = lens; s.olens = c.istr > 1 ? olens : nullptr; s.B = c.B; s.Lmax = c.S > 1 ? c.L : lout; s.act = c.act;   // Lmax: output positions per phase
  s.bbias = io.bbias; s.gamma = io.gamma; s.beta = io.beta; s.out_scale = io.out_scale;
  s.want = c.gemv ? CONV_GEMV : (c.c1 ? CONV_C1 : CONV_MFMA); s.ps = c.plan_frames ? &ps : nullptr;
  if (c.gemv)
    SMI_REQUIRE(!c.bf && c.K == 1 && c.S == 1 && c.istr == 1 && c.L == 1 && !io.X2 && !io.bbias && !io.gamma && !io.beta && !s.R && !io.Ys &&
                io.out_scale == 1.0f && (c.act == ACT_NONE || c.act == ACT_RELU || c.act == ACT_SIGMOID),
                "%s: the vector projection is an exact 1-tap layer on L = 1 with bias and ReLU / sigmoid only", who);
  L = make_conv(s);
  SMI_REQUIRE(!c.c1 || (L.plan.form >= 0 && conv_form_at(L.plan.form).kernel == CONV_K_C1),
              "%s: k_conv_c1 is an exact 7-tap conv to one channel with bias and activation only", who);
  return check_conv(L, who);
}

void conv_plan_info(const smi_conv_case& c, const Launch& L, smi_conv_plan_info* out) {
  memset(out, 0, sizeof(*out));
  out->form = form_record(conv_form_at(L.plan.form)); out->form_index = L.plan.form; out->xw = L.plan.xw;
  out->grid[0] = (int)L.grid.x; out->grid[1] = (int)L.grid.y; out->grid[2] = (int)L.grid.z;
  out->lout = c.gemv ? 1 : conv_case_lout(c, c.L);
  out->lds_bytes = (long long)L.lds;
  out->plan_blocks = L.plan_blocks;
}

}  // namespace

extern "C" {

int smi_conv_form_count(void) { return conv_form_count(); }

int smi_conv_form_get(int index, smi_conv_form* out) {
  SMI_REQUIRE(out && index >= 0 && index < conv_form_count(), "smi_conv_form_get: index %d out of range", index);
  *out = form_record(conv_form_at(index));
  return SMI_OK;
}

int smi_conv_plan(const smi_conv_case* c, smi_conv_plan_info* out) {
  SMI_REQUIRE(out, "smi_conv_plan: out is null");
  smi_conv_operands io;
  memset(&io, 0, sizeof(io));
  io.out_scale = 1.0f;
  io.W = io.X = (const float*)(uintptr_t)256;   // placeholders: never dereferenced on the host
  io.Y = (float*)(uintptr_t)512;
  Launch L;
  int rc = conv_case_launch(c, io, nullptr, (const int*)(uintptr_t)768, L, "smi_conv_plan");
  if (rc) return rc;
  conv_plan_info(*c, L, out);
  return SMI_OK;
}

int smi_conv_run(const smi_conv_case* c, const smi_conv_operands* io, const int32_t* lens_host, smi_conv_plan_info* plan, void* stream) {
  SMI_REQUIRE(c && io && io->W && io->X && (io->Y || io->Ys), "smi_conv_run: null argument");
  SMI_REQUIRE(!io->Ys || io->alpha, "smi_conv_run: Ys needs alpha");
  SMI_REQUIRE(!c->has_R == !io->R, "smi_conv_run: has_R and the R operand disagree");
  SMI_REQUIRE(c->B >= 1 && c->B <= 4096, "smi_conv_run: B out of range");
  hipStream_t st = (hipStream_t)stream;
  const int B = c->B;
  std::vector<int32_t> hl((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    const int n = c->gemv ? 1 : (lens_host ? lens_host[b] : c->L);
    SMI_REQUIRE(n >= 1 && n <= c->L, "smi_conv_run: lens[%d]=%d outside 1..%d", b, n, c->L);
    hl[b] = n; hl[(size_t)B + b] = c->gemv ? 1 : conv_case_lout(*c, n);
  }
  DevBuf<int> lens;
  int rc = lens.alloc(hl.size() * 4, "smi_conv_run: lens");
  if (rc) return rc;
  Launch L;
  rc = conv_case_launch(c, *io, lens, lens + B, L, "smi_conv_run");
  smi_conv_plan_info info;
  if (rc == SMI_OK) conv_plan_info(*c, L, &info);
  auto fail = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == SMI_OK) { smi_set_error("smi_conv_run: %s: %s", what, hipGetErrorString(e)); rc = SMI_EHIP; } };
  if (rc == SMI_OK) fail(hipMemcpyAsync(lens, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, st), "lens upload");
  if (rc == SMI_OK) rc = run_launch(L, st);
  fail(hipStreamSynchronize(st), "synchronize");   // (before lens goes)
  if (rc == SMI_OK && plan) *plan = info;
  return rc;
}

int smi_voc_block_plan(const smi_voc_block_cfg* cfg, int B, int L, smi_block_launch_info* out, int cap, int32_t* n) {
  SMI_REQUIRE(block_cfg_ok(cfg), "smi_voc_block_plan: config outside the kernel contract");
  SMI_REQUIRE(n && B >= 1 && B <= 64 && L >= 1 && L <= (1 << 20) && cap >= 0 && (out || cap == 0), "smi_voc_block_plan: bad B / L / output");
  const smi_voc_block_cfg& c = *cfg;
  VocLayout lay = block_layout(cfg);
  // placeholder addresses (distinct, non-null, never dereferenced): the builders only compare and store them
  const WSrc w{&lay.e, (const unsigned char*)(uintptr_t)(1 << 20)};
  float* buf[5];
  for (int i = 0; i < 5; ++i) buf[i] = (float*)(((uintptr_t)1 << 40) + ((uintptr_t)i << 34));
  float* ada = (float*)((uintptr_t)1 << 39);
  const int* lens = (const int*)((uintptr_t)1 << 38);
  const int Lout = c.kind == SMI_VOC_BLOCK_DECBLOCK ? L * c.S : L;
  const int Cres = c.kind == SMI_VOC_BLOCK_DECBLOCK ? c.Cout : c.C;
  const int Cmax = std::max(std::max(c.C, Cres), c.kind == SMI_VOC_BLOCK_CONVNEXT ? c.I : 1);
  const long long bs = (long long)smi_align_up((size_t)Cmax * Lout, 64);
  std::vector<Launch> P;
  block_program(P, c, w, buf, ada, (const float*)((uintptr_t)1 << 37), lens, bs, B, L);
  int rc = check_launches(P, "smi_voc_block_plan");
  if (rc) return rc;
  *n = (int32_t)P.size();
  for (size_t i = 0; i < P.size() && (int)i < cap; ++i) {
    smi_block_launch_info& o = out[i];
    memset(&o, 0, sizeof(o));
    strncpy(o.name, P[i].name.c_str(), sizeof(o.name) - 1);
    o.kind = P[i].kind; o.form_index = -1;
    if (P[i].kind == 0) {
      o.form_index = P[i].plan.form; o.form = form_record(conv_form_at(o.form_index));
    } else if (P[i].kind == 1) {
      o.cpt = dwln_form(P[i].cpt);
    } else if (P[i].kind == 5) {
      o.res_nwv = P[i].res_nwv;
    }
  }
  return SMI_OK;
}

}  // extern "C"
#endif   // SMI_DIAG
