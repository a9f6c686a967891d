// The denoiser's plan: weight repacking, activation workspace and the launch sequence of one reservation.
//
// Reference structure reproduced layer for layer:
//   local_map_encoder.py:101-122   encoder(local_map) -> 400-d, cat with obs_cond
//   conditional_unet1d.py:268-347  time MLP, down [CRB,CRB,Down] x3 (last Identity),
//                                  mid 2 x CRB, up [cat skip, CRB, CRB, Up] x2, final conv
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

#include "denoise_state.h"

namespace {

inline uint16_t f2bf_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);     // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f_host(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline uint16_t f2h_host(float f) { _Float16 h = (_Float16)f; uint16_t u; std::memcpy(&u, &h, 2); return u; }   // RNE
inline float h2f_host(uint16_t u) { _Float16 h; std::memcpy(&h, &u, 2); return (float)h; }

// Live (kh, kw) taps of a k x k Conv2d from an H x H to an OH x OH map.  Taps that fall into the zero padding for every output
// position are dropped from the GEMM and from the packed weights (exact: a 3 x 3 conv on a 1 x 1 map keeps the centre tap only).
TapList live_taps(int k, int stride, int pad, int H, int OH) {
  TapList tl{};
  for (int kh = 0; kh < k; ++kh)
    for (int kw = 0; kw < k; ++kw) {
      bool lh = false, lw = false;
      for (int o = 0; o < OH; ++o) {
        const int ih = o * stride + kh - pad, iw = o * stride + kw - pad;
        lh |= (ih >= 0 && ih < H);
        lw |= (iw >= 0 && iw < H);
      }
      if (!(lh && lw)) continue;
      if (tl.n < 12) { tl.kh[tl.n] = (signed char)kh; tl.kw[tl.n] = (signed char)kw; }
      ++tl.n;
    }
  return tl;
}

Act view(const Act& base, int coff, int C) {
  Act v = base;
  v.coff = coff;
  v.C = C;
  return v;
}
// a plain row-major matrix as a GEMM operand: no per-sample rows (the op sets the row counts per call)
Act matrix(void* p, int ld, long long plane = 0) {
  Act a;
  a.p = p; a.C = ld; a.ld = ld; a.padded = false; a.plane = plane;
  return a;
}

}  // namespace

int* DenoiserState::sat_slot(const std::string& layer, int fmt) {
  if (fmt_st(fmt) != ST_F16 || sat_flags == nullptr) return nullptr;
  for (size_t i = 0; i < sat_names.size(); ++i)
    if (sat_names[i] == layer) return sat_flags + i;
  if ((int)sat_names.size() >= SAT_SLOTS) return sat_flags + SAT_SLOTS - 1;
  sat_names.push_back(layer);
  return sat_flags + sat_names.size() - 1;
}

int DenoiserState::pick_splitk(const ConvGemmParams& p, int fmt) {
  const char* e = getenv("DITREE_DENOISE_SPLITK");
  if (!e || atoi(e) == 0 || !fmt_split(fmt) || p.L == 4 || conv_gemm_kind(p, fmt) != 0) return 1;   // (L = 4: no split-K form)
  const int tiles = (p.M >> 8) * (p.N >> 8), nvc = p.Cin >> 5;
  int sk = 1;
  // more work-groups only while the chip is mostly idle: every split adds a 256 KB partial tile to write and read back.
  // Measured (profiles/r04_splitk_latency_probe.json): a denoiser call of 1 / 16 / 64 / 128 samples 6.8 -> 4.9 / 4.9 / 5.0 / 6.2 ms
  // with at most 64 work-groups per layer; 128 or 256 are slower again
  static const int cap = [] { const char* c = getenv("DITREE_DENOISE_SPLITK_WGS"); return c ? atoi(c) : 64; }();
  while (sk < 16 && tiles * (sk * 2) <= cap && tiles * (sk * 2) <= SK_MAX_SLABS && nvc % (sk * 2) == 0 && nvc / (sk * 2) >= 2) sk *= 2;
  return sk;
}

void DenoiserState::run_gemm(const ConvGemmParams& p_in, int fmt, hipStream_t s) {
  ConvGemmParams p = p_in;
  p.xcd_strips = 1;                  // the halo / gemm16 kernels walk an XCD's tiles in strips of four tile columns (xcd_remap_strips)
  if (const int sk = pick_splitk(p, fmt); sk > 1) {
    if (sk_ws == nullptr) {
      sk_ws = (float*)dalloc((size_t)SK_MAX_SLABS * 65536 * sizeof(float), false);
      sk_cnt = (int*)dalloc(SK_MAX_SLABS * sizeof(int));
    }
    p.splitk = sk; p.sk_ws = sk_ws; p.sk_cnt = sk_cnt;
  }
  // shape contract of the tiles (split formats exist on the halo / gemm16 / small-Conv2d tiles only): an error, not an abort
  if (!conv_gemm_supported(p, fmt))
    throw std::runtime_error("denoiser layer of shape M " + std::to_string(p.M) + " x N " + std::to_string(p.N) + " x K " +
                             std::to_string(p.taps) + "*" + std::to_string(p.Cin) + " (L " + std::to_string(p.L) +
                             ") fits no tile of this precision");
  prof.launch(p, fmt, s);
}

void* DenoiserState::dalloc(size_t bytes, bool zero) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) throw std::runtime_error("hipMalloc failed");
  if (zero && hipMemset(p, 0, bytes ? bytes : 16) != hipSuccess) throw std::runtime_error("hipMemset failed");
  allocs.push_back(p);
  return p;
}
void DenoiserState::free_workspace() {
  for (void* p : allocs) hipFree(p);
  allocs.clear();
  sk_ws = nullptr;                   // (allocated through dalloc: freed with the rest)
  sk_cnt = nullptr;
  named.clear();
  dev_w.clear();
  dev_f.clear();
  enc_ops.clear();
  unet_ops.clear();
  film_op = nullptr;
  sat_flags = sat_cond = sat_sample = nullptr;
  sat_names.clear();
  prec = -1;
  Bmax = 0;
  Buser = 0;
  temb_t = -1.0f;
}

float* DenoiserState::upload_f32(const std::string& key, const float* src, int64_t n) {
  auto it = dev_f.find(key);
  if (it != dev_f.end()) return it->second;
  float* d = (float*)dalloc((size_t)n * 4, false);
  if (hipMemcpy(d, src, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("memcpy");
  dev_f[key] = d;
  return d;
}
float* DenoiserState::vec(const std::string& name) {
  const HostParam& hp = P_(name);
  return upload_f32(name, hp.data, hp.n);
}

// Pack a GEMM weight [Npad][T*Cin_pad] in format `fmt` from get(n, t, ci): f32, or 16-bit elements -- for a split
// format hi = rnd16(w) and lo = rnd16(w - hi), chunk-interleaved: the 32 channels of a K-step are one 128-byte unit
// [32 hi | 32 lo], so that the tile kernels stage an LDS row from ONE 128-byte line (rows of 4 K bytes); with
// `split_planar` as two planes [Npad][K] (rows of 2 K bytes), the A/B arm of that layout.  f16 has a narrow range: the
// matrix is stored multiplied by a power of two that puts its largest magnitude in [2^13, 2^14); the kernels multiply the
// accumulator by 1 / that.
template <class F>
Packed DenoiserState::pack(const std::string& key, int fmt, int N, int T, int Cin_pad, F get) {
  auto it = dev_w.find(key);
  if (it != dev_w.end()) return it->second;
  const int Npad = (N + 255) / 256 * 256;
  const size_t K = (size_t)T * Cin_pad, total = (size_t)Npad * K;
  const int st = fmt_st(fmt), e = fmt_es(fmt), npl = fmt_split(fmt) ? 2 : 1;
  std::vector<uint8_t> host(total * e * npl, 0);
  const bool inter = npl == 2 && !split_planar;
  const size_t row_bytes = K * e * (inter ? 2 : 1), lo_off = inter ? 64 : total * e;
  // the tile kernels reach a tile's 256 rows, and a lo half, through 32-bit buffer offsets from the tile's first row
  if (npl == 2 && ((K & 31) != 0 || 256 * row_bytes + lo_off >= 0x7f000000ull))
    throw std::runtime_error("split weight " + key + ": K must be a multiple of 32 and a 256-row tile span less than 2 GiB");
  const int nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  float mul = 1.0f;
  if (st == ST_F16) {
    std::vector<float> mx(nthreads, 0.0f);
    std::vector<std::thread> th;
    for (int ti = 0; ti < nthreads; ++ti)
      th.emplace_back([&, ti]() {
        float m = 0.f;
        for (int n = ti; n < N; n += nthreads)
          for (int t = 0; t < T; ++t)
            for (int ci = 0; ci < Cin_pad; ++ci) m = std::max(m, std::fabs(get(n, t, ci)));
        mx[ti] = m;
      });
    for (auto& t : th) t.join();
    const float m = *std::max_element(mx.begin(), mx.end());
    if (m > 0.f && std::isfinite(m)) {
      int ex;
      std::frexp(m, &ex);                      // m = f * 2^ex, f in [0.5, 1)
      mul = std::ldexp(1.0f, 14 - ex);         // m * mul in [2^13, 2^14)
    }
  }
  std::vector<std::thread> th;
  for (int ti = 0; ti < nthreads; ++ti) {
    th.emplace_back([&, ti]() {
      for (int n = ti; n < N; n += nthreads) {
        for (int t = 0; t < T; ++t)
          for (int ci = 0; ci < Cin_pad; ++ci) {
            const float v = get(n, t, ci) * mul;
            const size_t idx = (size_t)n * K + (size_t)t * Cin_pad + ci;
            if (st == ST_F32) { ((float*)host.data())[idx] = v; continue; }
            const size_t k = (size_t)t * Cin_pad + ci;
            uint16_t* hi = (uint16_t*)(host.data() + (inter ? (size_t)n * row_bytes + (k >> 5) * 128 + (k & 31) * 2 : idx * 2));
            uint16_t* lo = (uint16_t*)((uint8_t*)hi + lo_off);
            if (st == ST_BF16) {
              *hi = f2bf_host(v);
              if (npl == 2) *lo = f2bf_host(v - bf2f_host(*hi));
            } else {
              *hi = f2h_host(v);
              if (npl == 2) *lo = f2h_host(v - h2f_host(*hi));
            }
          }
      }
    });
  }
  for (auto& t : th) t.join();
  Packed pk;
  pk.p = dalloc(total * e * npl, false);
  pk.plane = npl == 2 ? (long long)lo_off : 0;
  pk.row_bytes = (int)row_bytes;
  pk.chunk_step = inter ? 128 : 64;
  pk.scale = 1.0f / mul;
  if (hipMemcpy(pk.p, host.data(), total * e * npl, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("memcpy");
  dev_w[key] = pk;
  return pk;
}

// a named activation buffer of `rows` samples in format `fmt`
Act DenoiserState::make_act(const std::string& name, int L, int C, bool padded, int fmt, int rows) {
  Act a;
  a.L = L; a.C = C; a.ld = C; a.coff = 0; a.padded = padded; a.fmt = fmt;
  const size_t bytes = (size_t)rows * a.Lp() * C * fmt_es(fmt);
  const int npl = fmt_split(fmt) ? 2 : 1;
  a.plane = npl == 2 ? (long long)bytes : 0;
  // split formats reach the lo plane through a 32-bit buffer offset from the tile base (2 GiB descriptor range)
  if (npl == 2 && bytes >= 0x7f000000ull) throw std::runtime_error("activation plane of 2 GiB or more: lower the reserved batch");
  a.p = dalloc(bytes * npl);
  named[name] = a;
  return a;
}
Act DenoiserState::make_act(const std::string& name, int L, int C, bool padded) { return make_act(name, L, C, padded, ufmt, Bmax); }

// ------------------------------------------------------------------ GEMM op builders
// What every GEMM of the plan fills alike: operands and their row geometry, the weight, bias and the f16 range-guard slot; mode
// MODE_BIAS.  M follows per call (rows of the batch at hand).
ConvGemmParams DenoiserState::gemm_params(const Act& in, const Act& out, const Packed& wp, int taps, int Cin, int Cout, int in_stride,
                                          int in_off, int out_stride, int out_off, int L, const float* bias, int* sat) {
  ConvGemmParams p{};
  p.A = aptr(in); p.lda = in.ld; p.in_Lp = in.Lp(); p.in_stride = in_stride; p.in_off = in_off; p.taps = taps; p.Cin = Cin;
  p.W = wp.p; p.w_plane = wp.plane; p.w_row = wp.row_bytes; p.w_step = wp.chunk_step; p.w_scale = wp.scale;
  p.a_plane = in.plane; p.out_plane = out.plane;
  p.sat = sat;
  p.Out = (void*)aptr(out); p.ldc = out.ld; p.out_Lp = out.Lp(); p.out_stride = out_stride; p.out_off = out_off;
  p.L = L; p.N = Cout; p.bias = bias; p.mode = MODE_BIAS;
  return p;
}
// ... of a U-Net layer `wname`: its bias, and its guard slot
ConvGemmParams DenoiserState::gemm_params(const Act& in, const Act& out, const Packed& wp, int taps, int Cin, int Cout, int in_stride,
                                          int in_off, int out_stride, int out_off, int L, const std::string& wname) {
  int* sat = sat_slot(wname, ufmt);
  return gemm_params(in, out, wp, taps, Cin, Cout, in_stride, in_off, out_stride, out_off, L, vec(wname + ".bias"), sat);
}
// the epilogue of a conv block: GroupNorm(8) `gn` + Mish (+ FiLM at column `film_off` | + residual `res`)
void DenoiserState::set_epilogue(ConvGemmParams& p, int mode, const std::string& gn, int film_off, const Act* res) {
  p.mode = mode; p.eps = 1e-5f;
  if (mode >= MODE_GN_MISH) {
    p.gamma = vec(gn + ".weight"); p.beta = vec(gn + ".bias"); p.group_ch = p.N / 8;
  }
  if (mode == MODE_GN_MISH_FILM) { p.film = film; p.film_ld = film_cols; p.film_off = film_off; }
  if (mode == MODE_GN_MISH_RES) {
    p.Res = aptr(*res); p.ldres = res->ld; p.res_Lp = res->Lp(); p.res_off = res->padded ? 1 : 0; p.res_plane = res->plane;
  }
}
// a plain GEMM op: conv + bias on the Bp samples of a call
void DenoiserState::push_gemm(const ConvGemmParams& p_in) {
  const int uf = ufmt;
  unet_ops.push_back([this, p = p_in, uf](int, int Bp, hipStream_t s) mutable {
    p.M = Bp * p.L;
    run_gemm(p, uf, s);
  });
}
// a matrix GEMM (FiLM, the encoder's fc): `rows` rows, or the whole 256-row tiles that hold them (rows beyond are scratch rows)
void DenoiserState::run_rows(ConvGemmParams p, int rows, bool whole_tiles, int fmt, hipStream_t s) {
  const int Mr = whole_tiles ? (rows + 255) / 256 * 256 : rows;
  p.M = Mr; p.L = Mr; p.in_Lp = Mr; p.out_Lp = Mr;
  run_gemm(p, fmt, s);
}
// Conv1d(k = 3, pad 1) [+ GroupNorm(8) + Mish (+ FiLM | + residual)] on padded activations.
void DenoiserState::add_conv3(const std::string& wname, const Act& in, const Act& out, int mode, const std::string& gn, int film_off,
                              const Act* res) {
  const HostParam& w = P_(wname + ".weight");
  const int Cout = (int)w.dims[0], Cin = (int)w.dims[1];
  const float* wd = w.data;
  const Packed wp = pack(wname, ufmt, Cout, 3, Cin, [=](int n, int t, int ci) { return wd[((size_t)n * Cin + ci) * 3 + t]; });
  ConvGemmParams p = gemm_params(in, out, wp, 3, Cin, Cout, 1, 0, 1, 1, in.L, wname);
  set_epilogue(p, mode, gn, film_off, res);
  emit_block(p, out);
}
// A GEMM whose epilogue is GroupNorm(8) + Mish (+ FiLM | + residual).  The fused epilogue needs whole GroupNorm
// groups inside a 256-channel tile: 64, 128 or 256 channels per group (C_out 512 / 1024 / 2048, the `large`
// denoiser).  Other sizes run conv + bias in the GEMM and the normalisation / Mish / FiLM / residual in gn1d_kernel.
void DenoiserState::emit_block(const ConvGemmParams& p, const Act& out) {
  const int Cout = p.N, L = p.L, uf = ufmt;
  const int gch = Cout / 8;
  // ... and a lane's four accumulator rows inside one sample: 16 | L, or L = 8 / 4 on the 16-bit tiles (the ant config's lower
  // levels)
  const bool short_fusable = (L == 8 || L == 4) && fmt_st(uf) != ST_F32;
  const bool fused = p.mode < MODE_GN_MISH ||
                     ((Cout & 255) == 0 && (gch == 64 || gch == 128 || gch == 256) && ((L & 15) == 0 || short_fusable));
  // short levels fuse on the gemm16 tile only: whole 256-row tiles (always so for the split formats, batch by batch otherwise)
  const bool fused_needs_tiles = fused && p.mode >= MODE_GN_MISH && (L & 15) != 0;
  ConvGemmParams qf = p, q = p;      // the fused launch; conv + bias alone, its epilogue then read from `qf` by gn1d_kernel
  q.mode = MODE_BIAS;
  unet_ops.push_back([=, this](int, int Bp, hipStream_t s) mutable {
    if (fused && (!fused_needs_tiles || ((Bp * L) & 255) == 0)) {
      qf.M = Bp * L;
      run_gemm(qf, uf, s);
      return;
    }
    q.M = Bp * L;
    run_gemm(q, uf, s);
    prof.note_other();
    // (the normalisation pass reports under the layer's name as well: qf.sat)
    launch_gn1d(out.p, out.ld, out.Lp(), 1, out.coff, L, Cout, qf.gamma, qf.beta, 1e-5f, qf.mode, qf.film, qf.film_ld, qf.film_off,
                qf.Res, qf.ldres, qf.res_Lp, qf.res_off, Bp, uf, out.plane, qf.res_plane, s, qf.sat);
  });
}
// Conv1d(k = 1) residual projection.
void DenoiserState::add_conv1(const std::string& wname, const Act& in, const Act& out) {
  const HostParam& w = P_(wname + ".weight");
  const int Cout = (int)w.dims[0], Cin = (int)w.dims[1];
  const float* wd = w.data;
  const Packed wp = pack(wname, ufmt, Cout, 1, Cin, [=](int n, int, int ci) { return wd[(size_t)n * Cin + ci]; });
  push_gemm(gemm_params(in, out, wp, 1, Cin, Cout, 1, 1, 1, 1, in.L, wname));
}
// Downsample1d: Conv1d(C, C, 3, stride 2, pad 1)  (conv1d_components.py:7-13)
void DenoiserState::add_down(const std::string& wname, const Act& in, const Act& out) {
  const HostParam& w = P_(wname + ".weight");
  const int Cout = (int)w.dims[0], Cin = (int)w.dims[1];
  const float* wd = w.data;
  const Packed wp = pack(wname, ufmt, Cout, 3, Cin, [=](int n, int t, int ci) { return wd[((size_t)n * Cin + ci) * 3 + t]; });
  push_gemm(gemm_params(in, out, wp, 3, Cin, Cout, 2, 0, 1, 1, out.L, wname));
}
// Upsample1d: ConvTranspose1d(C, C, 4, 2, 1) as two 2-tap GEMMs (even / odd outputs)
// out[2m] = W1^T x[m] + W3^T x[m-1];  out[2m+1] = W0^T x[m+1] + W2^T x[m]   (conv1d_components.py:15-21)
void DenoiserState::add_up(const std::string& wname, const Act& in, const Act& out) {
  const HostParam& w = P_(wname + ".weight");                  // [Cin][Cout][4]
  const int Cin = (int)w.dims[0], Cout = (int)w.dims[1];
  const float* wd = w.data;
  for (int par = 0; par < 2; ++par) {
    const int k0 = par == 0 ? 3 : 2, k1 = par == 0 ? 1 : 0;     // tap 0 -> earlier input row
    const Packed wp = pack(wname + (par ? ".odd" : ".even"), ufmt, Cout, 2, Cin, [=](int n, int t, int ci) {
      return wd[((size_t)ci * Cout + n) * 4 + (t == 0 ? k0 : k1)];
    });
    push_gemm(gemm_params(in, out, wp, 2, Cin, Cout, 1, par, 2, 1 + par, in.L, wname));
  }
}

// ConditionalResidualBlock1D (conditional_unet1d.py:41-142)
void DenoiserState::add_crb(const std::string& pre, const Act& in, const Act& out, int& film_cursor, const std::string& tag) {
  const int Cout = (int)P_(pre + ".blocks.0.block.0.weight").dims[0];
  Act h = make_act(tag + ".h", in.L, Cout);
  const int film_off = film_cursor;
  film_cursor += 2 * Cout;
  add_conv3(pre + ".blocks.0.block.0", in, h, MODE_GN_MISH_FILM, pre + ".blocks.0.block.1", film_off, nullptr);
  Act res = in;
  if (has(pre + ".residual_conv.weight")) {
    res = make_act(tag + ".res", in.L, Cout);
    add_conv1(pre + ".residual_conv", in, res);
  }
  add_conv3(pre + ".blocks.1.block.0", h, out, MODE_GN_MISH_RES, pre + ".blocks.1.block.1", 0, &res);
}

// ------------------------------------------------------------------ the plan
void DenoiserState::build(int prec_, int Bmax_) {
  free_workspace();
  prec = prec_;
  {
    const char* e = getenv("DITREE_SPLIT_PLANAR");          // A/B switch of the split weight layout
    split_planar = e != nullptr && atoi(e) != 0;
  }
  // DITREE_PREC_*  ->  formats of the U-Net and of the encoder (the split instantiations run the encoder split as well: its
  // stem is the fused kernel for both map sizes, 20 x 20 and 16 x 16).
  switch (prec) {
    case DITREE_PREC_BF16: ufmt = fmt_make(ST_BF16, false); efmt = ST_BF16; break;
    case DITREE_PREC_F32: ufmt = fmt_make(ST_F32, false); efmt = ST_F32; break;
    case DITREE_PREC_F16X3: ufmt = fmt_make(ST_F16, true); efmt = ufmt; break;
    case DITREE_PREC_BF16X3: ufmt = fmt_make(ST_BF16, true); efmt = ufmt; break;
    case DITREE_PREC_F16: ufmt = fmt_make(ST_F16, false); efmt = ST_F16; break;
    default: throw std::runtime_error("unknown precision");
  }
  prof.ufmt = ufmt;
  sat_flags = (int*)dalloc(SAT_SLOTS * sizeof(int));
  sat_cond = sat_slot("cond_encoder input: Mish(time | map embedding | observation)", ufmt);
  sat_sample = sat_slot("sample (the noisy action sequence)", ufmt);
  const int C0 = dims[0], C1 = dims[1], C2 = dims[2];
  const int L0 = P, L1 = P / 2, L2 = P / 4;
  if (P % 16 != 0 || P < 16 || P > 256 || (256 % P) != 0) throw std::runtime_error("pred_horizon must be 16, 32, 64, 128 or 256");
  // rows of a batch are padded to whole work units: 16 samples (f32), or -- the 16-bit formats run every level on the 256-row
  // halo / gemm16 tiles (the split formats exist there only; the fused GroupNorm epilogue of the short levels needs whole
  // tiles, and a sample's result must not depend on the batch it is part of) -- as many as fill a tile at the shortest level
  // (P / 4 rows per sample: 64 samples at P = 16)
  bgran = fmt_st(ufmt) != ST_F32 ? std::max(16, 1024 / P) : 16;
  Buser = Bmax_;
  Bmax = (Bmax_ + bgran - 1) / bgran * bgran;
  {
    // The split kernels reach the lo plane through a 32-bit buffer offset, so an activation plane must stay below 2 GiB; and
    // nothing is gained by a workspace beyond a few thousand samples (every layer already launches >> 256 tiles).  Larger
    // calls run as sub-batches of `Bmax` samples (denoise_core): the reserved batch is a capacity, not a workspace size.
    const long long per_sample = std::max({(long long)(L2 + 2) * 2 * C2, (long long)(L1 + 2) * 2 * C1, (long long)(L0 + 2) * C0,
                                           (long long)L0 * 64}) * fmt_es(ufmt);
    long long cap = std::min<long long>(8192, 0x7f000000LL / per_sample);
    cap = cap / 256 * 256;
    if (cap < 256) throw std::runtime_error("denoiser too large for one 256-sample work unit");
    if (Bmax > cap) Bmax = (int)cap;
  }
  if (fmt_split(ufmt) && ((C0 | C1 | C2) & 255) != 0)
    throw std::runtime_error("the split precisions need down_dims that are multiples of 256 (halo / gemm16 tiles)");
  x_cur = (float*)dalloc((size_t)Bmax * P * D * 4);
  temb = (float*)dalloc(256 * 4);
  condK = (cond_dim + 63) / 64 * 64;
  // split encoder: its fc layer runs on the gemm16 tiles too (rows and columns padded to 256)
  E_ld = (enc_kind == ENC_RESNET && fmt_split(efmt)) ? (E + 255) / 256 * 256 : E;      // the small encoders write E columns, no fc tile
  map_emb = (float*)dalloc((size_t)Brows() * E_ld * 4);
  cond_plane = planes() == 2 ? (long long)Brows() * condK * es() : 0;
  condA = dalloc((size_t)Brows() * condK * es() * planes());
  build_film();
  build_unet();
  if (enc_kind != ENC_RESNET) build_encoder_small();
  else build_encoder_resnet();
  if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("sync after build failed");
  validate_plan();
}

// FiLM: all cond_encoder Linear layers batched into one GEMM on whole 256-row tiles (zero rows in, ignored rows out)
void DenoiserState::build_film() {
  std::vector<std::string> crbs = {"unet.down_modules.0.0", "unet.down_modules.0.1", "unet.down_modules.1.0",
                                   "unet.down_modules.1.1", "unet.down_modules.2.0", "unet.down_modules.2.1",
                                   "unet.mid_modules.0",    "unet.mid_modules.1",    "unet.up_modules.0.0",
                                   "unet.up_modules.0.1",   "unet.up_modules.1.0",   "unet.up_modules.1.1"};   // film columns follow this order
  std::vector<const float*> wsrc, bsrc;
  std::vector<int> rows, start;
  film_cols = 0;
  for (auto& c : crbs) {
    wsrc.push_back(P_(c + ".cond_encoder.1.weight").data);
    bsrc.push_back(P_(c + ".cond_encoder.1.bias").data);
    rows.push_back((int)P_(c + ".cond_encoder.1.weight").dims[0]);
    start.push_back(film_cols);
    film_cols += rows.back();
  }
  film = (float*)dalloc((size_t)Brows() * film_cols * 4);
  const int cd = cond_dim;
  const Packed wp = pack("film.all", ufmt, film_cols, 1, condK, [=](int n, int, int ci) {
    size_t i = std::upper_bound(start.begin(), start.end(), n) - start.begin() - 1;
    return ci < cd ? wsrc[i][(size_t)(n - start[i]) * cd + ci] : 0.0f;
  });
  std::vector<float> ball(film_cols);
  for (size_t i = 0; i < rows.size(); ++i) std::memcpy(ball.data() + start[i], bsrc[i], (size_t)rows[i] * 4);
  float* bd = upload_f32("film.bias", ball.data(), film_cols);
  ConvGemmParams p = gemm_params(matrix(condA, condK, cond_plane), matrix(film, film_cols), wp, 1, condK, film_cols, 1, 0, 1, 0, 0, bd,
                                 nullptr);
  p.out_f32 = 1;
  const int uf = ufmt;
  film_op = [this, p, uf](int, int Bp, hipStream_t s) { run_rows(p, Bp, fmt_st(uf) != ST_F32, uf, s); };
}

void DenoiserState::build_unet() {
  const int C0 = dims[0], C1 = dims[1], C2 = dims[2];
  const int L0 = P, L1 = P / 2, L2 = P / 4;
  // first layer input: im2col rows [x[l-1], x[l], x[l+1]] padded to 64 columns, unpadded rows
  Act a0 = make_act("a0", L0, 64, false);
  const std::string pre = "unet.down_modules.0.0";
  int fc = (int)P_(pre + ".cond_encoder.1.weight").dims[0];   // film cursor: the blocks' columns in build_film's order
  {
    // down 0, block 1: Conv1d(D, C0, 3) as a 1-tap GEMM over the im2col rows
    const float* wd = P_(pre + ".blocks.0.block.0.weight").data;
    const int Dd = D;
    const Packed wp = pack(pre + ".blocks.0.block.0", ufmt, C0, 1, 64, [=](int n, int, int ci) {
      if (ci >= 3 * Dd) return 0.0f;
      const int t = ci / Dd, d = ci - t * Dd;
      return wd[((size_t)n * Dd + d) * 3 + t];
    });
    Act h = make_act("d0b1.h", L0, C0);
    ConvGemmParams p = gemm_params(a0, h, wp, 1, 64, C0, 1, 0, 1, 1, L0, pre + ".blocks.0.block.0");
    set_epilogue(p, MODE_GN_MISH_FILM, pre + ".blocks.0.block.1", 0, nullptr);
    emit_block(p, h);
    // residual Conv1d(D, C0, 1): centre-tap columns of the same rows
    const float* wrd = P_(pre + ".residual_conv.weight").data;
    const Packed wrp = pack(pre + ".residual_conv", ufmt, C0, 1, 64, [=](int n, int, int ci) {
      return (ci >= Dd && ci < 2 * Dd) ? wrd[(size_t)n * Dd + (ci - Dd)] : 0.0f;
    });
    Act res = make_act("d0b1.res", L0, C0);
    push_gemm(gemm_params(a0, res, wrp, 1, 64, C0, 1, 0, 1, 1, L0, pre + ".residual_conv"));
    Act o = make_act("d0b1.out", L0, C0);
    add_conv3(pre + ".blocks.1.block.0", h, o, MODE_GN_MISH_RES, pre + ".blocks.1.block.1", 0, &res);
  }
  Act cat1 = make_act("cat1", L1, 2 * C1);        // [x_up (C1) | skip1 (C1)] at L1
  Act cat0 = make_act("cat0", L2, 2 * C2);        // [x_mid (C2) | skip2 (C2)] at L2
  Act d0o = named["d0b1.out"];
  Act skip0 = make_act("skip0", L0, C0);
  add_crb("unet.down_modules.0.1", d0o, skip0, fc, "d0b2");
  Act d1in = make_act("d1.in", L1, C0);
  add_down("unet.down_modules.0.2.conv", skip0, d1in);
  Act d1o = make_act("d1b1.out", L1, C1);
  add_crb("unet.down_modules.1.0", d1in, d1o, fc, "d1b1");
  Act skip1 = view(cat1, C1, C1);
  named["skip1"] = skip1;
  add_crb("unet.down_modules.1.1", d1o, skip1, fc, "d1b2");
  Act d2in = make_act("d2.in", L2, C1);
  add_down("unet.down_modules.1.2.conv", skip1, d2in);
  Act d2o = make_act("d2b1.out", L2, C2);
  add_crb("unet.down_modules.2.0", d2in, d2o, fc, "d2b1");
  Act skip2 = view(cat0, C2, C2);
  named["skip2"] = skip2;
  add_crb("unet.down_modules.2.1", d2o, skip2, fc, "d2b2");
  Act m1 = make_act("mid1.out", L2, C2);
  add_crb("unet.mid_modules.0", skip2, m1, fc, "mid1");
  Act m2 = view(cat0, 0, C2);
  named["mid2.out"] = m2;
  add_crb("unet.mid_modules.1", m1, m2, fc, "mid2");
  Act u0a = make_act("u0b1.out", L2, C1);
  add_crb("unet.up_modules.0.0", cat0, u0a, fc, "u0b1");
  Act u0b = make_act("u0b2.out", L2, C1);
  add_crb("unet.up_modules.0.1", u0a, u0b, fc, "u0b2");
  Act up0 = view(cat1, 0, C1);
  named["up0.out"] = up0;
  add_up("unet.up_modules.0.2.conv", u0b, up0);
  Act u1a = make_act("u1b1.out", L1, C0);
  add_crb("unet.up_modules.1.0", cat1, u1a, fc, "u1b1");
  Act u1b = make_act("u1b2.out", L1, C0);
  add_crb("unet.up_modules.1.1", u1a, u1b, fc, "u1b2");
  Act fin = make_act("final.in", L0, C0);
  add_up("unet.up_modules.1.2.conv", u1b, fin);
  final_h = make_act("final.h", L0, C0);
  add_conv3("unet.final_conv.0.block.0", fin, final_h, MODE_GN_MISH, "unet.final_conv.0.block.1", 0, nullptr);
  vec("unet.final_conv.1.weight");
  vec("unet.final_conv.1.bias");
  vec("unet.diffusion_step_encoder.1.weight");
  vec("unet.diffusion_step_encoder.1.bias");
  vec("unet.diffusion_step_encoder.3.weight");
  vec("unet.diffusion_step_encoder.3.bias");
}

// one of the five small encoders: a single f32 launch (encoder_kernels.hip), whatever the precision
void DenoiserState::build_encoder_small() {
  SmallEncoderParams q{};
  q.kind = enc_kind; q.n = lm; q.E = E; q.k = enc_k;
  auto transposed = [&](const std::string& name, int out_f, int in_f) {       // Linear weight (out, in) -> [in][out]
    const HostParam& w = P_(name);
    if (w.dims.size() != 2 || w.dims[0] != out_f || w.dims[1] != in_f)
      throw std::runtime_error(name + " must be (" + std::to_string(out_f) + ", " + std::to_string(in_f) + ")");
    std::vector<float> t((size_t)out_f * in_f);
    for (int o = 0; o < out_f; ++o)
      for (int i = 0; i < in_f; ++i) t[(size_t)i * out_f + o] = w.data[(size_t)o * in_f + i];
    return upload_f32(name + "#t", t.data(), (int64_t)t.size());
  };
  auto conv_w = [&](const std::string& name, int co, int ci) {
    const HostParam& w = P_(name + ".weight");
    const HostParam& b = P_(name + ".bias");
    if (w.dims.size() != 4 || w.dims[0] != co || w.dims[1] != ci || w.dims[2] != 3 || w.dims[3] != 3 || b.n != co)
      throw std::runtime_error(name + " must be a Conv2d(" + std::to_string(ci) + ", " + std::to_string(co) + ", 3)");
  };
  if (enc_kind == ENC_MLP) {
    const int in_f = lm * lm;
    q.w[0] = transposed("encoder.fc1.weight", 128, in_f);
    q.w[1] = transposed("encoder.fc2.weight", 256, 128);
    q.w[2] = transposed("encoder.fc3.weight", E, 256);
    const int outs[3] = {128, 256, E};
    for (int l = 0; l < 3; ++l) {
      const std::string bn = "encoder.fc" + std::to_string(l + 1) + ".bias";
      if (P_(bn).n != outs[l]) throw std::runtime_error(bn + " must have " + std::to_string(outs[l]) + " elements");
      q.b[l] = vec(bn);
    }
  } else if (enc_kind == ENC_GRID || enc_kind == ENC_CNN) {
    const bool g = enc_kind == ENC_GRID;
    const int nl = g ? 3 : 4;
    const int ci[4] = {1, g ? 3 : 2, g ? 6 : 4, 4}, co[4] = {g ? 3 : 2, g ? 6 : 4, 4, 4};
    for (int l = 0; l < nl; ++l) {
      const std::string nm = "encoder.conv" + std::to_string(l + 1);
      conv_w(nm, co[l], ci[l]);
      q.w[l] = vec(nm + ".weight");
      q.b[l] = vec(nm + ".bias");
    }
  }
  q.out = map_emb;
  enc_ops.push_back([this, q](int B, int, hipStream_t s) {
    prof.note_other();
    SmallEncoderParams r = q;
    r.lm = lm_ptr; r.B = B;
    launch_small_encoder(r, s);
  });
}

// ResNet-18 with GroupNorm(C/16), NHWC: the fused stem, then implicit-GEMM convs (f32 output, split-K slabs) + GN kernels
// (the layers are small: 8..100 tiles each, far fewer than the 256 CUs)
void DenoiserState::build_encoder_resnet() {
  const std::string R = "encoder.resnet18.";
  const int pr = efmt;
  const void* zero_row = dalloc(256);                             // source of out-of-map taps
  const size_t gout_per_sample = 9216;                            // f32 GEMM output per sample: up to 8 split-K slabs of 9 * 128
  float* gout = (float*)dalloc((size_t)Bmax * gout_per_sample * 4);
  // (the pooled vector feeds a GEMM on whole 256-row tiles)
  auto ebuf = [&](const std::string& name, int HW, int C) { return make_act(name, HW, C, false, efmt, HW == 1 ? Brows() : Bmax); };
  // implicit-GEMM conv (the kernel gathers the (tap, channel-chunk) rows itself) -> f32 output in `gout`, as `splitk` slabs
  // of partial sums; returns splitk for the GroupNorm op that adds them
  auto conv2d = [&](const std::string& wname, const Act& in, int H, int Cout, int k, int stride, int pad, int OH) {
    const HostParam& w = P_(wname + ".weight");
    const float* wd = w.data;
    const int Cw = (int)w.dims[1], Cin = in.C;
    const TapList tl = live_taps(k, stride, pad, H, OH);
    if (Cin % 64 != 0 || tl.n > 12)
      throw std::runtime_error("encoder conv " + wname + " (" + std::to_string(Cin) + " input channels, " + std::to_string(tl.n) +
                               " live taps) fits no implicit-GEMM tile: channels in multiples of 64, at most 12 taps");
    const int K = tl.n * Cin;
    if ((size_t)OH * OH * Cout > gout_per_sample) throw std::runtime_error("encoder scratch region too small for " + wname);
    const Packed wp = pack(wname, efmt, Cout, 1, K, [=](int n, int, int kk) {
      const int c = kk % Cin, t = kk / Cin, kw = tl.kw[t], kh = tl.kh[t];
      return wd[(((size_t)n * Cw + c) * k + kh) * k + kw];
    });
    ConvGemmParams p = gemm_params(in, matrix(gout, Cout), wp, tl.n, Cin, Cout, 1, 0, 1, 0, 0, nullptr, nullptr);
    p.out_f32 = 1;
    p.c2d = 1; p.c2_H = H; p.c2_W = H; p.c2_OW = OH; p.c2_OHW = OH * OH; p.c2_stride = stride; p.c2_pad = pad;
    for (int t = 0; t < tl.n; ++t) { p.c2_kh[t] = tl.kh[t]; p.c2_kw[t] = tl.kw[t]; }
    p.zero = zero_row;
    // split-K: these layers have few tiles and long K loops; spread the K-steps over idle CUs.  The factor depends on the
    // layer only (sized for 1024 candidates), never on the batch, so that a candidate's result does not depend on which other
    // candidates share its launch (bitwise).  Aimed at one work-group per CU on the 256 x 256 tiles, at three per CU on the
    // 64 x 64 tiles (conv2d_small_eligible): split only the layers that cannot fill those slots.
    const int nk_total = tl.n * (Cin / 64);
    const bool small = conv2d_small_eligible(pr);
    const int tiles = small ? ((1024 * OH * OH + 63) / 64) * (Cout / 64) : ((1024 * OH * OH + 255) / 256) * ((Cout + 255) / 256);
    int sk = std::max(1, std::min(std::min(8, nk_total / 2), (small ? 768 : 256) / tiles));
    while (sk > 1 && (size_t)sk * OH * OH * Cout > gout_per_sample) --sk;
    if (sk > 1) {                                   // every split must own at least one K-step
      const int per = (nk_total + sk - 1) / sk;
      sk = (nk_total + per - 1) / per;
    }
    p.splitk = sk;
    enc_ops.push_back([this, p, pr, OHW = OH * OH](int B, int, hipStream_t s) mutable {
      const int M = B * OHW;
      p.M = M; p.L = M; p.in_Lp = M; p.out_Lp = M;
      p.slab_stride = (long long)M * p.N;
      run_gemm(p, pr, s);
    });
    return sk;
  };
  // GroupNorm over the `splitk` slabs the conv before it left in `gout` (+ residual, + ReLU) -> activation `out`
  auto gn = [&](const std::string& gname, int splitk, const Act& out, const Act* res, bool relu) {
    float* ga = vec(gname + ".weight");
    float* be = vec(gname + ".bias");
    const void* rp = res ? res->p : nullptr;
    const int HW = out.L, C = out.C;
    const long long rpl = res ? res->plane : 0;
    {                                                  // shape contract of gn2d_kernel, checked when the plan is built
      const int pp = (C >= 64 && C <= 1024 && (C & (C - 1)) == 0) ? 256 / (C >> 2) : 0;
      if (pp == 0 || (HW + pp - 1) / pp > 7)
        throw std::runtime_error("encoder GroupNorm: unsupported map (" + std::to_string(HW) + " pixels x " + std::to_string(C) + " channels)");
    }
    int* gsat = sat_slot(gname, efmt);
    enc_ops.push_back([=, this](int B, int, hipStream_t s) {
      prof.note_other();
      launch_gn2d(gout, splitk, (long long)B * HW * C, ga, be, rp, relu ? 1 : 0, out.p, B, HW, C, 1e-5f, pr, rpl, out.plane, s, gsat);
    });
  };
  const int H0 = lm;
  auto osz = [](int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; };
  const int H2 = osz(osz(H0, 7, 2, 3), 3, 2, 1);       // 20 -> 10 -> 5, 16 -> 8 -> 4
  Act pool = ebuf("enc.pool", H2 * H2, 64);
  {
    // the stem in one launch: conv 7x7/2 (x.repeat(1,3,1,1): the identical input channels fold into one) + GroupNorm + ReLU +
    // max-pool
    const HostParam& w = P_(R + "conv1.weight");
    const int Cw = (int)w.dims[1];
    std::vector<float> wf(64 * 49);
    for (int n = 0; n < 64; ++n)
      for (int t = 0; t < 49; ++t) {
        float sacc = 0.f;
        for (int cc = 0; cc < Cw; ++cc) sacc += w.data[((size_t)n * Cw + cc) * 49 + t];
        wf[t * 64 + n] = sacc;                       // tap-major: lanes (channels) read consecutive floats
      }
    float* wdev = upload_f32(R + "conv1.weight#folded", wf.data(), 64 * 49);
    float* ga = vec(R + "bn1.weight");
    float* be = vec(R + "bn1.bias");
    int* ssat = sat_slot(R + "conv1", efmt);
    enc_ops.push_back([=, this](int B, int, hipStream_t s) {
      prof.note_other();
      launch_encoder_stem(lm_ptr, H0, wdev, ga, be, pool.p, B, 1e-5f, pr, pool.plane, s, ssat);
    });
  }
  Act cur = pool;
  int Hc = H2;
  const int chans[4] = {64, 128, 256, 512};
  for (int li = 0; li < 4; ++li) {
    for (int bi = 0; bi < 2; ++bi) {
      const std::string pre = R + "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      const int Cout = chans[li];
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      const int Ho = osz(Hc, 3, stride, 1);
      const std::string tag = "enc.l" + std::to_string(li + 1) + "." + std::to_string(bi);
      Act t1 = ebuf(tag + ".t", Ho * Ho, Cout);
      gn(pre + ".bn1", conv2d(pre + ".conv1", cur, Hc, Cout, 3, stride, 1, Ho), t1, nullptr, true);
      Act idt = cur;
      if (has(pre + ".downsample.0.weight")) {
        Act ds = ebuf(tag + ".ds", Ho * Ho, Cout);
        gn(pre + ".downsample.1", conv2d(pre + ".downsample.0", cur, Hc, Cout, 1, stride, 0, Ho), ds, nullptr, false);
        idt = ds;
      }
      Act o = ebuf(tag + ".out", Ho * Ho, Cout);
      gn(pre + ".bn2", conv2d(pre + ".conv2", t1, Ho, Cout, 3, 1, 1, Ho), o, &idt, true);
      cur = o;
      Hc = Ho;
    }
  }
  Act pooled = ebuf("enc.avg", 1, cur.C);
  enc_ops.push_back([=, this](int B, int, hipStream_t s) {
    prof.note_other();
    launch_avgpool2d(cur.p, pooled.p, B, cur.L, cur.C, pr, cur.plane, pooled.plane, s);
  });
  {
    const HostParam& w = P_(R + "fc.weight");
    const float* wd = w.data;
    const int Kf = (int)w.dims[1], Nf = (int)w.dims[0];
    const Packed wp = pack(R + "fc", efmt, Nf, 1, Kf, [=](int n, int, int ci) { return wd[(size_t)n * Kf + ci]; });
    const bool esplit = fmt_split(efmt);
    float* bd;
    if (esplit) {                                        // gemm16 tiles: columns padded to E_ld (zero weights, zero bias)
      std::vector<float> bpad(E_ld, 0.0f);
      std::memcpy(bpad.data(), P_(R + "fc.bias").data, (size_t)Nf * 4);
      bd = upload_f32(R + "fc.bias#padded", bpad.data(), E_ld);
    } else {
      bd = vec(R + "fc.bias");
    }
    ConvGemmParams p = gemm_params(matrix(pooled.p, Kf, pooled.plane), matrix(map_emb, E_ld), wp, 1, Kf, esplit ? E_ld : Nf, 1, 0, 1, 0,
                                   0, bd, nullptr);
    p.out_f32 = 1;
    // split: whole tiles (rows beyond B are scratch rows)
    enc_ops.push_back([this, p, pr, esplit](int B, int, hipStream_t s) { run_rows(p, B, esplit, pr, s); });
  }
}

// Validation pass: every op of the plan once in DRY-RUN mode (the launchers run their dispatch and shape contracts, nothing is
// enqueued).  Any layer whose shape fits no kernel (a future kernel_size / n_groups / embedding width) throws HERE, i.e.
// ditree_denoise_reserve returns an error -- not the first denoise call, and never an abort of the host process.
void DenoiserState::validate_plan() {
  float* lm_dev = (float*)dalloc((size_t)bgran * lm * lm * 4);
  lm_ptr = lm_dev;
  denoise_set_dry_run(true);
  try {
    for (auto& op : enc_ops) op(bgran, bgran, nullptr);
    film_op(bgran, bgran, nullptr);
    for (auto& op : unet_ops) op(bgran, bgran, nullptr);
  } catch (...) {
    denoise_set_dry_run(false);
    lm_ptr = nullptr;
    throw;
  }
  denoise_set_dry_run(false);
  lm_ptr = nullptr;
}
