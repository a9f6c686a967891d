// Small kernels of the DiTree denoiser and its local-map encoder (gfx950): GroupNorm, encoder stem, sample / condition
// preparation, time embedding, final projection, im2col, pooling, unpacking -- with their launchers.
#include "denoise_device.h"

// x (B, P, D) f32 -> A0 rows (b, l): [x[l-1,:], x[l,:], x[l+1,:], 0 ...] (K padded to 64): the
// im2col of the first Conv1d(D -> C, 3) (conditional_unet1d.py:214-218 with dim_in = input_dim).
// GroupNorm(8 groups) + Mish (+ FiLM | + residual) in place on a padded channels-last activation: the unfused form
// of the GEMM epilogue, for channel counts whose groups do not map onto the 256-channel GEMM tiles (the reference's
// denoiser sizes other than `large`: C/8 < 64 or > 256 channels per group).  conv1d_components.py:23-40,
// conditional_unet1d.py:110-141.  One 256-thread work-group per (sample, group); a thread walks 8-channel vectors;
// mean, then centred squares, then the update: three passes over at most 16 KB that stay in L2.
template <int PREC>
__global__ void __launch_bounds__(256) gn1d_kernel(void* __restrict__ x, int ld, int Lp, int row_off, int coff, int L, int C,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                   int mode, const float* __restrict__ film, int film_ld, int film_off,
                                                   const void* __restrict__ res, int ldres, int res_Lp, int res_off,
                                                   long long x_plane, long long res_plane, int* __restrict__ sat) {
  __shared__ float red[8];
  float satm = 0.0f;
  const int b = blockIdx.x >> 3, g = blockIdx.x & 7;
  const int gc = C >> 3, vpr = gc >> 3, nvec = L * vpr;          // channels per group, 8-channel vectors per row
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto at = [&](int v, int& l, int& c) { l = v / vpr; c = g * gc + (v - l * vpr) * 8; };
  auto load8 = [&](int l, int c, float (&o)[8]) {
    const long long idx = ((long long)b * Lp + l + row_off) * ld + coff + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = load_elem<PREC>(x, idx + j, x_plane);
  };
  auto wg_sum = [&](float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
  };
  float s = 0.f;
  for (int v = tid; v < nvec; v += 256) {
    int l, c; at(v, l, c);
    float o[8]; load8(l, c, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += o[j];
  }
  const float inv_n = 1.0f / (float)(L * gc);
  const float mean = wg_sum(s) * inv_n;
  float q = 0.f;
  for (int v = tid; v < nvec; v += 256) {
    int l, c; at(v, l, c);
    float o[8]; load8(l, c, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = o[j] - mean; q = fmaf(d, d, q); }
  }
  const float rstd = rsqrtf(wg_sum(q) * inv_n + eps);
  for (int v = tid; v < nvec; v += 256) {
    int l, c; at(v, l, c);
    float o[8]; load8(l, c, o);
    const long long idx = ((long long)b * Lp + l + row_off) * ld + coff + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float y = MISH_OF(PREC)((o[j] - mean) * rstd * gamma[c + j] + beta[c + j]);
      if (mode == MODE_GN_MISH_FILM) {
        const float* fr = film + (long long)b * film_ld + film_off + c + j;
        y = y * fr[0] + fr[C];
      } else if (mode == MODE_GN_MISH_RES) {
        y += load_elem<PREC>(res, ((long long)b * res_Lp + l + res_off) * ldres + c + j, res_plane);
      }
      store_elem<PREC>(x, idx + j, y, x_plane, satm);
    }
  }
  if constexpr ((PREC & 3) == ST_F16) sat_flush(sat, satm);
}
// The same for short sequences in the 16-bit formats (the ant config's L = 8 and 4 levels: a (sample, group) is 128
// 8-channel vectors): one WAVE per (sample, group), its vectors (up to four per lane) stay in registers -- one 16-byte load
// per vector and plane, statistics by wave reductions, one 16-byte store per vector and plane; four (sample, group)s per
// work-group.  Same arithmetic as gn1d_kernel (mean, then centred squares), so results are identical.
template <int FMT>
__global__ void __launch_bounds__(256) gn1d_short_kernel(void* __restrict__ x, int ld, int Lp, int row_off, int coff, int L, int C,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, int mode, const float* __restrict__ film, int film_ld,
                                                         int film_off, const void* __restrict__ res, int ldres, int res_Lp,
                                                         int res_off, long long x_plane, long long res_plane, int n_sg,
                                                         int* __restrict__ sat) {
  constexpr int ET = (FMT & 3) == ST_F16 ? 1 : 0;
  constexpr bool SPL = (FMT & 4) != 0;
  float satm = 0.0f;
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= n_sg) return;
  const int b = sg >> 3, g = sg & 7;
  const int gc = C >> 3, vpr = gc >> 3, nvec = L * vpr;
  float v[4][8];
  long long idx[4];
  int cc[4], ll[4];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int vi = lane + 64 * k;
    if (vi < nvec) {
      const int l = vi / vpr, c = g * gc + (vi - l * vpr) * 8;
      ll[k] = l; cc[k] = c;
      idx[k] = ((long long)b * Lp + l + row_off) * ld + coff + c;
      const short8_t h = *(const short8_t*)((const char*)x + idx[k] * 2);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = e2f<ET>((unsigned short)h[j]);
      if constexpr (SPL) {
        const short8_t lo = *(const short8_t*)((const char*)x + x_plane + idx[k] * 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] += e2f<ET>((unsigned short)lo[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[k][j];
    }
  }
  auto wave_sum = [&](float t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m);
    return t;
  };
  const float inv_n = 1.0f / (float)(L * gc);
  const float mean = wave_sum(s) * inv_n;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[k][j] - mean; q = fmaf(d, d, q); }
    }
  const float rstd = rsqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (lane + 64 * k < nvec) {
      const int c = cc[k];
      const f32x4_t g0 = *(const f32x4_t*)(gamma + c), g1 = *(const f32x4_t*)(gamma + c + 4);
      const f32x4_t b0 = *(const f32x4_t*)(beta + c), b1 = *(const f32x4_t*)(beta + c + 4);
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        y[j] = MISH_OF(FMT)((v[k][j] - mean) * rstd * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? b0[j & 3] : b1[j & 3]));
      if (mode == MODE_GN_MISH_FILM) {
        const float* fr = film + (long long)b * film_ld + film_off + c;
        const f32x4_t s0 = *(const f32x4_t*)fr, s1 = *(const f32x4_t*)(fr + 4);
        const f32x4_t t0 = *(const f32x4_t*)(fr + C), t1 = *(const f32x4_t*)(fr + C + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = y[j] * (j < 4 ? s0[j & 3] : s1[j & 3]) + (j < 4 ? t0[j & 3] : t1[j & 3]);
      } else if (mode == MODE_GN_MISH_RES) {
        const long long ri = ((long long)b * res_Lp + ll[k] + res_off) * ldres + c;
        const short8_t rh = *(const short8_t*)((const char*)res + ri * 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] += e2f<ET>((unsigned short)rh[j]);
        if constexpr (SPL) {
          const short8_t rl = *(const short8_t*)((const char*)res + res_plane + ri * 2);
#pragma unroll
          for (int j = 0; j < 8; ++j) y[j] += e2f<ET>((unsigned short)rl[j]);
        }
      }
      short8_t oh, ol;
      if constexpr (ET == 1) {
#pragma unroll
        for (int j = 0; j < 8; j += 2) sat_see2(satm, y[j], y[j + 1]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned short hh = f2e<ET>(y[j]);
        oh[j] = (short)hh;
        if constexpr (SPL) ol[j] = (short)f2e<ET>(y[j] - e2f<ET>(hh));
      }
      *(short8_t*)((char*)x + idx[k] * 2) = oh;
      if constexpr (SPL) *(short8_t*)((char*)x + x_plane + idx[k] * 2) = ol;
    }
  if constexpr (ET == 1) sat_flush(sat, satm);
}
void launch_gn1d(void* x, int ld, int Lp, int row_off, int coff, int L, int C, const float* gamma, const float* beta, float eps,
                 int mode, const float* film, int film_ld, int film_off, const void* res, int ldres, int res_Lp, int res_off,
                 int B, int fmt, long long x_plane, long long res_plane, hipStream_t s, int* sat) {
  // short (sample, group)s in a 16-bit format, 16-byte aligned vectors: the one-wave form
  if (fmt_st(fmt) != ST_F32 && L * (C >> 6) <= 256 && (C & 63) == 0 && (ld & 7) == 0 && (coff & 7) == 0 &&
      (mode != MODE_GN_MISH_RES || (ldres & 7) == 0) && (mode != MODE_GN_MISH_FILM || ((film_ld | film_off) & 3) == 0)) {
    const int n_sg = B * 8;
#define CALLS(F) DN_LAUNCH(gn1d_short_kernel<F>, dim3((n_sg + 3) / 4), dim3(256), 0, s, x, ld, Lp, row_off, coff, L, C, gamma, \
                                    beta, eps, mode, film, film_ld, film_off, res, ldres, res_Lp, res_off, x_plane, res_plane, n_sg, sat)
    switch (fmt) {
      case 0: CALLS(0); break;
      case 2: CALLS(2); break;
      case 4: CALLS(4); break;
      case 6: CALLS(6); break;
      default: throw std::runtime_error("gn1d: unknown 16-bit format");
    }
#undef CALLS
    return;
  }
#define CALL(F) DN_LAUNCH(gn1d_kernel<F>, dim3(B * 8), dim3(256), 0, s, x, ld, Lp, row_off, coff, L, C, gamma, beta, eps, \
                                   mode, film, film_ld, film_off, res, ldres, res_Lp, res_off, x_plane, res_plane, sat)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

// Encoder stem in one launch: Conv2d(1 -> 64, 7x7, stride 2, pad 3; the three identical input channels of
// x.repeat(1,3,1,1) are folded into the weights) + GroupNorm(4 groups of 16 channels) + ReLU + MaxPool(3, 2, 1)
// (local_map_encoder.py:101-122 through torchvision's resnet18 stem).  One 256-thread work-group per sample:
// the padded 26 x 26 map and the 64 x 49 f32 weights sit in LDS / registers, thread (c = tid & 63, q = tid >> 6)
// computes channel c at positions q, q+4, ... (25 of the 100), f32 FMA in (kh, kw) order; group statistics in two
// passes over registers; the normalised 10 x 10 x 64 map goes through LDS to the 5 x 5 max-pool.
// Replaces im2col + GEMM + GroupNorm + max-pool launches (and their 26 MB of intermediates per 1024 samples).
template <int PREC, int N>
__global__ void __launch_bounds__(256) encoder_stem_kernel(const float* __restrict__ lm /*[B][N][N]*/,
                                                           const float* __restrict__ W /*[49][64]: tap-major, coalesced per lane*/,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           void* __restrict__ out /*[B][PH*PH][64]*/, float eps, long long plane,
                                                           int* __restrict__ sat) {
  // N = 20 (car): 26 x 26 padded map, 10 x 10 conv outputs, 5 x 5 after the pool;  N = 16 (ant): 22, 8 x 8, 4 x 4
  constexpr int PD = N + 6, OH = N / 2, NP = OH * OH, J = NP / 4, PH = (OH - 1) / 2 + 1;
  __shared__ float s_map[PD * PD];
  __shared__ float s_act[NP * 64];
  __shared__ float s_red[2][4][4];                    // [pass][position quarter][group]
  float satm = 0.0f;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int c = tid & 63, q = tid >> 6, g = c >> 4;
  for (int i = tid; i < PD * PD; i += 256) {
    const int r = i / PD - 3, cc = i % PD - 3;
    s_map[i] = (r >= 0 && r < N && cc >= 0 && cc < N) ? lm[(size_t)b * (N * N) + r * N + cc] : 0.0f;
  }
  float w[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) w[k] = W[k * 64 + c];
  __syncthreads();
  float v[J];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int p = q + 4 * j, oh = p / OH, ow = p - oh * OH;
    const float* m0 = s_map + (oh * 2) * PD + ow * 2;
    float a = 0.f;
#pragma unroll
    for (int kh = 0; kh < 7; ++kh)
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) a = fmaf(w[kh * 7 + kw], m0[kh * PD + kw], a);
    v[j] = a;
    sum += a;
  }
  // the 16 channels of a group are 16 adjacent lanes; the 4 position quarters are the 4 waves
  sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
  if ((c & 15) == 0) s_red[0][q][g] = sum;
  __syncthreads();
  constexpr float inv_n = 1.0f / (float)(NP * 16);
  const float mean = ((s_red[0][0][g] + s_red[0][1][g]) + (s_red[0][2][g] + s_red[0][3][g])) * inv_n;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) { const float d = v[j] - mean; sq = fmaf(d, d, sq); }
  sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4); sq += __shfl_xor(sq, 8);
  if ((c & 15) == 0) s_red[1][q][g] = sq;
  __syncthreads();
  const float var = ((s_red[1][0][g] + s_red[1][1][g]) + (s_red[1][2][g] + s_red[1][3][g])) * inv_n;
  const float rstd = rsqrtf(var + eps);
  const float ga = gamma[c] * rstd, be = beta[c] - mean * ga;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    float y = fmaf(v[j], ga, be);
    y = y > 0.f ? y : 0.f;
    if constexpr (PREC == ST_BF16) y = bf2f(f2bf(y));      // the activation is stored as bf16 before the pool in the layered path
    if constexpr (PREC == ST_F16) {                        // (the split formats keep the f32 value: hi + lo carries it)
      sat_see(satm, y);                                    // the range guard looks HERE: f2h clamps, the pool sees no more than 65504
      y = h2f(f2h(y));
    }
    s_act[(q + 4 * j) * 64 + c] = y;
  }
  __syncthreads();
  for (int o = tid; o < PH * PH * 64; o += 256) {
    const int oc = o & 63, op = o >> 6, oh = op / PH, ow = op - oh * PH;
    float best = -__builtin_huge_valf();
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh * 2 + kh - 1, iw = ow * 2 + kw - 1;
        if (ih >= 0 && ih < OH && iw >= 0 && iw < OH) best = fmaxf(best, s_act[(ih * OH + iw) * 64 + oc]);
      }
    store_elem<PREC>(out, (long long)b * (PH * PH * 64) + o, best, plane, satm);
  }
  if constexpr ((PREC & 3) == ST_F16) sat_flush(sat, satm);
}
void launch_encoder_stem(const float* lm, int n, const float* W, const float* gamma, const float* beta, void* out, int B, float eps,
                         int fmt, long long plane, hipStream_t s, int* sat) {
  if (n != 20 && n != 16) throw std::runtime_error("encoder stem: local map must be 20 x 20 or 16 x 16");
#define CALL(F)                                                                                                                    \
  do {                                                                                                                             \
    if (n == 20) DN_LAUNCH((encoder_stem_kernel<F, 20>), dim3(B), dim3(256), 0, s, lm, W, gamma, beta, out, eps, plane, sat);  \
    else DN_LAUNCH((encoder_stem_kernel<F, 16>), dim3(B), dim3(256), 0, s, lm, W, gamma, beta, out, eps, plane, sat);          \
  } while (0)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

template <int PREC>
__global__ void prep_sample_kernel(const float* __restrict__ x, void* __restrict__ A0, int B, int Bp, int P, int D, long long plane,
                                   int* __restrict__ sat) {
  const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (long long)Bp * P) return;
  const int b = (int)(row / P), l = (int)(row - (long long)b * P);
  float v = 0.f;
  // rows B .. Bp-1 pad the batch to whole work units: zeros, not what an earlier call left in x (the guard would see it)
  if (b < B && lane < 3 * D) {
    const int t = lane / D, d = lane - t * D;
    const int ls = l + t - 1;
    if (ls >= 0 && ls < P) v = x[((long long)b * P + ls) * D + d];
  }
  float satm = 0.0f;
  store_elem<PREC>(A0, row * 64 + lane, v, plane, satm);
  if constexpr ((PREC & 3) == ST_F16) sat_flush(sat, satm);
}
void launch_prep_sample(const float* x, void* A0, int B, int Bp, int P, int D, int fmt, long long plane, hipStream_t s, int* sat) {
  long long rows = (long long)Bp * P;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define CALL(F) DN_LAUNCH(prep_sample_kernel<F>, grid, block, 0, s, x, A0, B, Bp, P, D, plane, sat)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

// Time embedding of one flow step: sinusoidal(256) -> Linear(256,1024) -> Mish -> Linear(1024,256)
// (positional_embedding.py:10-17, conditional_unet1d.py:180-185).  Batch-invariant, f32.
__global__ void __launch_bounds__(1024) time_embed_kernel(float t, const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ W2, const float* __restrict__ b2,
                                                          float* __restrict__ out /*[256]*/) {
  __shared__ float emb[256];
  __shared__ float hid[1024];
  const int tid = threadIdx.x;
  if (tid < 256) {
    const int half = 128;
    const float wlog = logf(10000.0f) / (float)(half - 1);
    const int k = tid & 127;
    const float f = expf((float)k * -wlog);
    const float a = t * f;
    emb[tid] = (tid < 128) ? sinf(a) : cosf(a);
  }
  __syncthreads();
  {
    float s = b1[tid];
    const float* wr = W1 + (long long)tid * 256;
    for (int k = 0; k < 256; ++k) s += wr[k] * emb[k];
    hid[tid] = mish_f<1>(s);
  }
  __syncthreads();
  if (tid < 256) {
    float s = b2[tid];
    const float* wr = W2 + (long long)tid * 1024;
    for (int k = 0; k < 1024; ++k) s += wr[k] * hid[k];
    out[tid] = s;
  }
}
void launch_time_embed(float t, const float* W1, const float* b1, const float* W2, const float* b2, float* out,
                       hipStream_t s) {
  DN_LAUNCH(time_embed_kernel, dim3(1), dim3(1024), 0, s, t, W1, b1, W2, b2, out);
}

// FiLM input: Mish(cat(time_emb 256, map_emb E, obs_cond G)) zero-padded to Kpad columns
// (conditional_unet1d.py:59-64 cond_encoder = Mish -> Linear, :293 global_feature).
template <int PREC>
__global__ void prep_cond_kernel(const float* __restrict__ temb, const float* __restrict__ map_emb, int E, int E_ld,
                                 const float* __restrict__ cond, int G, void* __restrict__ out, int B, int Kpad, long long plane,
                                 int* __restrict__ sat) {
  const int b = blockIdx.x;
  float satm = 0.0f;
  for (int k = threadIdx.x; k < Kpad; k += blockDim.x) {
    float v = 0.f;
    bool live = true;
    if (b >= B) live = false;          // blocks B .. Bp-1 pad the batch to whole work units: zeros, not an earlier call's rows
    else if (k < 256) v = temb[k];
    else if (k < 256 + E) v = map_emb[(long long)b * E_ld + (k - 256)];
    else if (k < 256 + E + G) v = cond[(long long)b * G + (k - 256 - E)];
    else live = false;
    store_elem<PREC>(out, (long long)b * Kpad + k, live ? MISH_OF(PREC)(v) : 0.f, plane, satm);
  }
  if constexpr ((PREC & 3) == ST_F16) sat_flush(sat, satm);
}
void launch_prep_cond(const float* temb, const float* map_emb, int E, int E_ld, const float* cond, int G, void* out, int B,
                      int Bp, int Kpad, int fmt, long long plane, hipStream_t s, int* sat) {
#define CALL(F) DN_LAUNCH(prep_cond_kernel<F>, dim3(Bp), dim3(256), 0, s, temb, map_emb, E, E_ld, cond, G, out, B, Kpad, plane, sat)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

// Final Conv1d(C -> D, 1) + flow Euler step + un-normalise (conditional_unet1d.py:253-256,
// policies/fm_policy.py:193,201-203).  One wave per position; Y is the padded channels-last
// output of the last Conv1dBlock.
struct ActNormArg { double mu[8], sg[8]; };
template <int PREC, int D>
__global__ void __launch_bounds__(256) final_proj_flow_kernel(const void* __restrict__ Y, int C, int Lp, long long plane,
                                                              const float* __restrict__ W /*[D][C]*/,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ x /*[B][P][D] in/out*/, FlowStep fs,
                                                              ActNormArg nm, double* __restrict__ actions, int B, int P) {
  const long long pos = blockIdx.x * 4LL + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pos >= (long long)B * P) return;
  const int b = (int)(pos / P), l = (int)(pos - (long long)b * P);
  const long long row = (long long)b * Lp + l + 1;
  float s[D];
#pragma unroll
  for (int d = 0; d < D; ++d) s[d] = 0.f;
  // a lane takes 8 consecutive channels per pass (16-B loads of 16-bit rows; C is a multiple of 8)
  for (int c = lane * 8; c < C; c += 512) {
    float y[8];
    if constexpr ((PREC & 3) == ST_F32) {
      const f32x4_t y0 = *(const f32x4_t*)((const float*)Y + row * C + c), y1 = *(const f32x4_t*)((const float*)Y + row * C + c + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { y[j] = y0[j]; y[4 + j] = y1[j]; }
    } else {
      constexpr int ET = (PREC & 3) == ST_F16 ? 1 : 0;
      const short8_t yv = *(const short8_t*)((const unsigned short*)Y + row * C + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = e2f<ET>((unsigned short)yv[j]);
      if constexpr ((PREC & 4) != 0) {
        const short8_t yl = *(const short8_t*)((const unsigned short*)((const char*)Y + plane) + row * C + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] += e2f<ET>((unsigned short)yl[j]);
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const f32x4_t w0 = *(const f32x4_t*)(W + (long long)d * C + c), w1 = *(const f32x4_t*)(W + (long long)d * C + c + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[d] = fmaf(y[j], w0[j], s[d]); }
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[d] = fmaf(y[4 + j], w1[j], s[d]); }
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s[d] += __shfl_xor(s[d], m);
  }
  if (lane < D) {
    float sv = s[0];
    double sg = nm.sg[0], mu = nm.mu[0];
#pragma unroll
    for (int d = 1; d < D; ++d) if (lane == d) { sv = s[d]; sg = nm.sg[d]; mu = nm.mu[d]; }
    const float v = sv + bias[lane];
    const long long xi = pos * D + lane;
    float xn;
    if (fs.mode == 0) {
      xn = x[xi] + v * fs.dt;                                 // naction + vel_pred * dt[k]
    } else if (fs.mode == 1) {
      xn = v;                                                 // raw: the network output itself
    } else {                                                  // DDPM step, float32 as the scheduler's tensors
      const float xc = x[xi];
      float x0 = (xc - fs.sb * v) / fs.sa;
      x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      xn = fs.c0 * x0 + fs.c1 * xc;
      if (fs.sigma != 0.0f) {
        const long long zr = fs.z_idx ? (long long)fs.z_idx[b] : (long long)fs.z_row0 + b;
        xn += fs.sigma * fs.z[zr * fs.z_row + (long long)l * D + lane];
      }
    }
    x[xi] = xn;
    if (actions != nullptr) actions[xi] = (double)xn * sg + mu;     // float32 * float64 -> float64 (:203)
  }
}
// act_norm = [mu[0..D), sigma[0..D)] (host)
void launch_final_proj_flow(const void* Y, int C, int Lp, long long plane, const float* W, const float* bias, int D, float* x,
                            FlowStep fs, const double* act_norm, double* actions, int B, int P, int fmt, hipStream_t s) {
  long long pos = (long long)B * P;
  dim3 grid((unsigned)((pos + 3) / 4)), block(256);
  ActNormArg nm{};
  for (int d = 0; d < D && d < 8; ++d) { nm.mu[d] = act_norm[d]; nm.sg[d] = act_norm[D + d]; }
#define CALLD(F, DD) DN_LAUNCH((final_proj_flow_kernel<F, DD>), grid, block, 0, s, Y, C, Lp, plane, W, bias, x, fs, nm, actions, B, P)
#define CALL(F) do { if (D == 2) CALLD(F, 2); else if (D == 8) CALLD(F, 8); else throw std::runtime_error("final projection: action_dim must be 2 or 8"); } while (0)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
#undef CALLD
}

// ------------------------------------------------------------------------------- encoder helpers
// GroupNorm (C/16 groups, local_map_encoder.py:63-76) on the f32 GEMM output [B][HW][C] (sum of the split-K
// slabs), optional residual add and ReLU (torchvision BasicBlock), writes the activation type.
// One 256-thread workgroup per sample: a thread owns 4 consecutive channels (16-B loads) of one position per
// pass, T = C/4 threads span a position, 256/T positions per pass, <= GN2D_MAXP passes kept in registers;
// a group is 4 adjacent threads x all positions: shuffle over the 4 threads, then 64 LDS partials
// (positions-per-pass x groups) summed by every thread.  Mean first, then centred squares (two passes over
// registers), as torch's GroupNorm.
#define GN2D_MAXP 7
template <int PREC>
__global__ void __launch_bounds__(256) gn2d_kernel(const float* __restrict__ in, int nslab, long long slab_stride,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const void* __restrict__ res, int relu, void* __restrict__ out, int HW,
                                                   int C, float eps, long long res_plane, long long out_plane, int* __restrict__ sat) {
  float satm = 0.0f;
  __shared__ float red[2][64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = C >> 2, PP = 256 / T, G = C >> 4;
  const int tpos = tid / T, tc = tid - tpos * T, grp = tc >> 2;
  const long long base = (long long)b * HW * C + 4 * tc;
  f32x4_t v[GN2D_MAXP];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < GN2D_MAXP; ++k) {
    const int pos = k * PP + tpos;
    f32x4_t x = {0.f, 0.f, 0.f, 0.f};
    if (pos < HW) {
      const float* src = in + base + (long long)pos * C;
      for (int sl = 0; sl < nslab; ++sl) {
        const f32x4_t t = *(const f32x4_t*)(src + sl * slab_stride);
        x += t;
      }
      s += (x[0] + x[1]) + (x[2] + x[3]);
    }
    v[k] = x;
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if ((tc & 3) == 0) red[0][tpos * G + grp] = s;
  __syncthreads();
  float tot = 0.f;
  for (int q = 0; q < PP; ++q) tot += red[0][q * G + grp];
  const float inv_n = 1.0f / (float)(HW * 16);
  const float mean = tot * inv_n;
  float q2 = 0.f;
#pragma unroll
  for (int k = 0; k < GN2D_MAXP; ++k) {
    if (k * PP + tpos < HW) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[k][j] - mean; q2 = fmaf(d, d, q2); }
    }
  }
  q2 += __shfl_xor(q2, 1);
  q2 += __shfl_xor(q2, 2);
  if ((tc & 3) == 0) red[1][tpos * G + grp] = q2;
  __syncthreads();
  float var = 0.f;
  for (int q = 0; q < PP; ++q) var += red[1][q * G + grp];
  const float rstd = rsqrtf(var * inv_n + eps);
  const f32x4_t ga = *(const f32x4_t*)(gamma + 4 * tc), be = *(const f32x4_t*)(beta + 4 * tc);
#pragma unroll
  for (int k = 0; k < GN2D_MAXP; ++k) {
    const int pos = k * PP + tpos;
    if (pos >= HW) continue;
    const long long idx = base + (long long)pos * C;
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = (v[k][j] - mean) * rstd * ga[j] + be[j];
    constexpr int ET = (PREC & 3) == ST_F16 ? 1 : 0;
    if (res != nullptr) {
      if constexpr ((PREC & 3) == ST_F32) {
        const f32x4_t r = *(const f32x4_t*)((const float*)res + idx);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] += r[j];
      } else {
        const short4_t r = *(const short4_t*)((const unsigned short*)res + idx);
        if constexpr ((PREC & 4) != 0) {
          const short4_t rl = *(const short4_t*)((const unsigned short*)((const char*)res + res_plane) + idx);
#pragma unroll
          for (int j = 0; j < 4; ++j) y[j] += e2f<ET>((unsigned short)r[j]) + e2f<ET>((unsigned short)rl[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) y[j] += e2f<ET>((unsigned short)r[j]);
        }
      }
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = y[j] > 0.f ? y[j] : 0.f;
    }
    if constexpr ((PREC & 3) == ST_F32) {
      const f32x4_t o = {y[0], y[1], y[2], y[3]};
      *(f32x4_t*)((float*)out + idx) = o;
    } else {
      short4_t o;
      if constexpr (ET == 1) { sat_see2(satm, y[0], y[1]); sat_see2(satm, y[2], y[3]); }
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (short)f2e<ET>(y[j]);
      *(short4_t*)((unsigned short*)out + idx) = o;
      if constexpr ((PREC & 4) != 0) {
        short4_t o2;
#pragma unroll
        for (int j = 0; j < 4; ++j) o2[j] = (short)f2e<ET>(y[j] - e2f<ET>((unsigned short)o[j]));
        *(short4_t*)((unsigned short*)((char*)out + out_plane) + idx) = o2;
      }
    }
  }
  if constexpr ((PREC & 3) == ST_F16) sat_flush(sat, satm);
}
void launch_gn2d(const float* in, int nslab, long long slab_stride, const float* gamma, const float* beta, const void* res,
                 int relu, void* out, int B, int HW, int C, float eps, int fmt, long long res_plane, long long out_plane,
                 hipStream_t s, int* sat) {
  // host-side shape contract of the kernel (ResNet-18 stages on maps up to 10 x 10)
  if (C < 64 || C > 1024 || (C & (C - 1)) != 0 || (HW + 256 / (C >> 2) - 1) / (256 / (C >> 2)) > GN2D_MAXP)
    throw std::runtime_error("encoder GroupNorm: unsupported map shape");
  dim3 grid((unsigned)B), block(256);
#define CALL(F) DN_LAUNCH(gn2d_kernel<F>, grid, block, 0, s, in, nslab, slab_stride, gamma, beta, res, relu, out, HW, C, eps, \
                                   res_plane, out_plane, sat)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

// AdaptiveAvgPool2d(1) on NHWC -> [B][C].
template <int PREC>
__global__ void avgpool2d_kernel(const void* __restrict__ in, void* __restrict__ out, int B, int HW, int C, long long in_plane,
                                 long long out_plane) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)B * C) return;
  const int c = (int)(idx % C), b = (int)(idx / C);
  float s = 0.f;
  for (int q = 0; q < HW; ++q) s += load_elem<PREC>(in, ((long long)b * HW + q) * C + c, in_plane);
  store_elem<PREC>(out, idx, s / (float)HW, out_plane);
}
void launch_avgpool2d(const void* in, void* out, int B, int HW, int C, int fmt, long long in_plane, long long out_plane,
                      hipStream_t s) {
  long long total = (long long)B * C;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define CALL(F) DN_LAUNCH(avgpool2d_kernel<F>, grid, block, 0, s, in, out, B, HW, C, in_plane, out_plane)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}

// debug / test support: padded channels-last activation -> f32 [B][L][C]
template <int PREC>
__global__ void unpack_act_kernel(const void* __restrict__ in, int ld, int coff, int Lp, int roff, float* __restrict__ out,
                                  int B, int L, int C, long long plane) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= (long long)B * L * C) return;
  const int c = (int)(idx % C);
  const int l = (int)((idx / C) % L), b = (int)(idx / ((long long)C * L));
  out[idx] = load_elem<PREC>(in, ((long long)b * Lp + l + roff) * ld + coff + c, plane);
}
void launch_unpack_act(const void* in, int ld, int coff, int Lp, int roff, float* out, int B, int L, int C, int fmt,
                       long long plane, hipStream_t s) {
  long long total = (long long)B * L * C;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
#define CALL(F) DN_LAUNCH(unpack_act_kernel<F>, grid, block, 0, s, in, ld, coff, Lp, roff, out, B, L, C, plane)
  DISPATCH_FMT(fmt, CALL)
#undef CALL
}
