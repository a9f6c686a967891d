// The reference's five small local-map encoders (local_map_encoder.py:137-218) in f32: identity, mlp, max, grid, cnn.
//
// One launch writes map_emb[b, 0:E] for a batch of (n x n) f32 local maps.  Plain FMA arithmetic, no MFMA: the largest of
// them (mlp) is 186 k MAC per sample against 2.6 G for the car U-Net.  Every output element is one fixed chain
//     acc = bias;  acc = fma(x_k, w_k, acc)  for k = 0, 1, 2, ...
// (conv: k runs over (ci, kh, kw) in that order), formed by one thread; which tile, block or lane a sample lands in decides
// only WHERE the chain is evaluated, never its order -- a sample's embedding does not depend on the batch.
//
//   identity  flatten: a copy
//   max       AdaptiveMaxPool2d(k): cell i covers [floor(i n / k), ceil((i + 1) n / k))
//   grid      conv3x3(1->3) ReLU conv3x3(3->6) ReLU conv3x3(6->4), AdaptiveMaxPool2d(6), flatten (C, H, W)
//   cnn       conv3x3(1->2) Mish conv3x3(2->4) Mish conv3x3(4->4) Mish conv3x3(4->4) Mish, flatten (C, H, W)
//   mlp       Linear(n^2, 128) ReLU Linear(128, 256) ReLU Linear(256, E)
//
// grid / cnn: one work-group per sample; the whole parameter set (< 2 KB) and the sample's planes (two ping-pong buffers)
// live in LDS.  mlp: the weights (0.75 MB at n = 20) do not fit in LDS, so a work-group owns a tile of MLP_TS samples and
// walks the weights once per tile; the weights are stored transposed ([k][neuron]) so that the lanes of a wave -- consecutive
// neurons -- load consecutive floats, and the tile's activations are LDS broadcasts.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "denoise.h"

#define ENC_LAUNCH(...) do { if (!denoise_dry_run()) hipLaunchKernelGGL(__VA_ARGS__); } while (0)

namespace {

constexpr int MLP_TS = 8;          // samples per work-group of the mlp kernel
constexpr int MLP_H1 = 128, MLP_H2 = 256;
constexpr int MLP_MAX_IN = 1024;   // n <= 32
constexpr int CONV_MAX_N = 32;

__device__ __forceinline__ float enc_mish(float x) {
  // x * tanh(softplus(x)) = x * w / (w + 2), w = e^x (e^x + 2); softplus threshold as torch
  if (x > 20.0f) return x;
  const float n = expf(x);
  const float w = n * (n + 2.0f);
  return x * (w / (w + 2.0f));
}

__global__ void __launch_bounds__(256) enc_identity_kernel(const float* __restrict__ lm, float* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = lm[i];
}

__global__ void __launch_bounds__(256) enc_max_kernel(const float* __restrict__ lm, float* __restrict__ out, int B, int n, int k) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int E = k * k;
  if (i >= (long long)B * E) return;
  const int b = (int)(i / E), c = (int)(i - (long long)b * E);
  const int oi = c / k, oj = c - oi * k;
  const int h0 = (oi * n) / k, h1 = ((oi + 1) * n + k - 1) / k;
  const int w0 = (oj * n) / k, w1 = ((oj + 1) * n + k - 1) / k;
  const float* m = lm + (long long)b * n * n;
  float v = m[h0 * n + w0];
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) v = fmaxf(v, m[h * n + w]);
  out[i] = v;
}

// valid 3 x 3 convolution of CIN planes (H x H, in LDS) to COUT planes ((H - 2) x (H - 2)); ACT 0 none, 1 ReLU, 2 Mish.
// `dst` is LDS or (last layer of cnn) global memory.  wgt: [COUT][CIN][3][3] then bias[COUT], in LDS.
template <int CIN, int COUT, int ACT>
__device__ __forceinline__ void conv3x3_valid(const float* __restrict__ src, int H, float* __restrict__ dst, const float* __restrict__ wgt,
                                              const float* __restrict__ bias) {
  const int O = H - 2, OO = O * O, HH = H * H;
  for (int o = threadIdx.x; o < COUT * OO; o += blockDim.x) {
    const int co = o / OO, r = o - co * OO, oy = r / O, ox = r - oy * O;
    float acc = bias[co];
    const float* w = wgt + co * CIN * 9;
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      const float* s = src + ci * HH + oy * H + ox;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) acc = fmaf(s[kh * H + kw], w[ci * 9 + kh * 3 + kw], acc);
    }
    if (ACT == 1) acc = fmaxf(acc, 0.0f);
    if (ACT == 2) acc = enc_mish(acc);
    dst[o] = acc;
  }
}

struct ConvEncArgs {
  const float* lm;
  float* out;
  int n, E;
  const float* w[4];
  const float* b[4];
};

// KIND 0 grid, 1 cnn.  Dynamic LDS: params | buffer A | buffer B (sizes from the launcher).
template <int KIND>
__global__ void __launch_bounds__(256) enc_conv_kernel(ConvEncArgs a, int bufA) {
  extern __shared__ float lds[];
  constexpr int NL = KIND == 0 ? 3 : 4;
  constexpr int ci[4] = {1, KIND == 0 ? 3 : 2, KIND == 0 ? 6 : 4, 4};
  constexpr int co[4] = {KIND == 0 ? 3 : 2, KIND == 0 ? 6 : 4, 4, 4};
  constexpr int PAR = 512;                           // >= 418 (grid) / 392 (cnn) parameters
  float* par = lds;
  float* A = lds + PAR;
  float* Bf = A + bufA;
  const int n = a.n, b = blockIdx.x;
  int woff[4], boff[4], off = 0;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    woff[l] = off; off += co[l] * ci[l] * 9;
    boff[l] = off; off += co[l];
    for (int i = threadIdx.x; i < co[l] * ci[l] * 9; i += blockDim.x) par[woff[l] + i] = a.w[l][i];
    for (int i = threadIdx.x; i < co[l]; i += blockDim.x) par[boff[l] + i] = a.b[l][i];
  }
  const float* m = a.lm + (long long)b * n * n;
  for (int i = threadIdx.x; i < n * n; i += blockDim.x) A[i] = m[i];
  __syncthreads();
  float* out = a.out + (long long)b * a.E;
  if constexpr (KIND == 0) {
    conv3x3_valid<1, 3, 1>(A, n, Bf, par + woff[0], par + boff[0]);
    __syncthreads();
    conv3x3_valid<3, 6, 1>(Bf, n - 2, A, par + woff[1], par + boff[1]);
    __syncthreads();
    conv3x3_valid<6, 4, 0>(A, n - 4, Bf, par + woff[2], par + boff[2]);
    __syncthreads();
    const int h = n - 6;                             // AdaptiveMaxPool2d((6, 6)) over 4 planes of h x h
    for (int o = threadIdx.x; o < 4 * 36; o += blockDim.x) {
      const int c = o / 36, r = o - c * 36, oi = r / 6, oj = r - oi * 6;
      const int h0 = (oi * h) / 6, h1 = ((oi + 1) * h + 5) / 6, w0 = (oj * h) / 6, w1 = ((oj + 1) * h + 5) / 6;
      const float* p = Bf + c * h * h;
      float v = p[h0 * h + w0];
      for (int y = h0; y < h1; ++y)
        for (int x = w0; x < w1; ++x) v = fmaxf(v, p[y * h + x]);
      out[o] = v;
    }
  } else {
    conv3x3_valid<1, 2, 2>(A, n, Bf, par + woff[0], par + boff[0]);
    __syncthreads();
    conv3x3_valid<2, 4, 2>(Bf, n - 2, A, par + woff[1], par + boff[1]);
    __syncthreads();
    conv3x3_valid<4, 4, 2>(A, n - 4, Bf, par + woff[2], par + boff[2]);
    __syncthreads();
    conv3x3_valid<4, 4, 2>(Bf, n - 6, out, par + woff[3], par + boff[3]);      // (C, H, W) order is the flatten order
  }
}

struct MlpEncArgs {
  const float* lm;
  float* out;
  int B, K0, E;             // K0 = n * n inputs, E outputs
  const float *w1t, *b1;    // [K0][128]
  const float *w2t, *b2;    // [128][256]
  const float *w3t, *b3;    // [256][E]
};

// One Linear layer for the tile: thread -> neuron j, NS samples of the tile starting at s0.  x: LDS [MLP_TS][ldx].
template <int NS, bool RELU>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ x, int ldx, int s0, int K, const float* __restrict__ wt, int N, int j,
                                          float bias, float* __restrict__ y, long long ldy, int nvalid) {
  float acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = bias;
  const float* wp = wt + j;
  int k = 0;
  for (; k + 4 <= K; k += 4) {
    float w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = wp[(long long)(k + u) * N];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s] = fmaf(x[(s0 + s) * ldx + k + u], w[u], acc[s]);
  }
  for (; k < K; ++k) {
    const float w = wp[(long long)k * N];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = fmaf(x[(s0 + s) * ldx + k], w, acc[s]);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (s0 + s < nvalid) y[(s0 + s) * ldy + j] = RELU ? fmaxf(acc[s], 0.0f) : acc[s];
}

__global__ void __launch_bounds__(256) enc_mlp_kernel(MlpEncArgs a) {
  extern __shared__ float lds[];
  float* x0 = lds;                                   // [MLP_TS][K0]
  float* h1 = x0 + MLP_TS * a.K0;                    // [MLP_TS][128]
  float* h2 = h1 + MLP_TS * MLP_H1;                  // [MLP_TS][256]
  const int b0 = blockIdx.x * MLP_TS;
  const int nb = min(MLP_TS, a.B - b0);
  const int tid = threadIdx.x;
  for (int i = tid; i < MLP_TS * a.K0; i += 256) x0[i] = i < nb * a.K0 ? a.lm[(long long)b0 * a.K0 + i] : 0.0f;
  __syncthreads();
  {                                                  // 128 neurons x 8 samples: a thread takes one neuron and half the tile
    const int j = tid & (MLP_H1 - 1), s0 = (tid >> 7) * (MLP_TS / 2);
    mlp_layer<MLP_TS / 2, true>(x0, a.K0, s0, a.K0, a.w1t, MLP_H1, j, a.b1[j], h1, MLP_H1, MLP_TS);
  }
  __syncthreads();
  mlp_layer<MLP_TS, true>(h1, MLP_H1, 0, MLP_H1, a.w2t, MLP_H2, tid, a.b2[tid], h2, MLP_H2, MLP_TS);
  __syncthreads();
  for (int j = tid; j < a.E; j += 256)
    mlp_layer<MLP_TS, false>(h2, MLP_H2, 0, MLP_H2, a.w3t, a.E, j, a.b3[j], a.out + (long long)b0 * a.E, a.E, nb);
}

}  // namespace

const char* small_encoder_name(int kind) {
  static const char* names[] = {"resnet", "identity", "mlp", "max", "grid", "cnn"};
  return kind >= 0 && kind < 6 ? names[kind] : "?";
}

int small_encoder_width(int kind, int n, int k) {
  switch (kind) {
    case ENC_IDENTITY: case ENC_MLP: return n * n;
    case ENC_MAX: return k * k;
    case ENC_GRID: return 144;
    case ENC_CNN: return n > 8 ? 4 * (n - 8) * (n - 8) : 0;
    default: return 0;
  }
}

void launch_small_encoder(const SmallEncoderParams& p, hipStream_t s) {
  const int n = p.n;
  if (p.B <= 0) return;
  if (n < 1 || p.E != small_encoder_width(p.kind, n, p.k) || p.E < 1)
    throw std::runtime_error(std::string("encoder '") + small_encoder_name(p.kind) + "': embedding width " + std::to_string(p.E) +
                             " does not fit a " + std::to_string(n) + " x " + std::to_string(n) + " map");
  switch (p.kind) {
    case ENC_IDENTITY: {
      const long long total = (long long)p.B * n * n;
      ENC_LAUNCH(enc_identity_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p.lm, p.out, total);
      return;
    }
    case ENC_MAX: {
      const long long total = (long long)p.B * p.E;
      ENC_LAUNCH(enc_max_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p.lm, p.out, p.B, n, p.k);
      return;
    }
    case ENC_GRID: case ENC_CNN: {
      const bool grid = p.kind == ENC_GRID;
      const int nmin = grid ? 7 : 9;
      if (n < nmin || n > CONV_MAX_N)
        throw std::runtime_error(std::string("encoder '") + small_encoder_name(p.kind) + "': local_map_size " + std::to_string(n) +
                                 " is outside " + std::to_string(nmin) + ".." + std::to_string(CONV_MAX_N));
      // ping-pong planes: A holds the map and layer 2's output, B layer 1's and layer 3's
      const int c1 = grid ? 3 : 2, c2 = grid ? 6 : 4;
      const int bufA = std::max(n * n, c2 * (n - 4) * (n - 4));
      const int bufB = std::max(c1 * (n - 2) * (n - 2), 4 * (n - 6) * (n - 6));
      const size_t lds = (size_t)(512 + bufA + bufB) * sizeof(float);      // <= 40 KB at n = 32
      ConvEncArgs a{};
      a.lm = p.lm; a.out = p.out; a.n = n; a.E = p.E;
      for (int l = 0; l < 4; ++l) { a.w[l] = p.w[l]; a.b[l] = p.b[l]; }
      if (grid) ENC_LAUNCH(enc_conv_kernel<0>, dim3(p.B), dim3(256), lds, s, a, bufA);
      else ENC_LAUNCH(enc_conv_kernel<1>, dim3(p.B), dim3(256), lds, s, a, bufA);
      return;
    }
    case ENC_MLP: {
      if (n * n > MLP_MAX_IN)
        throw std::runtime_error("encoder 'mlp': local_map_size " + std::to_string(n) + " is beyond " + std::to_string(32));
      MlpEncArgs a{};
      a.lm = p.lm; a.out = p.out; a.B = p.B; a.K0 = n * n; a.E = p.E;
      a.w1t = p.w[0]; a.b1 = p.b[0]; a.w2t = p.w[1]; a.b2 = p.b[1]; a.w3t = p.w[2]; a.b3 = p.b[2];
      const size_t lds = (size_t)MLP_TS * (a.K0 + MLP_H1 + MLP_H2) * sizeof(float);   // 24.5 KB at n = 20, 44 KB at n = 32
      ENC_LAUNCH(enc_mlp_kernel, dim3((p.B + MLP_TS - 1) / MLP_TS), dim3(256), lds, s, a);
      return;
    }
    default:
      throw std::runtime_error("launch_small_encoder: unknown encoder kind " + std::to_string(p.kind));
  }
}
