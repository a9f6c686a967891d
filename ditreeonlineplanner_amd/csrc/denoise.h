// Internal interface between the denoiser's host orchestration and its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { MODE_BIAS = 0, MODE_GN_MISH = 1, MODE_GN_MISH_FILM = 2, MODE_GN_MISH_RES = 3 };

// Numeric format of an activation buffer / a GEMM: storage type | split << 2.
//   storage: bf16, f32, f16.  split (16-bit storage only): the buffer holds two planes, hi = rnd16(x) and
//   lo = rnd16(x - hi), `plane` bytes apart; a split GEMM forms hi*hi + hi*lo + lo*hi on the 16-bit MFMA pipeline.
enum { ST_BF16 = 0, ST_F32 = 1, ST_F16 = 2 };
static inline int fmt_make(int st, bool split) { return st | (split ? 4 : 0); }
static inline __host__ __device__ int fmt_st(int f) { return f & 3; }
static inline __host__ __device__ bool fmt_split(int f) { return (f & 4) != 0; }
static inline int fmt_es(int f) { return fmt_st(f) == ST_F32 ? 4 : 2; }

// One implicit-GEMM launch (see conv_tiles.hip).  All counts are in elements of the
// activation type (bf16 or f32); pointers are device pointers.
struct ConvGemmParams {
  const void* A;      // activations, channels contiguous
  int lda;            // elements per A row
  int in_Lp;          // A rows per sample (L_in + 2 for padded conv inputs)
  int in_stride;      // row(b, l, tap) = b*in_Lp + l*in_stride + tap + in_off
  int in_off;
  int taps, Cin;      // K = taps * Cin, Cin a multiple of 64
  const void* W;      // [ceil(N/256)*256][taps*Cin], row co = [tap][ci]
  void* Out;
  int ldc;            // elements per output row
  int out_Lp, out_stride, out_off;   // out row(b, l) = b*out_Lp + l*out_stride + out_off
  int out_coff;       // channel offset inside the output row (concat halves)
  int L;              // positions per sample in this GEMM; M = samples * L
  int M, N;
  const float* bias;  // [N] or null
  int mode;
  const float* gamma; // [N] GroupNorm affine
  const float* beta;
  int group_ch;       // channels per group (N / 8)
  float eps;
  const float* film;  // [samples][film_ld] f32: scale at film_off + c, bias at film_off + N + c
  int film_ld, film_off;
  const void* Res;    // residual, activation type
  int ldres, res_Lp, res_off;
  int out_f32;        // store f32 regardless of the activation type
  int xcd_strips;     // halo / gemm16 kernels: 1 = walk an XCD's tile range in strips of four tile columns (xcd_remap_strips)
  // implicit Conv2d on NHWC activations (c2d != 0): GEMM row m = (b, oh, ow); K = live taps x Cin
  // (Cin a multiple of 64: one tap spans Cin/64 K-steps); A is the input activation (B, H, W, Cin);
  // taps that fall outside the map read `zero` (>= 128 zero bytes).
  int c2d, c2_H, c2_W, c2_OW, c2_OHW, c2_stride, c2_pad;
  signed char c2_kh[12], c2_kw[12];
  const void* zero;
  // split formats: bytes from the hi plane to the lo plane of each operand (the weights: from an element's hi half to its lo
  // half, see w_row / w_step below); f16 weights are stored multiplied by a power of two (the range of f16 is narrow) and
  // `w_scale` = its reciprocal is applied to the accumulator
  long long a_plane, w_plane, out_plane, res_plane;
  float w_scale;
  // split-K (implicit Conv2d mode only): gridDim.y = splitk blocks share a tile, block y handles a
  // contiguous range of K-steps and writes its partial f32 tile to Out + y * slab_stride elements
  int splitk;
  long long slab_stride;
  // split-K of the halo kernel (latency mode, small batches): gridDim.y = splitk work-groups share a tile, each walks nv / splitk
  // channel chunks and dumps its f32 accumulators to sk_ws[(y * tiles + tile) * 65536]; the last one to arrive (sk_cnt[tile])
  // adds the slabs in split order -- one fixed order whoever arrives last -- and runs the epilogue
  float* sk_ws;
  int* sk_cnt;
  // f16 range guard: device flag word of this layer (set to 1 by any thread that stores a value beyond +-65504; null = off).
  // Only the f16 instantiations look at it.
  int* sat;
  // split weights, where element (row n, K index k = tap * Cin + ci) lives: n * w_row + (k >> 5) * w_step + (k & 31) * 2 bytes,
  // its lo half w_plane bytes further.  Chunk-interleaved (the default): a 32-channel chunk is one 128-byte unit [32 hi | 32 lo],
  // w_step = 128, w_plane = 64, w_row = 4 K.  Planar (DITREE_SPLIT_PLANAR=1): w_step = 64, w_plane = the plane distance,
  // w_row = 2 K.  The non-split formats do not read these.
  int w_row, w_step;
};

void denoise_set_dry_run(bool on);   // launchers check their contracts but enqueue nothing (plan validation at reserve time)
bool denoise_dry_run();
void launch_conv_gemm(const ConvGemmParams& p, int fmt, hipStream_t s);
bool conv2d_small_eligible(int fmt);                    // implicit Conv2d layers run on the 64 x 64-tile kernel
int conv_gemm_kind(const ConvGemmParams& p, int fmt);   // 0 halo kernel, 1 gemm16 / generic, 2 implicit Conv2d
bool conv_gemm_supported(const ConvGemmParams& p, int fmt);   // split formats: only shapes of the halo / gemm16 tiles
// (prep_sample / prep_cond: rows B .. Bp-1, the padding up to the batch granule, are written as zeros)
void launch_prep_sample(const float* x, void* A0, int B, int Bp, int P, int D, int fmt, long long plane, hipStream_t s, int* sat = nullptr);
void launch_time_embed(float t, const float* W1, const float* b1, const float* W2, const float* b2, float* out,
                       hipStream_t s);
void launch_prep_cond(const float* temb, const float* map_emb, int E, int E_ld, const float* cond, int G, void* out, int B,
                      int Bp, int Kpad, int fmt, long long plane, hipStream_t s, int* sat = nullptr);
// What the last projection does with the network output v of a sampler step:
//   FLOW  x += v * dt                     (policies/fm_policy.py:183-196)
//   RAW   x  = v                          (one raw network evaluation)
//   DDPM  x0 = clip((x - sb v) / sa, -1, 1); x = c0 x0 + c1 x + sigma z   (policies/fm_policy.py:164-182 with a DDPM scheduler:
//         epsilon prediction, clip_sample, fixed_small variance; z = the step's standard-normal noise, row r of it for dense row r
//         = z[(z_idx ? z_idx[r] : z_row0 + r) * z_row + (l * D + d)]; sigma == 0 at the last step)
struct FlowStep {
  int mode;                 // 0 FLOW, 1 RAW, 2 DDPM
  float dt;
  float sb, sa, c0, c1, sigma;
  const float* z;
  long long z_row;
  const int* z_idx;
  int z_row0;
};
void launch_final_proj_flow(const void* Y, int C, int Lp, long long plane, const float* W, const float* bias, int D, float* x,
                            FlowStep fs, const double* act_norm /*[mu[D], sigma[D]]*/, double* actions, int B, int P, int fmt,
                            hipStream_t s);
void launch_gn1d(void* x, int ld, int Lp, int row_off, int coff, int L, int C, const float* gamma, const float* beta, float eps,
                 int mode, const float* film, int film_ld, int film_off, const void* res, int ldres, int res_Lp, int res_off,
                 int B, int fmt, long long x_plane, long long res_plane, hipStream_t s, int* sat = nullptr);
void launch_encoder_stem(const float* lm, int n, const float* W, const float* gamma, const float* beta, void* out, int B, float eps,
                         int fmt, long long plane, hipStream_t s, int* sat = nullptr);
void launch_gn2d(const float* in, int nslab, long long slab_stride, const float* gamma, const float* beta, const void* res,
                 int relu, void* out, int B, int HW, int C, float eps, int fmt, long long res_plane, long long out_plane,
                 hipStream_t s, int* sat = nullptr);
void launch_avgpool2d(const void* in, void* out, int B, int HW, int C, int fmt, long long in_plane, long long out_plane,
                      hipStream_t s);
void launch_unpack_act(const void* in, int ld, int coff, int Lp, int roff, float* out, int B, int L, int C, int fmt,
                       long long plane, hipStream_t s);

// The reference's small local-map encoders (encoder_kernels.hip), f32 in every DITREE_PREC_*: one launch writes
// out[b, 0:E] (row stride E) for B maps of n x n.  Parameter pointers by kind:
//   identity, max   none (max: k x k cells, E = k * k)
//   mlp             w[0..2] = fc1..fc3 weights TRANSPOSED to [in][out], b[0..2] the biases; E = fc3's outputs
//   grid            w[0..2], b[0..2] = conv1..conv3 as stored ([Cout][Cin][3][3]); E = 144
//   cnn             w[0..3], b[0..3] = conv1..conv4 as stored; E = 4 (n - 8)^2
// A size the kernels do not cover throws std::runtime_error (also in dry-run mode: it surfaces at reserve time).
enum { ENC_RESNET = 0, ENC_IDENTITY = 1, ENC_MLP = 2, ENC_MAX = 3, ENC_GRID = 4, ENC_CNN = 5 };
struct SmallEncoderParams {
  int kind;
  const float* lm;
  float* out;
  int B, n, E, k;
  const float* w[4];
  const float* b[4];
};
const char* small_encoder_name(int kind);
int small_encoder_width(int kind, int n, int k);   // embedding width of a kind (0: none)
void launch_small_encoder(const SmallEncoderParams& p, hipStream_t s);
