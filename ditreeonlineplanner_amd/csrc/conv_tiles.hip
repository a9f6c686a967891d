// MFMA kernels of the DiTree denoiser (gfx950 / CDNA4).
//
// One implicit-GEMM kernel serves every dense layer of the reference network
// (model/diffusion/conditional_unet1d.py:41-142,268-347, conv1d_components.py:7-40,
//  local_map_encoder.py:112-122):
//      Out[(b,l), co] = sum_{tap, ci} X[b, l*stride + tap + off, ci] * W[co, tap, ci]
//  * activations are channels-last with one zero row on either side of every sample
//    ([B][L+2][C]), so the k = 3 taps of a Conv1d are three *overlapping row windows* of
//    the same buffer -- no im2col copy, the A operand is streamed straight from HBM/L2
//    into LDS with `global_load_lds` (16 B per lane) and per-lane source addresses;
//  * GEMM orientation: M = positions (B*L), N = output channels, K = taps*C_in;
//    256 x 256 x (128 bytes of K) tiles, 8 waves as 4(M) x 2(N), each wave 64 x 128 with
//    v_mfma_f32_32x32x16_bf16 / _f16 (PREC 0 / 2) or v_mfma_f32_32x32x2_f32 (PREC 1, parity path);
//  * LDS rows are 128 B; the 16-B slot index is XOR-swizzled on the *source* address and on the ds_read_b128 address:
//    with (row >> 1) & 7 in the kernels whose fragment rows start at multiples of 16 (conflict-free there), with row & 7 in
//    the halo kernels, whose fragment rows are shifted by the tap and by the halo rows of the samples in front (the
//    (row >> 1) swizzle cost them 17.6 % of their LDS cycles in bank conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE,
//    profiles/r02_bf16_pmc_sq.json; row & 7 is conflict-free for ANY row offset: a ds_read_b128 lane group then holds
//    16 distinct (row parity, slot) pairs);
//  * the weight rows of a tile are permuted in LDS so that lane r of a wave owns output
//    channels 4r..4r+3: the epilogue then stores 8 B (bf16) / 16 B (f32) per lane,
//    256 / 512 contiguous bytes per output row;
//  * epilogue fused in registers: bias, GroupNorm (two-pass statistics through LDS
//    atomics; a tile always holds whole (sample, group) sets), Mish, FiLM scale/bias or
//    residual add.
#include <type_traits>

#include "denoise_device.h"

// The one definition of the dry-run flag (DN_LAUNCH, denoise_device.h, reads it through denoise_dry_run()).
static thread_local bool g_dn_dry_run = false;
void denoise_set_dry_run(bool on) { g_dn_dry_run = on; }
bool denoise_dry_run() { return g_dn_dry_run; }

// ---- shared epilogue: bias, GroupNorm + Mish (+ FiLM | + residual), store ------------------------
// acc[mb][j][i] of lane (r5, h), wave (wm, wn) holds tile row wm*64 + mb*32 + (i&3) + 8*(i>>2) + 4*h,
// tile channel wn*128 + 4*r5 + j.  `smem` must be free for reuse (callers barrier first).
// PREC 0: bf16 storage, 1: f32 (parity instantiation, two-pass statistics, exact Mish), 2: f16 storage.
template <int PREC>
__device__ __forceinline__ void gemm_epilogue(const ConvGemmParams& p, f32x16_t (&acc)[2][4], char* smem, int tm, int tn,
                                              int tid, int lane, int r5, int h, int wm, int wn,
                                              long long out_extra_bytes = 0) {

  constexpr int ET = PREC == 2 ? 1 : 0;
  float satm = 0.0f;                                          // f16 range guard (sat_see2)
  const int c_l = wn * 128 + 4 * r5;                          // lane's 4 consecutive channels in the tile
  const int n0 = tn * 256 + c_l;
  const bool n_ok = n0 < p.N;
  float bias4[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && n_ok) {
    f32x4_t t = *(const f32x4_t*)(p.bias + n0);
#pragma unroll
    for (int j = 0; j < 4; ++j) bias4[j] = t[j];
  }
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if constexpr (PREC == 2) acc[mb][j][i] = fmaf(acc[mb][j][i], p.w_scale, bias4[j]);   // f16 weights are stored scaled
        else acc[mb][j][i] += bias4[j];
      }

  // 16-row blocks of this lane: blk = mb*2 + hf covers tile rows wm*64 + mb*32 + hf*16 .. +15
  int blk_b[4], blk_l[4];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const int m0 = tm * 256 + wm * 64 + (blk >> 1) * 32 + (blk & 1) * 16;
    const int b = m0 / p.L;
    blk_b[blk] = b;
    blk_l[blk] = m0 - b * p.L;
  }

  if (p.mode >= MODE_GN_MISH) {
    float* s_sum = (float*)smem;                              // [16 slots][4 groups]
    float* s_sq = s_sum + 64;
    if (tid < 128) s_sum[tid] = 0.0f;
    // per-channel / per-sample epilogue operands are requested before the statistics so that their
    // latency hides under the reductions
    const f32x4_t gam = *(const f32x4_t*)(p.gamma + n0);
    const f32x4_t bet = *(const f32x4_t*)(p.beta + n0);
    f32x4_t film_s[4], film_b[4];
    if (p.mode == MODE_GN_MISH_FILM) {
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        const float* fr = p.film + (long long)blk_b[blk] * p.film_ld + p.film_off + n0;
        film_s[blk] = *(const f32x4_t*)fr;
        film_b[blk] = *(const f32x4_t*)(fr + p.N);
      }
    }
    short4_t resv[2][8];
    auto fetch_res = [&](int blk, short4_t (&dst)[8]) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rofs = (i & 3) + 8 * (i >> 2) + 4 * h;
        const long long rrow = (long long)blk_b[blk] * p.res_Lp + blk_l[blk] + rofs + p.res_off;
        dst[i] = *(const short4_t*)((const char*)p.Res + (rrow * p.ldres + n0) * 2);
      }
    };
    const bool res_bf16 = (PREC != 1) && p.mode == MODE_GN_MISH_RES;
    if (res_bf16) fetch_res(0, resv[0]);
    __syncthreads();
    const int spt = 256 / p.L;                                // sample slots per tile
    const int gi = c_l / p.group_ch;                          // lane's group within the tile
    const bool wide = p.group_ch >= 128;
    int slot[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) slot[blk] = blk_b[blk] - tm * spt;
    const float inv_cnt = 1.0f / (float)(p.group_ch * p.L);
    // One lane per group adds a row block's partial into its sample's cell.  Where several waves feed a cell with more than
    // one add each (L >= 128: two or four wm waves; a 256-wide group at L = 32 / 64: both wn waves) the order the adds land
    // in would reach the bits, so those levels are `ordered` as in gemm_epilogue16: a wave adds its row blocks of a sample
    // in registers, writes a cell of its own, [wm][wn][group][sample of the wave (two at L = 32)], and the cells of a
    // sample are added in index order after the barrier.  Cells that no wave writes stay 0.
    const bool ordered = p.L >= 128 || (p.group_ch == 256 && p.L >= 32);
    const bool adder = lane == 0 || (!wide && lane == 16);
    const int ocell = ((wm * 2 + wn) * 4 + gi) * 2;
    auto put = [&](float* cell, float (&t)[4]) {               // t: the wave's four row-block partials (reduced over the lanes)
      if (ordered) {
        if (p.L >= 64) { t[0] = (t[0] + t[1]) + (t[2] + t[3]); t[2] = 0.0f; }
        else { t[0] += t[1]; t[2] += t[3]; }
        if (adder) { cell[ocell] = t[0]; cell[ocell + 1] = t[2]; }
      } else if (adder) {
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) atomicAdd(&cell[slot[blk] * 4 + gi], t[blk]);
      }
    };
    auto get = [&](const float* cell, float (&t)[4]) {
      if (!ordered) {
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) t[blk] = cell[slot[blk] * 4 + gi];
        return;
      }
#pragma unroll
      for (int blk = 0; blk < 4; blk += 2) {
        const int r0 = slot[blk] * p.L;                          // the sample's first row in the tile
        const int w0 = r0 >> 6, nw = p.L >= 64 ? p.L >> 6 : 1, sub = (r0 >> 5) & 1;
        float v = 0.0f;
        for (int w = w0; w < w0 + nw; ++w) {
          v += cell[((w * 2 + 0) * 4 + gi) * 2 + sub];
          v += cell[((w * 2 + 1) * 4 + gi) * 2 + sub];
        }
        t[blk] = v; t[blk + 1] = v;
      }
    };
    float mean[4], rstd[4];
    if constexpr (PREC != 1) {
      // one pass: sum and sum of squares (f32), var = E[x^2] - mean^2
      float ps[4], pq[4];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float v = acc[blk >> 1][j][(blk & 1) * 8 + i];
            s += v;
            q = fmaf(v, v, q);
          }
        s += __shfl_xor(s, 1); q += __shfl_xor(q, 1);
        s += __shfl_xor(s, 2); q += __shfl_xor(q, 2);
        s += __shfl_xor(s, 4); q += __shfl_xor(q, 4);
        s += __shfl_xor(s, 8); q += __shfl_xor(q, 8);
        s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
        if (wide) { s += __shfl_xor(s, 16); q += __shfl_xor(q, 16); }
        ps[blk] = s; pq[blk] = q;
      }
      put(s_sum, ps);
      put(s_sq, pq);
      __syncthreads();
      get(s_sum, ps);
      get(s_sq, pq);
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        mean[blk] = ps[blk] * inv_cnt;
        const float var = fmaxf(pq[blk] * inv_cnt - mean[blk] * mean[blk], 0.0f);
        rstd[blk] = rsqrtf(var + p.eps);
      }
    } else {
    // pass 1: sums
    {
      float ps[4];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 8; ++i) s += acc[blk >> 1][j][(blk & 1) * 8 + i];
        ps[blk] = s;
      }
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        float s = ps[blk];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 32);
        if (wide) s += __shfl_xor(s, 16);
        ps[blk] = s;
      }
      put(s_sum, ps);
      __syncthreads();
      get(s_sum, ps);
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) mean[blk] = ps[blk] * inv_cnt;
    }
    // pass 2: centred squares
    {
      float ps[4];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            float d = acc[blk >> 1][j][(blk & 1) * 8 + i] - mean[blk];
            s += d * d;
          }
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4); s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 32);
        if (wide) s += __shfl_xor(s, 16);
        ps[blk] = s;
      }
      put(s_sq, ps);
      __syncthreads();
      get(s_sq, ps);
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) rstd[blk] = rsqrtf(ps[blk] * inv_cnt + p.eps);
    }

    }

    // normalise + Mish (+ FiLM | + residual) and store, one 16-row block at a time; the residual rows of
    // the next block are fetched while the current one is processed (bf16: 8 x 8 B per lane in flight)
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      if (res_bf16 && blk < 3) fetch_res(blk + 1, resv[(blk + 1) & 1]);
      f32x4_t fs = {1.f, 1.f, 1.f, 1.f}, fb = {0.f, 0.f, 0.f, 0.f};
      if (p.mode == MODE_GN_MISH_FILM) { fs = film_s[blk]; fb = film_b[blk]; }
      float ga[4], be[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { ga[j] = gam[j] * rstd[blk]; be[j] = bet[j] - mean[blk] * ga[j]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int ii = (blk & 1) * 8 + i;
        const int rofs = (i & 3) + 8 * (i >> 2) + 4 * h;
        const int b = blk_b[blk], l = blk_l[blk] + rofs;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = mish_f<PREC == 1 ? 1 : 0>(acc[blk >> 1][j][ii] * ga[j] + be[j]) * fs[j] + fb[j];
        if (p.mode == MODE_GN_MISH_RES) {
          if constexpr (PREC != 1) {
            const short4_t rv = resv[blk & 1][i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += e2f<ET>((unsigned short)rv[j]);
          } else {
            const long long rrow = (long long)b * p.res_Lp + l + p.res_off;
            const f32x4_t rv = *(const f32x4_t*)((const char*)p.Res + (rrow * p.ldres + n0) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += rv[j];
          }
        }
        const long long orow = (long long)b * p.out_Lp + (long long)l * p.out_stride + p.out_off;
        const long long oidx = orow * p.ldc + p.out_coff + n0;
        if constexpr (PREC == 1) {
          const f32x4_t o = {v[0], v[1], v[2], v[3]};
          *(f32x4_t*)((char*)p.Out + out_extra_bytes + oidx * 4) = o;
        } else {
          short4_t o;
          if constexpr (ET == 1) { sat_see2(satm, v[0], v[1]); sat_see2(satm, v[2], v[3]); }
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (short)f2e<ET>(v[j]);
          *(short4_t*)((char*)p.Out + out_extra_bytes + oidx * 2) = o;
        }
      }
    }
    if constexpr (ET == 1) sat_flush(p.sat, satm);
    return;
  }

  // ---- plain store (MODE_BIAS; ragged M / N allowed) ------------------------------------------------
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ii = (blk & 1) * 8 + i;
      const int rofs = (i & 3) + 8 * (i >> 2) + 4 * h;         // row within the 16-row block
      const int m = tm * 256 + wm * 64 + (blk >> 1) * 32 + (blk & 1) * 16 + rofs;
      if (m >= p.M || !n_ok) continue;
      int b = blk_b[blk], l = blk_l[blk] + rofs;
      if ((p.L & 15) != 0) { b = m / p.L; l = m - b * p.L; }      // short sequences (ant: L = 8, 4): rows of a block span samples
      const long long orow = (long long)b * p.out_Lp + (long long)l * p.out_stride + p.out_off;
      const long long oidx = orow * p.ldc + p.out_coff + n0;
      if (p.out_f32 || PREC == 1) {
        const f32x4_t o = {acc[blk >> 1][0][ii], acc[blk >> 1][1][ii], acc[blk >> 1][2][ii], acc[blk >> 1][3][ii]};
        *(f32x4_t*)((char*)p.Out + out_extra_bytes + oidx * 4) = o;
      } else {
        short4_t o;
        if constexpr (ET == 1) { sat_see2(satm, acc[blk >> 1][0][ii], acc[blk >> 1][1][ii]); sat_see2(satm, acc[blk >> 1][2][ii], acc[blk >> 1][3][ii]); }
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (short)f2e<ET>(acc[blk >> 1][j][ii]);
        *(short4_t*)((char*)p.Out + out_extra_bytes + oidx * 2) = o;
      }
    }
  }
  if constexpr (ET == 1) sat_flush(p.sat, satm);
}

template <int PREC, bool C2D = false>
__global__ void __launch_bounds__(512, 2) conv_gemm_kernel(ConvGemmParams p) {
  constexpr int ES = (PREC == 1) ? 4 : 2;          // element bytes
  constexpr int ET = PREC == 2 ? 1 : 0;
  constexpr int EK = 128 / ES;                     // elements of K per step
  constexpr int EPS = 16 / ES;                     // elements per 16-B slot
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r5 = lane & 31, h = lane >> 5;
  const int wm = w >> 1, wn = w & 1;
  const int ntn = (p.N + 255) >> 8;
  const int ntm = (p.M + 255) >> 8;
  const int tile = xcd_remap(blockIdx.x, ntm * ntn);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int K = p.taps * p.Cin;
  const int kpt = p.Cin / EK;                      // K-steps per tap
  int nk = K / EK;
  int k_first = 0;                                 // split-K (implicit Conv2d): this block's K-step range
  long long out_extra = 0;
  if constexpr (C2D) {
    if (p.splitk > 1) {
      const int per = (nk + p.splitk - 1) / p.splitk;
      k_first = blockIdx.y * per;
      nk = min(nk - k_first, per);
      out_extra = (long long)blockIdx.y * p.slab_stride * 4;     // never write to `p`: a modified kernarg struct is
    }                                                            // copied to scratch and every later read spills
  }

  // ---- per-lane staging sources (byte offsets) ------------------------------------------
  const char* Abase = (const char*)p.A;
  const char* Wbase = (const char*)p.W;
  long long aoff[4], boff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = (w * 4 + q) * 8 + (lane >> 3);          // LDS row 0..255
    const int sw = (r >> 1) & 7;
    const int slot = (lane & 7) ^ sw;
    int m = tm * 256 + r;
    m = m < p.M ? m : p.M - 1;
    const int b = m / p.L, l = m - b * p.L;
    aoff[q] = (((long long)b * p.in_Lp + (long long)l * p.in_stride + p.in_off) * p.lda + slot * EPS) * ES;
    // weight row permutation: LDS row rho = wn*128 + j*32 + rr  <->  channel wn*128 + 4*rr + j
    const int c = (r & 128) + 4 * (r & 31) + ((r >> 5) & 3);
    boff[q] = (((long long)(tn * 256 + c)) * K + slot * EPS) * ES;
  }
  // running per-lane source pointers of the K-step being staged; advanced by a wave-uniform
  // increment per K-step (128 B inside a tap, a row jump at a tap boundary)
  const char* pa[4];
  const char* pb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    pa[q] = Abase + aoff[q];
    pb[q] = Wbase + boff[q] + (long long)k_first * 128;
  }
  int kin = C2D ? (k_first % kpt) : 0;               // K-step index inside the current tap
  const long long a_tap_jump = ((long long)p.lda - (long long)p.Cin + EK) * ES;
  // implicit Conv2d: per staged row the sample base, the top-left input pixel of its window and
  // the swizzled slot; the source pointer is rebuilt for every K-step (tap, channel chunk)
  const char* c2_base[4];
  int c2_ih0[4], c2_iw0[4], c2_slot[4];
  int c2_tap = C2D ? (k_first / kpt) : 0;
  if constexpr (C2D) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = (w * 4 + q) * 8 + (lane >> 3);
      int m = tm * 256 + r;
      m = m < p.M ? m : p.M - 1;
      const int b = m / p.c2_OHW, rem = m - b * p.c2_OHW;
      const int oh = rem / p.c2_OW, ow = rem - oh * p.c2_OW;
      c2_base[q] = Abase + (long long)b * p.c2_H * p.c2_W * p.Cin * ES;
      c2_ih0[q] = oh * p.c2_stride - p.c2_pad;
      c2_iw0[q] = ow * p.c2_stride - p.c2_pad;
      c2_slot[q] = ((lane & 7) ^ ((r >> 1) & 7)) * 16;
    }
  }
  auto c2_point = [&]() {                              // pa[] for K-step (c2_tap, kin)
    const int kh = p.c2_kh[c2_tap], kw = p.c2_kw[c2_tap];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ih = c2_ih0[q] + kh, iw = c2_iw0[q] + kw;
      const bool ok = ih >= 0 && ih < p.c2_H && iw >= 0 && iw < p.c2_W;
      const char* src = c2_base[q] + ((long long)(ih * p.c2_W + iw) * p.Cin + kin * EK) * ES;
      pa[q] = (ok ? src : (const char*)p.zero) + c2_slot[q];
    }
  };
  if constexpr (C2D) c2_point();
  auto advance = [&]() {
    ++kin;
    if constexpr (C2D) {
      if (kin == kpt) { kin = 0; ++c2_tap; }
      if (c2_tap < p.taps) c2_point();
#pragma unroll
      for (int q = 0; q < 4; ++q) pb[q] += 128;
    } else {
      long long ainc = 128;
      if (kin == kpt) { kin = 0; ainc = a_tap_jump; }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pa[q] += ainc;
        pb[q] += 128;
      }
    }
  };
  // one 1-KiB piece (q = 0..3: activations, 4..7: weights) into the LDS stage at `sbase`
  auto stage_piece = [&](int q, char* sbase) {
    if (q < 4)
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)pa[q], (LDS_AS void*)(sbase + (w * 4 + q) * 1024), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)pb[q - 4],
                                       (LDS_AS void*)(sbase + 32768 + (w * 4 + q - 4) * 1024), 16, 0, 0);
  };

  f32x16_t acc[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][j][i] = 0.0f;

  const int swl = (r5 >> 1) & 7;
  const int a_row_off = (wm * 64 + r5) * 128;               // + mb*32*128
  const int b_row_off = 32768 + (wn * 128 + r5) * 128;      // + j*32*128

  // K-step body.  STAGE: also issue the 8 LDS-DMA pieces of K-step kt+1, two per 16-wide
  // sub-step, interleaved with the MFMAs (an LDS-DMA issue costs the wave 60+ cycles; behind
  // an MFMA it is hidden, in front of the first ds_read it is not).
  auto kstep = [&](const char* sb, auto stage_tag, char* snext) {
    constexpr bool STAGE = decltype(stage_tag)::value;
    if constexpr (PREC != 1) {
      short8_t af[2][2], bfr[2][4];
      auto rd = [&](int ks, int slot) {
        const int ps = (((ks << 1) | h) ^ swl) << 4;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
          af[slot][mb] = *(const short8_t*)(sb + a_row_off + mb * 4096 + ps);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bfr[slot][j] = *(const short8_t*)(sb + b_row_off + j * 4096 + ps);
      };
      if constexpr (STAGE) {
#pragma unroll
        for (int q = 0; q < 8; ++q) stage_piece(q, snext);
      }
      rd(0, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < 3) rd(ks + 1, (ks + 1) & 1);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[mb][j] = mfma32<ET>(af[ks & 1][mb], bfr[ks & 1][j], acc[mb][j]);
      }
      // pin the order: the next tile's LDS-DMA first (it has the whole step to land), then for every
      // sub-step the reads of the following one ahead of its own 8 MFMAs (true fragment double buffering;
      // left alone hipcc sinks the reads behind the MFMAs and waits for LDS in front of every group)
      if constexpr (STAGE) __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < 3) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      }
    } else {
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {                       // 16-B slot = 4 floats = k 4*sl .. 4*sl+3
        const int ps = (sl ^ swl) << 4;
        f32x4_t af[2], bfr[4];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) af[mb] = *(const f32x4_t*)(sb + a_row_off + mb * 4096 + ps);
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = *(const f32x4_t*)(sb + b_row_off + j * 4096 + ps);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {                     // k pair (2*s2, 2*s2+1): lane half h takes k = 2*s2 + h
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) {
            const float a = h ? af[mb][2 * s2 + 1] : af[mb][2 * s2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float bv = h ? bfr[j][2 * s2 + 1] : bfr[j][2 * s2];
              acc[mb][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[mb][j], 0, 0, 0);
            }
          }
        }
        if constexpr (STAGE) stage_piece(sl, snext);
      }
    }
  };

#pragma unroll
  for (int q = 0; q < 8; ++q) stage_piece(q, smem);
  advance();
  for (int kt = 0; kt < nk - 1; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    kstep(smem + (kt & 1) * 65536, std::true_type{}, smem + ((kt + 1) & 1) * 65536);
    advance();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  kstep(smem + ((nk - 1) & 1) * 65536, std::false_type{}, nullptr);
  __syncthreads();                                            // all fragment reads done: LDS reusable
  gemm_epilogue<PREC>(p, acc, smem, tm, tn, tid, lane, r5, h, wm, wn, out_extra);
}

// =================================================================================================
// conv3_halo16_kernel: the halo kernel on v_mfma_f32_16x16x32_bf16.
//
// Same tile (256 x 256, 8 waves 4(M) x 2(N), wave tile 64 x 128), same LDS images, staging and
// barrier protocol as conv3_halo_kernel; only the MFMA shape and with it the fragment / accumulator
// geometry differ.  Measured in situ (same loop, two 16x16x32 per 32x32x16): the chip holds a higher
// clock on this shape under load, -8.4 % kernel time at equal cycles, FLOPs and LDS bytes
// (MI355X_MICROARCH.md "DVFS give-back" (7)).
//   lane (r4 = lane & 15, h4 = lane >> 4); acc[mb][j][i]: tile row wm*64 + mb*16 + 4*h4 + i,
//   tile channel wn*128 + 8*r4 + j  (W rows are permuted in LDS so a lane owns 8 consecutive channels:
//   16-B stores, 256 B contiguous per row).
//   A K-step (64 channels of one tap) is four phases of 16 MFMAs: (ks, j-half) = (0,0) (0,1) (1,0) (1,1);
//   A fragments are double-buffered per 32-deep sub-step, B fragments per half (64 fragment VGPRs in all);
//   phase n reads what phase n+1 needs; the barrier sits before the last phase, which carries the LDS-DMA issue.
// =================================================================================================
template <int ET, bool SPLIT, bool SHORT = false>
__device__ __forceinline__ void gemm_epilogue16(const ConvGemmParams& p, f32x4_t (&acc)[4][8], char* smem, int tm, int tn,
                                                int tid, int lane, int r4, int h4, int wm, int wn) {
  const int c_l = wn * 128 + 8 * r4;                          // lane's 8 consecutive channels in the tile
  const int n0 = tn * 256 + c_l;
  {
    f32x4_t b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (p.bias != nullptr) { b0 = *(const f32x4_t*)(p.bias + n0); b1 = *(const f32x4_t*)(p.bias + n0 + 4); }
    if constexpr (ET == 1) {                                  // f16 weights are stored scaled by a power of two
      const float ws = p.w_scale;
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[mb][j] = acc[mb][j] * ws + b0[j]; acc[mb][4 + j] = acc[mb][4 + j] * ws + b1[j]; }
    } else if (p.bias != nullptr) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[mb][j] += b0[j]; acc[mb][4 + j] += b1[j]; }
    }
  }
  // 16-row block mb of this wave: tile rows wm*64 + mb*16 .. +15.  16 | L: the block lies inside one sample.  L = 8, 4 (the ant
  // config's lower levels): the block holds 2 / 4 samples, but the four rows 4*h4 .. 4*h4 + 3 a LANE owns are consecutive
  // positions of ONE sample (4 | L): sample blk_b + lane_b, first position blk_l + 4*h4 + lane_l with the per-lane offsets below
  // (L | 16, so they do not depend on the block).  SHORT is its own instantiation (gemm16_kernel at L = 8 / 4, the split halo
  // kernel at L = 8): the 16 | L kernels have no registers to spare for it.
  constexpr bool short_l = SHORT;
  const int lane_b = short_l ? (4 * h4) / p.L : 0, lane_l = -lane_b * p.L;
  int blk_b[4], blk_l[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int m0 = tm * 256 + wm * 64 + mb * 16;
    const int b = m0 / p.L;
    blk_b[mb] = b;
    blk_l[mb] = m0 - b * p.L;
  }
  // SPLIT: the row goes out as two planes, hi = rnd16(v) and lo = rnd16(v - hi).  f16 saturates at +-65504 (one
  // v_med3 per element, before the split: |v - hi| is below half an ulp of hi and needs no clamp of its own).
  auto store_row = [&](char* o, const float (&v)[8]) {
    short8_t hi, lo;
    if constexpr (ET == 1) {
      sat_check_row(p.sat, v);                                // f16 range guard
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const f32x2_t c = {__builtin_amdgcn_fmed3f(v[2 * jj], -65504.0f, 65504.0f),
                           __builtin_amdgcn_fmed3f(v[2 * jj + 1], -65504.0f, 65504.0f)};
        const half2_t h = __builtin_convertvector(c, half2_t);                  // v_cvt_pk_f16_f32 (RNE)
        const short2_t hs = __builtin_bit_cast(short2_t, h);
        hi[2 * jj] = hs[0]; hi[2 * jj + 1] = hs[1];
        if constexpr (SPLIT) {
          const half2_t l = __builtin_convertvector(c - __builtin_convertvector(h, f32x2_t), half2_t);
          const short2_t ls = __builtin_bit_cast(short2_t, l);
          lo[2 * jj] = ls[0]; lo[2 * jj + 1] = ls[1];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        hi[j] = (short)f2bf(v[j]);
        if constexpr (SPLIT) lo[j] = (short)f2bf(v[j] - bf2f((unsigned short)hi[j]));
      }
    }
    *(short8_t*)o = hi;
    if constexpr (SPLIT) *(short8_t*)(o + p.out_plane) = lo;
  };
  // first row of 16-row block mb of this lane (row 4*h4 of the block), and the byte step to the next row
  auto out_ptr = [&](int mb, int esize) {
    const long long orow = (long long)(blk_b[mb] + lane_b) * p.out_Lp + (long long)(blk_l[mb] + 4 * h4 + lane_l) * p.out_stride + p.out_off;
    return (char*)p.Out + (orow * p.ldc + p.out_coff + n0) * esize;
  };
  if (p.mode < MODE_GN_MISH) {                                // plain store: 16-bit activations, or f32 (the FiLM table)
    const int esize = p.out_f32 ? 4 : 2;
    const long long ostep = (long long)p.out_stride * p.ldc * esize;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      char* ob = out_ptr(mb, esize);
#pragma unroll
      for (int i = 0; i < 4; ++i, ob += ostep) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = acc[mb][j][i];
        if (p.out_f32) {
          *(f32x4_t*)ob = f32x4_t{v[0], v[1], v[2], v[3]};
          *(f32x4_t*)(ob + 16) = f32x4_t{v[4], v[5], v[6], v[7]};
        } else {
          store_row(ob, v);
        }
      }
    }
    return;
  }
  // LDS (free after the K loop): GroupNorm sums, then the tile's per-channel and per-sample operands.  They are read
  // back block by block (16 transient registers instead of 48 resident ones: the accumulators fill the register file),
  // and an LDS read does not queue behind the row stores the way a global load does (see below).
  const bool has_film = p.mode == MODE_GN_MISH_FILM, has_res = p.mode == MODE_GN_MISH_RES;
  const int spt = 256 / p.L;                                  // samples per tile: 4 .. 16, 32 (L = 8), 64 (L = 4)
  const int ns = spt > 16 ? spt * 4 : 64;                     // statistics cells: [sample of the tile][4 groups]
  float* s_sum = (float*)smem;
  float* s_sq = s_sum + ns;
  float* s_gb = s_sq + ns;                                    // gamma[256] | beta[256] of the tile's channels
  float* s_film = s_gb + 512;                                 // FiLM rows of the tile's samples: [slot][scale 256 | bias 256]
  // short samples: 64 FiLM rows would not fit the LDS -- a lane reads its sample's 2 x 8 values from the table itself, one
  // block ahead (below)
  const bool film_direct = has_film && short_l;
  const int b_last = p.M / p.L - 1;
  for (int i = tid; i < 2 * ns; i += 512) s_sum[i] = 0.0f;
  s_gb[tid] = tid < 256 ? p.gamma[tn * 256 + tid] : p.beta[tn * 256 + tid - 256];
  if (has_film && !film_direct) {
    for (int idx = tid; idx < spt * 128; idx += 512) {
      const int sm = idx >> 7, c4 = idx & 127;
      const int b = min(tm * spt + sm, b_last);
      const float* src = p.film + (long long)b * p.film_ld + p.film_off + tn * 256 + (c4 & 63) * 4 + (c4 >> 6) * p.N;
      *(f32x4_t*)(s_film + sm * 512 + c4 * 4) = *(const f32x4_t*)src;
    }
  }
  // The memory counter (vmcnt) retires in issue order and counts stores too: a load that is waited for behind a row's
  // stores pays their round trip.  The residual rows therefore run in a ring of two tile rows (8 channels: hi [, lo]
  // per row), refilled as soon as a pair has been read -- before the stores of that pair are issued.
  f32x4_t rh[2], rl[2];                                       // (film_direct: the same registers hold the next block's FiLM values)
  const long long rstep = (long long)p.ldres * 2;
  auto fetch_film = [&](int mb) {
    const float* fr = p.film + (long long)min(blk_b[mb] + lane_b, b_last) * p.film_ld + p.film_off + n0;
    rh[0] = *(const f32x4_t*)fr; rh[1] = *(const f32x4_t*)(fr + 4);
    rl[0] = *(const f32x4_t*)(fr + p.N); rl[1] = *(const f32x4_t*)(fr + p.N + 4);
  };
  if (film_direct) fetch_film(0);
  auto fetch_res = [&](int r) {
    const long long rrow = (long long)(blk_b[r >> 2] + lane_b) * p.res_Lp + blk_l[r >> 2] + 4 * h4 + lane_l + p.res_off;
    const char* rp = (const char*)p.Res + (rrow * p.ldres + n0) * 2 + (r & 3) * rstep;
    rh[r & 1] = *(const f32x4_t*)rp;
    if constexpr (SPLIT) rl[r & 1] = *(const f32x4_t*)(rp + p.res_plane);
  };
  if (has_res) { fetch_res(0); fetch_res(1); }
  __syncthreads();
  const int gi = c_l / p.group_ch;
  const bool wide = p.group_ch >= 128;
  const float inv_cnt = 1.0f / (float)(p.group_ch * p.L);
  int slot[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) slot[mb] = (blk_b[mb] + lane_b - tm * spt) * 4 + gi;
  // group reduction of the per-lane partials of the four row blocks: the 16 lanes r4 of a row hold 8 channels each ->
  // DPP adds inside the row of 16 lanes (xor 1, 2, 4: 64 channels; the mirror of 16 when the group is 128+ wide), the
  // four rows h4 by two lane exchanges, and one lane per group adds into the sample's LDS cell.  For L <= 64 a cell is
  // fed by one wave (in program order) or by the two wn waves of a 256-wide group with one add each, so the sum does not
  // depend on the order the adds land in: results are reproducible bit for bit, whatever batch a sample is part of.
  // That does not hold where several waves feed a cell with more than one add each: L >= 128 (a sample's rows span two or
  // four wm waves with four row blocks each) and a 256-wide group at L = 32 / 64 (both wn waves, two / four row blocks each).
  // Those levels are `ordered`: a wave adds its row blocks of a sample in registers and writes the sum to a cell of its
  // own, [wm][wn][group][sample of the wave (two at L = 32)] = 64 cells (at most 2 x 4 x 4 of them are a sample's), and
  // cell_sums() adds a sample's cells in index order after the barrier.  Cells that no wave writes stay 0.
  const bool ordered = !short_l && (p.L >= 128 || (p.group_ch == 256 && p.L >= 32));
  // rows h4 of one sample: all four (16 | L), pairs (L = 8), each its own (L = 4)
  const int hsame = short_l ? (p.L == 8 ? 2 : 1) : 4;
  const bool adder = (r4 == 0 || (!wide && r4 == 8)) && (h4 & (hsame - 1)) == 0;
  const int ocell = ((wm * 2 + wn) * 4 + gi) * 2;
  auto block_sums = [&](float (&s)[4], float* cell) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) s[mb] = dpp_add<0xB1>(s[mb]);           // quad_perm [1,0,3,2]
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) s[mb] = dpp_add<0x4E>(s[mb]);           // quad_perm [2,3,0,1]
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) s[mb] = dpp_add<0x141>(s[mb]);          // row_half_mirror
    if (wide) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) s[mb] = dpp_add<0x140>(s[mb]);        // row_mirror
    }
    if (hsame >= 2) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) s[mb] += __shfl_xor(s[mb], 16);
    }
    if (hsame == 4) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) s[mb] += __shfl_xor(s[mb], 32);
    }
    if (ordered) {
      if (p.L >= 64) { s[0] = (s[0] + s[1]) + (s[2] + s[3]); s[2] = 0.0f; }
      else { s[0] += s[1]; s[2] += s[3]; }                                   // L = 32: row blocks 0, 1 | 2, 3
      if (adder) { cell[ocell] = s[0]; cell[ocell + 1] = s[2]; }
    } else if (adder) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) atomicAdd(&cell[slot[mb]], s[mb]);
    }
  };
  // the statistics of the samples of the four row blocks
  auto cell_sums = [&](const float* cell, float (&t)[4]) {
    if (!ordered) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) t[mb] = cell[slot[mb]];
      return;
    }
#pragma unroll
    for (int mb = 0; mb < 4; mb += 2) {
      const int r0 = (blk_b[mb] - tm * spt) * p.L;                           // the sample's first row in the tile
      const int w0 = r0 >> 6, nw = p.L >= 64 ? p.L >> 6 : 1, sub = (r0 >> 5) & 1;
      float v = 0.0f;
      for (int w = w0; w < w0 + nw; ++w) {
        v += cell[((w * 2 + 0) * 4 + gi) * 2 + sub];
        v += cell[((w * 2 + 1) * 4 + gi) * 2 + sub];
      }
      t[mb] = v; t[mb + 1] = v;
    }
  };
  float mean_[4], rstd_[4];
  auto pair = [&](int mb, int j, int ip) { return f32x2_t{acc[mb][j][2 * ip], acc[mb][j][2 * ip + 1]}; };
  if constexpr (!SPLIT) {
    // one pass: sum and sum of squares (f32), var = E[x^2] - mean^2
    float s[4], q[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      f32x2_t s2 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
          const f32x2_t v = pair(mb, j, ip);
          s2 += v;
          q2 = __builtin_elementwise_fma(v, v, q2);
        }
      s[mb] = s2[0] + s2[1];
      q[mb] = q2[0] + q2[1];
    }
    block_sums(s, s_sum);
    block_sums(q, s_sq);
    __syncthreads();
    cell_sums(s_sum, s);
    cell_sums(s_sq, q);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      mean_[mb] = s[mb] * inv_cnt;
      const float var = fmaxf(q[mb] * inv_cnt - mean_[mb] * mean_[mb], 0.0f);
      rstd_[mb] = rsqrtf(var + p.eps);
    }
  } else {
    // f32-class instantiations: mean first, then centred squares (as torch's GroupNorm)
    float s[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      f32x2_t s2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) s2 += pair(mb, j, ip);
      s[mb] = s2[0] + s2[1];
    }
    block_sums(s, s_sum);
    __syncthreads();
    cell_sums(s_sum, s);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      mean_[mb] = s[mb] * inv_cnt;
      f32x2_t q2 = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int ip = 0; ip < 2; ++ip) {
          const f32x2_t d = pair(mb, j, ip) - mean_[mb];
          q2 = __builtin_elementwise_fma(d, d, q2);
        }
        if (j & 1) __builtin_amdgcn_sched_barrier(0);         // keeps the differences short-lived (they would spill)
      }
      s[mb] = q2[0] + q2[1];
    }
    block_sums(s, s_sq);
    __syncthreads();
    cell_sums(s_sq, s);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) rstd_[mb] = rsqrtf(s[mb] * inv_cnt + p.eps);
  }
  // rows go through the arithmetic two at a time (rows 2ip, 2ip+1 of a block: the accumulator pairs above)
  const long long ostep = (long long)p.out_stride * p.ldc * 2;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    float mean = mean_[mb];
    const float rstd = rstd_[mb];
    // (SPLIT: x - mean is formed again here.  Made opaque so that the compiler does not keep the 128 centred values of
    // the statistics pass alive next to the accumulators instead)
    if constexpr (SPLIT) asm volatile("" : "+v"(mean));
    float ga[8], be[8], fs[8], fb[8];
    {
      const f32x4_t gam0 = *(const f32x4_t*)(s_gb + c_l), gam1 = *(const f32x4_t*)(s_gb + c_l + 4);
      const f32x4_t bet0 = *(const f32x4_t*)(s_gb + 256 + c_l), bet1 = *(const f32x4_t*)(s_gb + 256 + c_l + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ga[j] = gam0[j] * rstd; ga[4 + j] = gam1[j] * rstd;
        if constexpr (SPLIT) { be[j] = bet0[j]; be[4 + j] = bet1[j]; }
        else { be[j] = bet0[j] - mean * ga[j]; be[4 + j] = bet1[j] - mean * ga[4 + j]; }
      }
    }
    if (film_direct) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { fs[j] = rh[0][j]; fs[4 + j] = rh[1][j]; fb[j] = rl[0][j]; fb[4 + j] = rl[1][j]; }
      if (mb + 1 < 4) fetch_film(mb + 1);                     // issued before this block's stores (vmcnt retires in order)
    } else if (has_film) {
      const float* fr = s_film + (blk_b[mb] - tm * spt) * 512 + c_l;
      const f32x4_t f0 = *(const f32x4_t*)fr, f1 = *(const f32x4_t*)(fr + 4);
      const f32x4_t f2 = *(const f32x4_t*)(fr + 256), f3 = *(const f32x4_t*)(fr + 260);
#pragma unroll
      for (int j = 0; j < 4; ++j) { fs[j] = f0[j]; fs[4 + j] = f1[j]; fb[j] = f2[j]; fb[4 + j] = f3[j]; }
    }
    char* ob = out_ptr(mb, 2);
#pragma unroll
    for (int ip = 0; ip < 2; ++ip, ob += 2 * ostep) {
      const int r = mb * 4 + 2 * ip;
      f32x2_t v[8];
      if (has_res) {
        const short8_t h0 = __builtin_bit_cast(short8_t, rh[0]), h1 = __builtin_bit_cast(short8_t, rh[1]);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f32x2_t{e2f<ET>((unsigned short)h0[j]), e2f<ET>((unsigned short)h1[j])};
        if constexpr (SPLIT) {
          const short8_t l0 = __builtin_bit_cast(short8_t, rl[0]), l1 = __builtin_bit_cast(short8_t, rl[1]);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += f32x2_t{e2f<ET>((unsigned short)l0[j]), e2f<ET>((unsigned short)l1[j])};
        }
        if (r + 2 < 16) { fetch_res(r + 2); fetch_res(r + 3); }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f32x2_t{0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f32x2_t x = pair(mb, j, ip);
        if constexpr (SPLIT) x = (x - mean) * ga[j] + be[j];
        else x = x * ga[j] + be[j];
        x = mish2<SPLIT ? 2 : 0>(x);
        v[j] += x;
      }
      if (has_film) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * fs[j] + fb[j];
      }
      float row[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) row[j] = v[j][0];
      store_row(ob, row);
#pragma unroll
      for (int j = 0; j < 8; ++j) row[j] = v[j][1];
      store_row(ob + ostep, row);
      __builtin_amdgcn_sched_barrier(0);                      // one row pair at a time: interleaved pairs spill
    }
  }
}

// ---- shared by the two halo kernels ------------------------------------------------------------------
// 16 MFMAs of a 4 x 4 block in snake order: consecutive MFMAs always share one operand (A along a row, B at the turn)
template <int ET>
__device__ __forceinline__ void mm16_snake(f32x4_t (&acc)[4][8], const short8_t (&a)[4], const short8_t (&b)[4], int half) {
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = (mb & 1) ? 3 - jj : jj;
      acc[mb][half * 4 + j] = mfma16<ET>(a[mb], b[j], acc[mb][half * 4 + j]);
    }
}

// Activation fragment addresses as loop invariants (LM = 16, 32, 64; LM = 0: L at run time, none).
// Fragment (mb, tap t) of a lane reads row lrow0 + d, d = halo_frag_step(mb) + t: 16 rows per mb plus the two halo rows of
// every sample boundary crossed, which for 16 | L does not depend on the wave.  Its byte address in the A block is
//     (lrow0 + d) * 128 + (((plane * 4 + h4) ^ ((lrow0 + d) & 7)) << 4)
//   = [lrow0 * 128 + ((h4 ^ ((lrow0 + (d & 7)) & 7)) << 4)]  ^  plane * 64   +  d * 128
// a per-lane base that only depends on d & 7 (3 / 5 / 8 distinct values at L >= 64 / 32 / 16), one XOR for the lo plane, and
// a constant that goes into the immediate offset of ds_read_b128 together with the buffer offset (< 64 KB).  The bases hold
// the LDS address of the block itself (lds0), so that no add is left in front of a read: the XOR then needs the block on a
// 128-byte boundary, which the halo kernels declare.
template <int LM>
__device__ __forceinline__ constexpr int halo_frag_step(int mb) {
  return LM == 16 ? 18 * mb : LM == 32 ? 16 * mb + 2 * (mb >> 1) : 16 * mb;
}
template <int LM>
__device__ __forceinline__ constexpr unsigned halo_frag_keys() {      // bit k: some fragment has d & 7 = k
  unsigned m = 0;
  for (int mb = 0; mb < 4; ++mb)
    for (int t = 0; t < 3; ++t) m |= 1u << ((halo_frag_step<LM>(mb) + t) & 7);
  return m;
}
template <int LM>
__device__ __forceinline__ void halo_frag_bases(unsigned (&abase)[8], unsigned lds0, int lrow0, int h4) {
#pragma unroll
  for (int k = 0; k < 8; ++k) abase[k] = LM != 0 ? lds0 + (unsigned)(lrow0 * 128 + ((h4 ^ ((lrow0 + k) & 7)) << 4)) : 0u;
}
__device__ __forceinline__ short8_t halo_frag_read(unsigned addr) { return *(const LDS_AS short8_t*)(size_t)addr; }

#ifdef HALO16_STAMP   // diagnostic build only: in-kernel clock of the K loop (MI355X_MICROARCH.md, DVFS give-back (6))
__device__ unsigned long long g_halo_stamp[8];
extern "C" int ditree_debug_halo_stamp(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_halo_stamp), sizeof(g_halo_stamp));
}
__device__ unsigned int g_x3_phase[8][32];
extern "C" int ditree_debug_x3_phase(unsigned int* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_x3_phase), sizeof(g_x3_phase));
}
// per-block timeline of the split halo kernel: {t_start, t_loop, t_epilogue, t_end} (100 MHz real-time clock),
// {nv, block, HW_ID, XCC_ID}; one record per work-group, launch order
#define X3_STAMP_MAX 65536
__device__ unsigned long long g_x3_stamp[X3_STAMP_MAX][6];
__device__ unsigned int g_x3_count;
extern "C" int ditree_debug_x3_stamp(unsigned long long* out, unsigned int* count, int reset) {
  int rc = (int)hipMemcpyFromSymbol(count, HIP_SYMBOL(g_x3_count), 4);
  if (rc == 0 && out != nullptr) rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_x3_stamp), sizeof(unsigned long long) * 6 * X3_STAMP_MAX);
  if (rc == 0 && reset) { unsigned int z = 0; rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(g_x3_count), &z, 4); }
  return rc;
}
#endif
template <int ET, int LM>
__device__ __forceinline__ void conv3_halo16_body(const ConvGemmParams& p) {
  extern __shared__ __attribute__((aligned(128))) char smem_halo[];   // 128: halo_frag_bases
  static_assert(LM == 0 || LM == 16 || LM == 32 || LM == 64, "L at run time, or L = 16, 32, 64 (halo_frag_step)");
  constexpr int A_BUF = 40960, W_BUF = 32768, W_BASE = 2 * A_BUF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);          // wave index: uniform, keeps every wave-level offset in SGPRs
  const int r4 = lane & 15, h4 = lane >> 4;
  const int wm = w >> 1, wn = w & 1;
  const int ntn = (p.N + 255) >> 8;
  const int ntm = (p.M + 255) >> 8;
  const int tile = xcd_remap_strips(blockIdx.x, ntm, ntn, p.xcd_strips);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int L = p.L, Lp = p.in_Lp, S = 256 / L;
  const int a_rows = S * Lp;
  const int nc = p.Cin >> 6;                                         // 64-channel chunks
  const long long K = 3LL * p.Cin;

  // ---- staging sources (buffer addressing, as conv3_halo_kernel) ------------------------------------
  // pieces 0..3 of the A block differ by 64 rows (a wave-uniform byte offset, folded into the scalar offset);
  // only piece 4 can run past the block and is clamped per lane
  unsigned pa0, pa4, pb;
  const char* const a_base = (const char*)p.A + ((long long)tm * S * Lp + p.in_off) * p.lda * 2;
  const char* const w_base = (const char*)p.W + ((long long)tn * 256) * K * 2;
  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a_base, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, 0x7fffffff, 0x00020000);
  {
    const int r = w * 8 + (lane >> 3);                               // LDS row of the A block, piece 0
    const int slot = (lane & 7) ^ (r & 7);                           // (r + 64 i) & 7 is the same for every piece
    pa0 = (unsigned)((r * p.lda + slot * 8) * 2);
    const int r4r = r + 256;
    const int rs = r4r < a_rows ? r4r : a_rows - 1;
    pa4 = (unsigned)((rs * p.lda + slot * 8) * 2);
  }
  const int a_piece = 64 * p.lda * 2;                                // bytes between pieces
  // W tile: LDS row r = (w*4 + q)*8 + (lane >> 3) holds channel c(r) = (r & 128) + 8*(r & 15) + ((r >> 4) & 7)
  // (row wn*128 + j*16 + r4 <- channel wn*128 + 8*r4 + j).  Per lane only 8*(lane >> 3) and the swizzled slot vary,
  // and r & 7 = lane >> 3 for every piece q: one lane offset + a wave-uniform row offset.
  long long wq[4];
  {
    const int lr = lane >> 3;
    const int slot = (lane & 7) ^ lr;                                // r & 7 = lr for every piece q
    pb = (unsigned)(((long long)(8 * lr) * K + slot * 8) * 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r0 = (w * 4 + q) * 8;                                // row with lane >> 3 = 0
      const int cu = (r0 & 128) + 8 * (r0 & 8) + ((r0 >> 4) & 7);    // wave-uniform part of c(r)
      wq[q] = (long long)cu * K * 2;
    }
  }
  const int w_tap = p.Cin * 2;
  // par = parity of the LDS buffer the request / the read goes to ((c & 1) activations, ((c + t) & 1) weights): a constant in
  // the two-chunk loop body
  auto issue_a = [&](int par, int c, int i) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (LDS_AS void*)(smem_halo + par * A_BUF + (w + 8 * i) * 1024), 16,
                                             i < 4 ? pa0 : pa4, c * 128 + (i < 4 ? i * a_piece : 0), 0, 0);
  };
  auto issue_w = [&](int par, int c, int t, int q) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (LDS_AS void*)(smem_halo + W_BASE + par * W_BUF + (w * 4 + q) * 1024),
                                             16, pb, (int)wq[q] + c * 128 + t * w_tap, 0, 0);
  };

  // ---- fragment addressing ---------------------------------------------------------------------
  // row of the A block of fragment row (wm*64 + mb*16 + r4): lrow0 + a wave-uniform step (16 rows per mb plus the
  // two halo rows of every sample boundary crossed; 16 | L) + tap.  LM != 0: every address is one of the per-lane bases
  // + an immediate (halo_frag_bases)
  int lrow0;
  {
    const int ml = wm * 64 + r4;
    const int sb = ml / L;
    lrow0 = sb * Lp + (ml - sb * L);                                 // + tap
  }
  int lstep[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) lstep[mb] = 16 * mb + 2 * (((wm * 64 + 16 * mb) / L) - ((wm * 64) / L));
  unsigned abase[8];
  halo_frag_bases<LM>(abase, (unsigned)(size_t)(LDS_AS char*)smem_halo, lrow0, h4);
  // weight fragments of the fixed forms: one base per ks; buffer, half and jj are immediates (< 48 KB above W_BASE)
  unsigned bbase[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    bbase[ks] = (unsigned)(size_t)(LDS_AS char*)smem_halo + (unsigned)(W_BASE + (wn * 128 + r4) * 128 + ((((ks << 2) | h4) ^ (r4 & 7)) << 4));

  f32x4_t acc[4][8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[mb][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  short8_t af[2][4], bq[2][4];
  auto rdA = [&](int set, int par, int t, int ks) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      if constexpr (LM != 0) {          // one base register (ks = 1: one XOR) + an immediate
        const int d = halo_frag_step<LM>(mb) + t;
        af[set][mb] = halo_frag_read((abase[d & 7] ^ (unsigned)(ks << 6)) + (unsigned)(par * A_BUF + d * 128));
      } else {
        const int row = lrow0 + lstep[mb] + t;
        const int ps = (((ks << 2) | h4) ^ (row & 7)) << 4;
        af[set][mb] = *(const short8_t*)(smem_halo + par * A_BUF + row * 128 + ps);
      }
    }
  };
  auto rdB = [&](int set, int par, int ks, int half) {
    if constexpr (LM != 0) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) bq[set][jj] = halo_frag_read(bbase[ks] + (unsigned)(par * W_BUF + half * 8192 + jj * 2048));
    } else {
      const char* wb = smem_halo + W_BASE + par * W_BUF + (wn * 128 + r4) * 128 + half * 8192;
      const int psb = (((ks << 2) | h4) ^ (r4 & 7)) << 4;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) bq[set][jj] = *(const short8_t*)(wb + jj * 2048 + psb);
    }
  };
  auto mm = [&](int aset, int bset, int half, int mb, int jj) {
    acc[mb][half * 4 + jj] = mfma16<ET>(af[aset][mb], bq[bset][jj], acc[mb][half * 4 + jj]);
  };
  auto mm16 = [&](int aset, int bset, int half) { mm16_snake<ET>(acc, af[aset], bq[bset], half); };

  // One K-step (chunk c, tap T); flags as in conv3_halo_kernel.  On entry af[0] = A(ks 0), bq[0] = B(ks 0, half 0).
  // Wave priorities and the placement of the LDS-DMA requests: see conv3_halo16x3_kernel (same scheme, four phases).
  auto step = [&](auto tT, auto tNext, auto tIW, auto tIA, auto tVM, auto tPar, int c) {
    constexpr int T = decltype(tT)::value;
    constexpr bool HAS_NEXT = decltype(tNext)::value, ISSUE_W = decltype(tIW)::value, ISSUE_A = decltype(tIA)::value;
    constexpr int VM = decltype(tVM)::value;
    constexpr int NV = ISSUE_W ? 4 : 0;
    constexpr int PAR = decltype(tPar)::value;      // c & 1 where the caller knows it, -1 where not
    auto par = [&](int known, int x) { return PAR >= 0 ? known : (x & 1); };
    const int pa = par(PAR, c);                     // activation buffer of chunk c
    const int pw = par((PAR + T) & 1, c + T);       // weight buffer of step (c, T)
    // keep the fragment addresses what they are inside a step: the fixed forms one base register + an immediate (with the
    // XORed ks = 1 bases hoisted out of the loop they spill), the run-time form its arithmetic (hoisted it spills)
    if constexpr (LM != 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((halo_frag_keys<LM>() >> i) & 1) asm volatile("" : "+v"(abase[i]));
    } else {
      asm volatile("" : "+v"(lrow0));
    }
    if constexpr (LM != 0) asm volatile("" : "+v"(bbase[0]), "+v"(bbase[1]));
    // Each phase is its own scheduling region (sched_barrier), inside it the fragment reads for the NEXT phase
    // are issued first, then the 16 MFMAs: hipcc otherwise sinks the reads to the end of the phase and the next
    // phase waits for LDS in front of every MFMA.
    __builtin_amdgcn_s_setprio(2);
    rdB(1, pw, 0, 1);                   // phase (0,0)
    mm16(0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    rdA(1, pa, T, 1);                   // phase (0,1)
    rdB(0, pw, 1, 0);
    mm16(0, 1, 1);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    rdB(1, pw, 1, 1);                   // phase (1,0) + the activation pieces of chunk c+1 (T = 0: 0..2, T = 1: 3, 4)
    mm16(1, 0, 0);
    if constexpr (ISSUE_A && T != 2) {
      const int pa1 = par(PAR ^ 1, c + 1);
      if constexpr (T == 0) { issue_a(pa1, c + 1, 0); issue_a(pa1, c + 1, 1); issue_a(pa1, c + 1, 2); }
      else { issue_a(pa1, c + 1, 3); issue_a(pa1, c + 1, 4); }
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      if constexpr (T == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    } else {
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS_NEXT) {
      if constexpr (VM == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else if constexpr (VM == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(3);
      constexpr int T1 = (T + 1) % 3;
      const int cn = c + (T + 1) / 3;
      rdA(0, par(PAR ^ ((T + 1) / 3), cn), T1, 0);
      rdB(0, par((PAR + T + 1) & 1, cn + T1), 0, 0);
    }
    constexpr int T2 = (T + 2) % 3;
    const int c2 = c + (T + 2) / 3;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)      // phase (1,1) + the weight pieces of step s+2
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        mm(1, 1, 1, mb, (mb & 1) ? 3 - jj : jj);
        const int i = mb * 4 + jj;
        // An LDS-DMA issue holds the wave's instruction stream for 60-180 cycles and both waves of a SIMD run this
        // phase together: one issue behind every second MFMA instead of all in a row leaves the partner wave MFMAs to
        // issue in between (-1.7 % kernel time).
        const int d = (i & 1) ? -1 : (i >> 1);
        if constexpr (ISSUE_W) { if (d >= 0 && d < 4) issue_w(par((PAR + T) & 1, c2 + T2), c2, T2, d); }      // c2 + T2 = c + T + 2 - 2 [T > 0]
      }
    if constexpr (HAS_NEXT) __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      if (!(i & 1) && (i >> 1) < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using Tt = std::true_type;
  using Ff = std::false_type;

  // ---- prologue: A(0), W(0,0) -> visible; then W(0,1) in flight ----------------------------------------
#pragma unroll
  for (int i = 0; i < 5; ++i) issue_a(0, 0, i);
#pragma unroll
  for (int q = 0; q < 4; ++q) issue_w(0, 0, 0, q);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int q = 0; q < 4; ++q) issue_w(1, 0, 1, q);
  rdA(0, 0, 0, 0);
  rdB(0, 0, 0, 0);

#ifdef HALO16_STAMP
  const unsigned long long st0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  // Issue order and counted waits as in conv3_halo16x3_kernel: vmcnt(3) at the barrier of T = 0 (the three activation
  // pieces requested in this step may stay in flight), vmcnt(2) at T = 1, vmcnt(0) at T = 2 (whole next activation stage).
  // Two chunks per trip: the buffer parities are constants and go into the immediates of the fragment reads and of the
  // LDS-DMA destinations; an odd chunk left over and the tails take the parity from c (constant parities there cost
  // registers: the compiler spills).
  using PR = std::integral_constant<int, -1>;
  int c = 0;
  if constexpr (LM != 0) {
    for (; c + 1 < nc - 2; c += 2) {
      step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, I0{}, c);
      step(I1{}, Tt{}, Tt{}, Tt{}, I2{}, I0{}, c);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, I0{}, c);
      step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, I1{}, c + 1);
      step(I1{}, Tt{}, Tt{}, Tt{}, I2{}, I1{}, c + 1);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, I1{}, c + 1);
    }
    for (; c < nc - 2; ++c) {                         // full waits: spills may sit here, as in the tails
      step(I0{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);
      step(I1{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);
    }
  } else {
    for (; c < nc - 2; ++c) {
      step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, PR{}, c);
      step(I1{}, Tt{}, Tt{}, Tt{}, I2{}, PR{}, c);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);
    }
  }
#ifdef HALO16_STAMP
  if (blockIdx.x == 100 && tid == 0 && nc >= 32) {
    g_halo_stamp[0] = __builtin_amdgcn_s_memtime() - st0;
    g_halo_stamp[1] = __builtin_amdgcn_s_memrealtime() - rt0;
    g_halo_stamp[2] = (unsigned long long)(nc - 2) * 3;
  }
#endif
  // The counted waits are only used inside the loop above, whose body holds no other vector-memory operation.  The
  // chunks behind it wait for everything: register spills the compiler may place here (scratch accesses count in vmcnt)
  // must not take part in a counted wait.
  {
    const int c = nc - 2;
    step(I0{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);    // the activation stage of the last chunk
    step(I1{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, c);
    step(I2{}, Tt{}, Tt{}, Ff{}, I0{}, PR{}, c);
  }
  {
    const int c = nc - 1;
    step(I0{}, Tt{}, Tt{}, Ff{}, I0{}, PR{}, c);
    step(I1{}, Tt{}, Ff{}, Ff{}, I0{}, PR{}, c);
    step(I2{}, Ff{}, Ff{}, Ff{}, I0{}, PR{}, c);
  }
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();
  // the epilogue derives its lane indices anew: only tid stays live across the K loop
  int te = tid;
  asm volatile("" : "+v"(te));
  gemm_epilogue16<ET, false>(p, acc, smem_halo, tm, tn, te, te & 63, te & 15, (te & 63) >> 4, wm, wn);
}
// L at run time (what is left: L = 128 / 256), and L = 16 / 32 / 64 with fixed fragment addresses
template <int ET>
__global__ void __launch_bounds__(512, 2) conv3_halo16_kernel(ConvGemmParams p) { conv3_halo16_body<ET, 0>(p); }
template <int ET, int LM>
__global__ void __launch_bounds__(512, 2) conv3_halo16_fixed_kernel(ConvGemmParams p) { conv3_halo16_body<ET, LM>(p); }

// =================================================================================================
// conv3_halo16x3_kernel: the halo kernel for the split (hi + lo) formats.
//
// Same tile, wave geometry, LDS image sizes, double buffers, barrier protocol and epilogue as conv3_halo16_kernel.  What
// differs is what a 128-byte LDS row holds and how many MFMAs a K-step runs on it: a row is [32 channels of the hi plane |
// the same 32 channels of the lo plane] (the 16-byte staging slots 0..3 come from the hi plane, 4..7 from the lo plane --
// only the per-lane source offset knows; the weights are stored chunk-interleaved, so a weight row's eight slots are one
// 128-byte line: ConvGemmParams::w_row / w_step / w_plane), so fragment read "ks = 0" is the hi and "ks = 1" the lo
// fragment of the SAME 32 channels, for activations and weights alike.  One K-step (32 channels of one tap) then forms all
// three products
//      A_hi x W_lo,  A_hi x W_hi,  A_lo x W_hi            (A_lo x W_lo, 2^-22 of the result, is dropped)
// = 96 MFMAs per wave on the bytes a plain K-step stages for 64: against walking the planes as three separate passes
// (what the first version did: 14.7 k candidates/s) a third fewer barriers and LDS-DMA issues per MFMA.
//   Phases (16 MFMAs each; af[0] = A_hi, af[1] = A_lo; bq[] double-buffers the four weight fragment groups):
//     P1 A_hi x W_lo(half 0)   P2 A_hi x W_lo(half 1)   P3 A_hi x W_hi(0)   P4 A_lo x W_hi(0)   P5 A_hi x W_hi(1)
//     -- wait, barrier, read-ahead of the next step's A_hi / W_lo(0) --   P6 A_lo x W_hi(1) + the LDS-DMA issue.
//   The small cross terms are accumulated first.
// =================================================================================================
template <int ET, bool SHORT, bool SPLITK, int NP, int LM>
__device__ __forceinline__ void conv3_halo16x3_body(const ConvGemmParams& p) {
  extern __shared__ __attribute__((aligned(128))) char smem_halo[];   // 128: halo_frag_bases
  // NP staging pieces of 64 rows: 5 hold the 256 + 2 S <= 320 padded rows of a tile at L >= 8; L = 4 (64 samples x 6 padded rows =
  // 384) takes a sixth -- 2 x 48 KB of activations + 2 x 32 KB of weights = all 160 KB of LDS
  static_assert(NP == 5 || NP == 6, "five or six activation pieces");
  static_assert(LM == 0 || (!SHORT && !SPLITK && NP == 5), "fixed fragment addresses: whole-tile, five-piece form, L >= 16");
  constexpr int A_BUF = NP * 8192, W_BUF = 32768, W_BASE = 2 * A_BUF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r4 = lane & 15, h4 = lane >> 4;
  const int wm = w >> 1, wn = w & 1;
  const int ntn = (p.N + 255) >> 8;
  const int ntm = (p.M + 255) >> 8;
  const int tile = xcd_remap_strips(blockIdx.x, ntm, ntn, p.xcd_strips);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  const int L = p.L, Lp = p.in_Lp, S = 256 / L;
  const int a_rows = S * Lp;
  const int nv_all = p.Cin >> 5;                                     // 32-channel chunks
  // SPLITK (latency mode): this work-group walks chunks [v_lo, nv) of the layer's nv_all (host: splitk | nv_all, >= 2 each)
  const int v_lo = SPLITK ? (int)blockIdx.y * (nv_all / p.splitk) : 0;
  const int nv = SPLITK ? v_lo + nv_all / p.splitk : nv_all;
  // weight layout (denoise.h): bytes per row, between 32-channel chunks of a row, and from a chunk's hi to its lo half
  const long long w_row = p.w_row;
  const int w_step = p.w_step;
  const unsigned a_plane = (unsigned)p.a_plane, w_plane = (unsigned)p.w_plane;

  unsigned pa0, pa4, pa5 = 0, pb;
  const char* const a_base = (const char*)p.A + ((long long)tm * S * Lp + p.in_off) * p.lda * 2;
  const char* const w_base = (const char*)p.W + ((long long)tn * 256) * w_row;
  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a_base, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, 0x7fffffff, 0x00020000);
  {
    const int r = w * 8 + (lane >> 3);
    const int slot = (lane & 7) ^ (r & 7);                           // logical slot this lane fetches; 4..7 = lo plane
    const unsigned po = (slot & 4) ? a_plane : 0u;
    pa0 = (unsigned)((r * p.lda + (slot & 3) * 8) * 2) + po;
    const int r4r = r + 256;
    const int rs = r4r < a_rows ? r4r : a_rows - 1;
    pa4 = (unsigned)((rs * p.lda + (slot & 3) * 8) * 2) + po;
    if constexpr (NP == 6) {
      const int r5r = r + 320;
      const int rs5 = r5r < a_rows ? r5r : a_rows - 1;
      pa5 = (unsigned)((rs5 * p.lda + (slot & 3) * 8) * 2) + po;
    }
  }
  const int a_piece = 64 * p.lda * 2;
  long long wq[4];
  {
    const int lr = lane >> 3;
    const int slot = (lane & 7) ^ lr;                                // r & 7 = lr for every piece q
    pb = (unsigned)((long long)(8 * lr) * w_row + (slot & 3) * 16) + ((slot & 4) ? w_plane : 0u);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r0 = (w * 4 + q) * 8;
      const int cu = (r0 & 128) + 8 * (r0 & 8) + ((r0 >> 4) & 7);
      wq[q] = (long long)cu * w_row;
    }
  }
  const int w_tap = (p.Cin >> 5) * w_step;                            // one tap = Cin / 32 chunks further
  // par = parity of the LDS buffer the request / the read goes to ((v & 1) activations, ((v + t) & 1) weights): a constant in
  // the two-chunk loop body of the LM forms
  auto issue_a = [&](int par, int v, int i) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (LDS_AS void*)(smem_halo + par * A_BUF + (w + 8 * i) * 1024), 16,
                                             i < 4 ? pa0 : (i == 4 ? pa4 : pa5), v * 64 + (i < 4 ? i * a_piece : 0), 0, 0);
  };
  auto issue_w = [&](int par, int v, int t, int q) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (LDS_AS void*)(smem_halo + W_BASE + par * W_BUF + (w * 4 + q) * 1024),
                                             16, pb, (int)wq[q] + v * w_step + t * w_tap, 0, 0);
  };

  int lrow0;
  {
    const int ml = wm * 64 + r4;
    const int sb = ml / L;
    lrow0 = sb * Lp + (ml - sb * L);
  }
  int lstep[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) lstep[mb] = 16 * mb + 2 * (((wm * 64 + 16 * mb) / L) - ((wm * 64) / L));
  unsigned abase[8];
  halo_frag_bases<LM>(abase, (unsigned)(size_t)(LDS_AS char*)smem_halo, lrow0, h4);
  const int swl = r4 & 7;
  const int b_row_off = (wn * 128 + r4) * 128;

  f32x4_t acc[4][8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[mb][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  short8_t af[2][4], bq[2][4];
  // pl: 0 = hi plane, 1 = lo plane (slots 0..3 / 4..7 of the row)
  auto rdA = [&](int set, int par, int t, int pl) {
    const char* ab = smem_halo + par * A_BUF;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      if constexpr (LM != 0) {          // one base register (the lo plane: one XOR) + an immediate
        const int d = halo_frag_step<LM>(mb) + t;
        af[set][mb] = halo_frag_read((abase[d & 7] ^ (unsigned)(pl << 6)) + (unsigned)(par * A_BUF + d * 128));
      } else {
        const int row = lrow0 + lstep[mb] + t;
        const int ps = (((pl << 2) | h4) ^ (row & 7)) << 4;
        af[set][mb] = *(const short8_t*)(ab + row * 128 + ps);
      }
    }
  };
  auto rdB = [&](int set, int par, int pl, int half) {
    const char* wb = smem_halo + W_BASE + par * W_BUF + b_row_off + half * 8192;
    const int psb = (((pl << 2) | h4) ^ swl) << 4;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) bq[set][jj] = *(const short8_t*)(wb + jj * 2048 + psb);
  };
  auto mm = [&](int aset, int bset, int half, int mb, int jj) {
    acc[mb][half * 4 + jj] = mfma16<ET>(af[aset][mb], bq[bset][jj], acc[mb][half * 4 + jj]);
  };
  auto mm16 = [&](int aset, int bset, int half) { mm16_snake<ET>(acc, af[aset], bq[bset], half); };

#ifdef X3_PHASE_STAMP     // diagnostic build: issue time (core clock) of every phase of the last full K-steps, per tap
  unsigned pst[24];
#define PSTAMP(k) do { pst[T * 8 + (k)] = (unsigned)__builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PSTAMP(k) do { } while (0)
#endif
  // One K-step (chunk v, tap T).  On entry af[0] = A_hi, bq[0] = W_lo(half 0) of this step.
  //
  // Wave priorities.  The in-kernel phase stamps (profiles/probes/x3_phases.py) showed that the two waves of a SIMD do not
  // share the MFMA pipe: the older one issues back to back (16 MFMAs in 256 cycles), reaches the barrier 1 500 - 2 600
  // cycles early and idles there, the younger one only gets the slots the older one leaves and then runs alone with nobody
  // to cover its LDS waits.  Graded priorities (early phases high, late phases low, the phase behind the barrier highest)
  // let the wave that is behind win the arbitration: the two stay within a phase of each other and arrive together.
  //
  // LDS-DMA issue.  All of a step's requests used to go out behind its barrier (4 weight pieces per wave, and the 5
  // activation pieces of the chunk after next behind the T = 2 barrier): 72 KB per CU in one burst, on every CU at the same
  // moment.  The address FIFO filled, and the younger waves sat 1 500 - 3 000 cycles in ONE buffer_load (MFMAs queued behind
  // it in program order).  The activation pieces now go out in the middle of the following steps (3 in P4 of T = 0, 2 in
  // P4 of T = 1), 16 - 24 KB per CU at a time.
  auto step = [&](auto tT, auto tNext, auto tIW, auto tIA, auto tVM, auto tPar, int v) {
    constexpr int T = decltype(tT)::value;
    constexpr bool HAS_NEXT = decltype(tNext)::value, ISSUE_W = decltype(tIW)::value, ISSUE_A = decltype(tIA)::value;
    constexpr int VM = decltype(tVM)::value;
    constexpr int PAR = decltype(tPar)::value;      // v & 1 where the caller knows it, -1 where not
    auto par = [&](int known, int x) { return PAR >= 0 ? known : (x & 1); };
    const int pa = par(PAR, v);                     // activation buffer of chunk v
    const int pw = par((PAR + T) & 1, v + T);       // weight buffer of step (v, T)
    // keep the fragment addresses what they are inside a step: the fixed forms one base register + an immediate (with the
    // XORed lo-plane bases hoisted out of the loop they spill), the generic form its arithmetic (hoisted it spills)
    if constexpr (LM != 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((halo_frag_keys<LM>() >> i) & 1) asm volatile("" : "+v"(abase[i]));
    } else {
      asm volatile("" : "+v"(lrow0));
    }
    PSTAMP(0);
    __builtin_amdgcn_s_setprio(2);
    rdB(1, pw, 1, 1);                   // P1: A_hi x W_lo(0); fetch W_lo(1)
    mm16(0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(1);
    rdB(0, pw, 0, 0);                   // P2: A_hi x W_lo(1); fetch W_hi(0) and A_lo
    rdA(1, pa, T, 1);
    mm16(0, 1, 1);
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(2);
    __builtin_amdgcn_s_setprio(1);
    rdB(1, pw, 0, 1);                   // P3: A_hi x W_hi(0); fetch W_hi(1)
    mm16(0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(3);
    mm16(1, 0, 0);                      // P4: A_lo x W_hi(0) + the activation pieces of chunk v+1 (T = 0: 0..2, T = 1: 3, 4)
    if constexpr (ISSUE_A && T != 2) {
      const int pa1 = par(PAR ^ 1, v + 1);
      if constexpr (T == 0) { issue_a(pa1, v + 1, 0); issue_a(pa1, v + 1, 1); issue_a(pa1, v + 1, 2); }
      else { issue_a(pa1, v + 1, 3); issue_a(pa1, v + 1, 4); if constexpr (NP == 6) issue_a(pa1, v + 1, 5); }
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 2);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 2);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 2);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 2);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 2);
      if constexpr (T == 0 || NP == 6) __builtin_amdgcn_sched_group_barrier(0x020, 1, 2);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 2);
    }
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(4);
    __builtin_amdgcn_s_setprio(0);
    mm16(0, 1, 1);                      // P5: A_hi x W_hi(1)
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(5);
    if constexpr (HAS_NEXT) {
      if constexpr (VM == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else if constexpr (VM == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(3);
      PSTAMP(6);
      constexpr int T1 = (T + 1) % 3;
      const int vn = v + (T + 1) / 3;
      rdA(0, par(PAR ^ ((T + 1) / 3), vn), T1, 0);  // next step's A_hi and W_lo(0)
      rdB(0, par((PAR + T + 1) & 1, vn + T1), 1, 0);
    }
    constexpr int T2 = (T + 2) % 3;
    const int v2 = v + (T + 2) / 3;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)      // P6: A_lo x W_hi(1) + the weight pieces of step s+2, one behind every second MFMA
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        mm(1, 1, 1, mb, (mb & 1) ? 3 - jj : jj);
        const int i = mb * 4 + jj;
        const int d = (i & 1) ? -1 : (i >> 1);
        if constexpr (ISSUE_W) { if (d >= 0 && d < 4) issue_w(par((PAR + T) & 1, v2 + T2), v2, T2, d); }      // v2 + T2 = v + T + 2 - 2 [T > 0]
      }
    if constexpr (HAS_NEXT) __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
    constexpr int NV = ISSUE_W ? 4 : 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      if (!(i & 1) && (i >> 1) < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    PSTAMP(7);
  };
#undef PSTAMP
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using Tt = std::true_type;
  using Ff = std::false_type;

#ifdef HALO16_STAMP
  const unsigned long long xs0 = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
  for (int i = 0; i < NP; ++i) issue_a(v_lo & 1, v_lo, i);
#pragma unroll
  for (int q = 0; q < 4; ++q) issue_w(v_lo & 1, v_lo, 0, q);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int q = 0; q < 4; ++q) issue_w((v_lo & 1) ^ 1, v_lo, 1, q);
  rdA(0, v_lo & 1, 0, 0);
  rdB(0, v_lo & 1, 1, 0);
#ifdef HALO16_STAMP
  const unsigned long long xs1 = __builtin_amdgcn_s_memrealtime();
#endif

  // Issue order: [behind the barrier of (v-1,2): W(v,1) x 4] [P4 of (v,0): A(v+1)[0..2]] [behind the barrier of (v,0): W(v,2)
  // x 4] [P4 of (v,1): A(v+1)[3,4]] [(v,1): W(v+1,0) x 4] [(v,2): W(v+1,1) x 4] ...  The barrier of a step needs the W
  // pieces requested behind the previous barrier -- what was requested after them may stay in flight: vmcnt(3) at T = 0,
  // vmcnt(2) at T = 1 -- and the barrier of T = 2 the whole activation stage of the next chunk: vmcnt(0).
  using IT1 = std::integral_constant<int, NP == 6 ? 3 : 2>;      // activation pieces requested in P4 of T = 1
  using PR = std::integral_constant<int, -1>;                     // buffer parity from v
  int v = v_lo;
  if constexpr (LM != 0) {
    // two chunks per trip: the buffer parities are constants and go into the immediates of the fragment reads and of the
    // LDS-DMA destinations (v_lo = 0: no split-K form)
    for (; v + 1 < nv - 2; v += 2) {
      step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, I0{}, v);
      step(I1{}, Tt{}, Tt{}, Tt{}, IT1{}, I0{}, v);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, I0{}, v);
      step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, I1{}, v + 1);
      step(I1{}, Tt{}, Tt{}, Tt{}, IT1{}, I1{}, v + 1);
      step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, I1{}, v + 1);
    }
  }
  for (; v < nv - 2; ++v) {             // every chunk of the generic forms; an odd chunk left over in the fixed ones
    step(I0{}, Tt{}, Tt{}, Tt{}, I3{}, PR{}, v);
    step(I1{}, Tt{}, Tt{}, Tt{}, IT1{}, PR{}, v);
    step(I2{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, v);
  }
#ifdef X3_PHASE_STAMP
  if (blockIdx.x == 100 && lane == 0 && nv == 64) {
#pragma unroll
    for (int k = 0; k < 24; ++k) g_x3_phase[w][k] = pst[k];
    g_x3_phase[w][24] = (unsigned)nv;
  }
#endif
  {
    const int v = nv - 2;               // tails wait for everything (no counted wait next to possible spill traffic)
    step(I0{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, v);    // the activation stage of the last chunk
    step(I1{}, Tt{}, Tt{}, Tt{}, I0{}, PR{}, v);
    step(I2{}, Tt{}, Tt{}, Ff{}, I0{}, PR{}, v);
  }
  {
    const int v = nv - 1;
    step(I0{}, Tt{}, Tt{}, Ff{}, I0{}, PR{}, v);
    step(I1{}, Tt{}, Ff{}, Ff{}, I0{}, PR{}, v);
    step(I2{}, Ff{}, Ff{}, Ff{}, I0{}, PR{}, v);
  }
  __builtin_amdgcn_s_setprio(0);
  __syncthreads();
#ifdef HALO16_STAMP
  const unsigned long long xs2 = __builtin_amdgcn_s_memrealtime();
#endif
  if constexpr (SPLITK) {
    const int ntiles = ntm * ntn;
    float* mine = p.sk_ws + ((size_t)blockIdx.y * ntiles + tile) * 65536;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int j = 0; j < 8; ++j) *(f32x4_t*)(mine + ((mb * 8 + j) * 512 + tid) * 4) = acc[mb][j];
    __threadfence();                                          // the slab is visible device-wide before the arrival is counted
    __syncthreads();
    int* s_last = (int*)smem_halo;
    if (tid == 0) *s_last = atomicAdd(p.sk_cnt + tile, 1) == p.splitk - 1;
    __syncthreads();
    const bool last = *s_last != 0;
    __syncthreads();                                          // smem_halo is the epilogue's from here on
    if (!last) return;
    __threadfence();
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[mb][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < p.splitk; ++sp) {                   // split order: the sum does not depend on who arrived last
      const float* sl = p.sk_ws + ((size_t)sp * ntiles + tile) * 65536;
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[mb][j] += *(const f32x4_t*)(sl + ((mb * 8 + j) * 512 + tid) * 4);
    }
    if (tid == 0) p.sk_cnt[tile] = 0;                         // ready for the next launch on this stream
  }
  gemm_epilogue16<ET, true, SHORT>(p, acc, smem_halo, tm, tn, tid, lane, r4, h4, wm, wn);
#ifdef HALO16_STAMP
  __syncthreads();
  if (tid == 0) {
    const unsigned long long xs3 = __builtin_amdgcn_s_memrealtime();
    const unsigned int k = atomicAdd(&g_x3_count, 1u);
    if (k < X3_STAMP_MAX) {
      g_x3_stamp[k][0] = xs0; g_x3_stamp[k][1] = xs1; g_x3_stamp[k][2] = xs2; g_x3_stamp[k][3] = xs3;
      g_x3_stamp[k][4] = ((unsigned long long)nv << 32) | blockIdx.x;
      g_x3_stamp[k][5] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                         (unsigned int)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    }
  }
#endif
}
// L at run time (the SHORT, six-piece and split-K forms, and L = 128 / 256), and L = 16 / 32 / 64 with fixed fragment addresses
template <int ET, bool SHORT = false, bool SPLITK = false, int NP = 5>
__global__ void __launch_bounds__(512, 2) conv3_halo16x3_kernel(ConvGemmParams p) { conv3_halo16x3_body<ET, SHORT, SPLITK, NP, 0>(p); }
template <int ET, int LM>
__global__ void __launch_bounds__(512, 2) conv3_halo16x3_fixed_kernel(ConvGemmParams p) { conv3_halo16x3_body<ET, false, false, 5, LM>(p); }

// =================================================================================================
// conv2d_small_kernel: implicit-GEMM Conv2d for the local-map encoder (bf16), 64 x 64 tiles.
//
// The encoder's GEMMs are small (M = B*OH*OW <= 25 600 rows, N = 64..512 channels, K = live taps x Cin) and,
// on 256 x 256 tiles, leave most CUs idle behind long latency-bound K loops (one work-group per CU, 128 KB of
// LDS, split-K slabs to be reduced afterwards).  Here a work-group is 4 waves on a 64 x 64 tile (one 32 x 32
// accumulator per wave), 3 LDS stages of 16 KB (two K-steps in flight), so 3 work-groups share a CU and
// every layer launches 128..400 of them: latency is hidden by occupancy, no split-K, no slabs.
//   GEMM row m = (b, oh, ow); K-step = (live tap, 64-channel chunk); a tap outside the map reads `zero`.
//   LDS stage: A 64 rows x 128 B + W 64 rows x 128 B, 16-B slots XOR-swizzled on the source address
//   (slot ^ (row >> 1) & 7), staged by LDS-DMA: 16 one-KiB pieces per stage, 4 per wave.
//   Output f32 [M][N] (the GroupNorm kernel follows), rows >= M masked.
// =================================================================================================
//   SPLIT (hi + lo planes, the encoder of the f32-class instantiations): a K-step is 32 channels of a tap, an LDS row is
//   [32 ch hi | the same 32 ch lo] and the step runs A_hi W_lo, A_hi W_hi, A_lo W_hi = 6 MFMAs instead of 4.
template <int ET, bool SPLIT>
__global__ void __launch_bounds__(256) conv2d_small_kernel(ConvGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STAGE = 16384;
  constexpr int CK = SPLIT ? 32 : 64;                                // channels per K-step
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r5 = lane & 31, h = lane >> 5;
  const int wm = w >> 1, wn = w & 1;
  const int ntn = p.N >> 6;
  const int tm = blockIdx.x / ntn, tn = blockIdx.x - tm * ntn;      // N-tiles of one M-block are neighbours (A reuse in L2)
  const int kpt = p.Cin / CK;                                       // K-steps per tap
  const long long K = (long long)p.taps * p.Cin;
  // split-K over blockIdx.y (layers with few tiles and long K): a contiguous range of K-steps per block, partial
  // tiles go to Out + y * slab_stride and are summed, in slab order, by the GroupNorm kernel
  int k0 = 0, nk = p.taps * kpt;
  long long out_extra = 0;
  if (p.splitk > 1) {
    const int per = (nk + p.splitk - 1) / p.splitk;
    k0 = blockIdx.y * per;
    nk = min(nk - k0, per);
    out_extra = (long long)blockIdx.y * p.slab_stride;
  }

  // ---- staging: wave w stages A pieces {2w, 2w+1} (rows 8*piece + (lane >> 3)) and the same W pieces
  const char* a_base[2];
  int ih0[2], iw0[2];
  const char* w_src[2];
  int slot_b[2];
  long long plane_a[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = (2 * w + q) * 8 + (lane >> 3);                     // tile row 0..63
    const int slot = (lane & 7) ^ ((r >> 1) & 7);
    slot_b[q] = SPLIT ? (slot & 3) * 16 : slot * 16;                 // byte offset inside the K-step's channel run
    plane_a[q] = (SPLIT && (slot & 4)) ? p.a_plane : 0;
    const long long plane_w = (SPLIT && (slot & 4)) ? p.w_plane : 0;
    int m = tm * 64 + r;
    m = m < p.M ? m : p.M - 1;
    const int b = m / p.c2_OHW, rem = m - b * p.c2_OHW;
    const int oh = rem / p.c2_OW, ow = rem - oh * p.c2_OW;
    a_base[q] = (const char*)p.A + (long long)b * p.c2_H * p.c2_W * p.Cin * 2;
    ih0[q] = oh * p.c2_stride - p.c2_pad;
    iw0[q] = ow * p.c2_stride - p.c2_pad;
    w_src[q] = (const char*)p.W + (long long)(tn * 64 + r) * (SPLIT ? (long long)p.w_row : K * 2) + slot_b[q] + plane_w;
  }
  auto issue = [&](int kl) {                                         // local K-step kl -> ring slot kl % 3
    const int k = k0 + kl;
    const int tap = k / kpt, kin = k - tap * kpt;
    const int kh = p.c2_kh[tap], kw = p.c2_kw[tap];
    char* st = smem + (kl % 3) * STAGE;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ih = ih0[q] + kh, iw = iw0[q] + kw;
      const bool ok = ih >= 0 && ih < p.c2_H && iw >= 0 && iw < p.c2_W;
      const char* src = ok ? a_base[q] + ((long long)(ih * p.c2_W + iw) * p.Cin + kin * CK) * 2 + plane_a[q] : (const char*)p.zero;
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(src + slot_b[q]), (LDS_AS void*)(st + (2 * w + q) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(w_src[q] + (long long)k * (SPLIT ? p.w_step : 128)),
                                       (LDS_AS void*)(st + 8192 + (2 * w + q) * 1024), 16, 0, 0);
  };

  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  const int a_row = wm * 32 + r5, b_row = wn * 32 + r5;
  const int a_off = a_row * 128, b_off = 8192 + b_row * 128;
  const int sa = (a_row >> 1) & 7, sb = (b_row >> 1) & 7;

  issue(0);
  if (nk > 1) issue(1);
  for (int k = 0; k < nk; ++k) {
    // stage k landed (the 4 pieces of stage k+1 may stay in flight), every wave is done with stage k-1
    if (k + 1 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (k + 2 < nk) issue(k + 2);                                    // into the slot read at step k-1
    const char* st = smem + (k % 3) * STAGE;
    if constexpr (SPLIT) {
      // 16-channel sub-steps 0, 1 = hi plane, 2, 3 = lo plane of the same 32 channels
      short8_t af[4], bf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        af[ks] = *(const short8_t*)(st + a_off + ((((ks << 1) | h) ^ sa) << 4));
        bf[ks] = *(const short8_t*)(st + b_off + ((((ks << 1) | h) ^ sb) << 4));
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) acc = mfma32<ET>(af[kk], bf[kk + 2], acc);       // A_hi x W_lo
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) acc = mfma32<ET>(af[kk], bf[kk], acc);           // A_hi x W_hi
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) acc = mfma32<ET>(af[kk + 2], bf[kk], acc);       // A_lo x W_hi
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const short8_t af = *(const short8_t*)(st + a_off + ((((ks << 1) | h) ^ sa) << 4));
        const short8_t bf = *(const short8_t*)(st + b_off + ((((ks << 1) | h) ^ sb) << 4));
        acc = mfma32<ET>(af, bf, acc);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // this wave's reads of stage k are complete
  }

  // ---- store: acc[i] = C[row (i & 3) + 8 (i >> 2) + 4 h][col r5]
  const int n = tn * 64 + wn * 32 + r5;
  float bias = (p.bias != nullptr && k0 == 0) ? p.bias[n] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m = tm * 64 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (m < p.M) ((float*)p.Out)[out_extra + (long long)m * p.ldc + p.out_coff + n] = (ET == 1 ? acc[i] * p.w_scale : acc[i]) + bias;
  }
}

// =================================================================================================
// gemm16_kernel: the other dense bf16 layers of the U-Net on the halo kernel's machinery -- stride-2 down
// convs, the two 2-tap halves of a transposed conv, 1x1 residual convs, the first conv (K padded to 64) and the
// batched FiLM linears.  Same tile, wave and fragment geometry, 16x16x32 MFMAs in snake order, four 16-MFMA phases per
// K-step with the next phase's ds_reads issued first, epilogue16; what differs is the K walk: K-step k = (tap k / nc,
// 64-channel chunk k % nc) stages BOTH a 256-row activation tile and a 256-row weight tile (2 x 32 KB each,
// double-buffered), two K-steps in flight, one barrier per K-step with a plain vmcnt(0).
//   Activation row of tile row m = (b, l):  b*in_Lp + l*in_stride + in_off + tap.  An 8-row staging piece covers whole
//   samples or lies inside one (L = 4, or 8 | L), so its source offset is wave-uniform + 8 lane-dependent rows: two lane
//   offsets (the XOR swizzle depends on the piece parity) + scalar offsets, as for the weights.  L = 8 and 4 are the ant
//   config's lower levels.
// =================================================================================================
template <int ET, bool SPLIT, bool SHORT = false>
__global__ void __launch_bounds__(512, 2) gemm16_kernel(ConvGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BUF = 32768, W_BASE = 2 * BUF;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r4 = lane & 15, h4 = lane >> 4;
  const int wm = w >> 1, wn = w & 1;
  const int ntn = p.N >> 8, ntm = p.M >> 8;
  const int tile = xcd_remap_strips(blockIdx.x, ntm, ntn, p.xcd_strips);
  const int tm = tile / ntn, tn = tile - tm * ntn;
  // SPLIT (hi + lo planes): a K-step is 32 channels of one tap, an LDS row holds [32 ch hi | the same 32 ch lo] (slots
  // 0..3 / 4..7, chosen by the per-lane source offset) and the step runs the three products A_hi W_lo, A_hi W_hi, A_lo W_hi
  // = 96 MFMAs on it (conv3_halo16x3_kernel explains the scheme)
  constexpr int KB = SPLIT ? 64 : 128;                               // bytes of K per plane and K-step
  const int nc = SPLIT ? (p.Cin >> 5) : (p.Cin >> 6), nk = p.taps * nc;
  const unsigned a_plane = (unsigned)p.a_plane, w_plane = (unsigned)p.w_plane;
  const long long K = (long long)p.taps * p.Cin;

  // buffer descriptors based at the TILE's first activation row / weight row: the 32-bit offsets below then only span the
  // tile (a few MB) plus, for the split formats, the distance to the lo plane (< 2 GiB, checked on the host)
  long long a_tile0;
  {
    const int m0 = tm * 256;
    const int b0 = m0 / p.L, l0 = m0 - b0 * p.L;
    a_tile0 = (((long long)b0 * p.in_Lp + (long long)l0 * p.in_stride + p.in_off) * p.lda) * 2;
  }
  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.A + a_tile0), 0, 0x7fffffff, 0x00020000);
  // weights (denoise.h): split rows are w_row bytes, their 32-channel chunks w_step apart, a chunk's lo half w_plane behind hi
  const long long w_row = SPLIT ? (long long)p.w_row : K * 2;
  const int w_step = SPLIT ? p.w_step : 128;
  const __amdgpu_buffer_rsrc_t w_rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.W + ((long long)tn * 256) * w_row), 0, 0x7fffffff, 0x00020000);
  unsigned pae, pao, pbe, pbo;
  int aq[4], wq[4];
  {
    const int lr = lane >> 3;
    const int slot0 = (lane & 7) ^ (lr >> 1), slot1 = slot0 ^ 4;     // piece parity 0 / 1: (r >> 1) & 7 = (lr >> 1) (+ 4)
    // activation row of piece row lr, relative to the piece's first row: L >= 8 keeps the piece inside a sample, L = 4
    // puts its second half into the next sample (in_Lp rows further)
    const int lrb = lr / p.L, lro = lrb * p.in_Lp + (lr - lrb * p.L) * p.in_stride;
    if constexpr (SPLIT) {
      pae = (unsigned)((lro * p.lda + (slot0 & 3) * 8) * 2) + ((slot0 & 4) ? a_plane : 0u);
      pao = (unsigned)((lro * p.lda + (slot1 & 3) * 8) * 2) + ((slot1 & 4) ? a_plane : 0u);
      pbe = (unsigned)((long long)(8 * lr) * w_row + (slot0 & 3) * 16) + ((slot0 & 4) ? w_plane : 0u);
      pbo = (unsigned)((long long)(8 * lr) * w_row + (slot1 & 3) * 16) + ((slot1 & 4) ? w_plane : 0u);
    } else {
      pae = (unsigned)((lro * p.lda + slot0 * 8) * 2);
      pao = (unsigned)((lro * p.lda + slot1 * 8) * 2);
      pbe = (unsigned)(((long long)(8 * lr) * K + slot0 * 8) * 2);
      pbo = (unsigned)(((long long)(8 * lr) * K + slot1 * 8) * 2);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r0 = (w * 4 + q) * 8;                                // tile row of the piece's first lane row
      const int m = tm * 256 + r0;
      const int b = m / p.L, l = m - b * p.L;
      aq[q] = (int)((((long long)b * p.in_Lp + (long long)l * p.in_stride + p.in_off) * p.lda) * 2 - a_tile0);
      const int cu = (r0 & 128) + 8 * (r0 & 8) + ((r0 >> 4) & 7);    // W: LDS row wn*128 + j*16 + r4 <- channel wn*128 + 8*r4 + j
      wq[q] = (int)((long long)cu * w_row);
    }
  }
  const int tap_bytes = p.lda * 2;                                   // one activation row further per tap
  // scalar source offsets of (virtual) K-step kv: activations / weights
  auto src_off = [&](int k, int& ao, int& wo) {
    // (both are wave-uniform, but the compiler keeps the split forms' weight offset in a VGPR and then wraps every LDS-DMA
    // request that takes it as its scalar offset in a waterfall loop: four per K-step.  readfirstlane pins them to SGPRs)
    const int t = k / nc, c = k - t * nc;
    ao = __builtin_amdgcn_readfirstlane(t * tap_bytes + c * KB);
    wo = __builtin_amdgcn_readfirstlane(k * w_step);
  };
  auto issue = [&](int kv) {                                         // K-step kv -> buffers kv & 1
    int ao, wo;
    src_off(kv, ao, wo);
    char* ab = smem + (kv & 1) * BUF;
    char* wb = smem + W_BASE + (kv & 1) * BUF;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (LDS_AS void*)(ab + (w * 4 + q) * 1024), 16, (q & 1) ? pao : pae,
                                               aq[q] + ao, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (LDS_AS void*)(wb + (w * 4 + q) * 1024), 16, (q & 1) ? pbo : pbe,
                                               wq[q] + wo, 0, 0);
  };

  // split formats: the weight pieces of a step go out in the first two phases of the step BEFORE it (two each) instead of
  // with the activation pieces behind the barrier: eight requests per wave in one burst fill the address FIFO (see
  // conv3_halo16x3_kernel); -2 % on these launches
  auto issue_wq = [&](int kv, int q) {                               // one weight piece of K-step kv
    int ao, wo;
    src_off(kv, ao, wo);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (LDS_AS void*)(smem + W_BASE + (kv & 1) * BUF + (w * 4 + q) * 1024), 16,
                                             (q & 1) ? pbo : pbe, wq[q] + wo, 0, 0);
  };
  const int a_row = wm * 64 + r4;                                    // + 16 mb
  const int swa = (a_row >> 1) & 7;                                  // (a_row + 16 mb) >> 1 & 7 is the same for every mb
  const int a_off = a_row * 128, b_off = (wn * 128 + r4) * 128;
  const int swb = (r4 >> 1) & 7;

  f32x4_t acc[4][8];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[mb][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  short8_t af[2][4], bq[2][4];
  auto rdA = [&](int set, int k, int ks) {
    const char* ab = smem + (k & 1) * BUF + a_off + ((((ks << 2) | h4) ^ swa) << 4);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) af[set][mb] = *(const short8_t*)(ab + mb * 2048);
  };
  auto rdB = [&](int set, int k, int ks, int half) {
    const char* wb = smem + W_BASE + (k & 1) * BUF + b_off + half * 8192 + ((((ks << 2) | h4) ^ swb) << 4);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) bq[set][jj] = *(const short8_t*)(wb + jj * 2048);
  };
  auto mm = [&](int aset, int bset, int half, int mb, int jj) {
    acc[mb][half * 4 + jj] = mfma16<ET>(af[aset][mb], bq[bset][jj], acc[mb][half * 4 + jj]);
  };
  // (not mm16_snake: through the shared helper the non-split instantiations of this kernel come out with other code)
  auto mm16 = [&](int aset, int bset, int half) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) mm(aset, bset, half, mb, (mb & 1) ? 3 - jj : jj);
  };
  // One K-step.  On entry af[0] = A(ks 0), bq[0] = B(ks 0, half 0) of step k  (SPLIT: af[0] = A_hi, bq[0] = W_lo(half 0)).
  auto step = [&](auto tNext, auto tIssue, int k) {
    constexpr bool HAS_NEXT = decltype(tNext)::value, ISSUE = decltype(tIssue)::value;
    if constexpr (SPLIT) {
      rdB(1, k, 1, 1);                  // P1: A_hi x W_lo(0); fetch W_lo(1)
      mm16(0, 0, 0);
      if constexpr (HAS_NEXT) {
        issue_wq(k + 1, 0); issue_wq(k + 1, 1);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      } else
      {
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      rdB(0, k, 0, 0);                  // P2: A_hi x W_lo(1); fetch W_hi(0) and A_lo
      rdA(1, k, 1);
      mm16(0, 1, 1);
      if constexpr (HAS_NEXT) {
        issue_wq(k + 1, 2); issue_wq(k + 1, 3);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      } else
      {
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      rdB(1, k, 0, 1);                  // P3: A_hi x W_hi(0); fetch W_hi(1)
      mm16(0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      __builtin_amdgcn_sched_barrier(0);
      mm16(1, 0, 0);                    // P4: A_lo x W_hi(0)
      __builtin_amdgcn_sched_barrier(0);
      mm16(0, 1, 1);                    // P5: A_hi x W_hi(1)
      __builtin_amdgcn_sched_barrier(0);
    } else {
      rdB(1, k, 0, 1);                  // phase (0,0)
      mm16(0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      __builtin_amdgcn_sched_barrier(0);
      rdA(1, k, 1);                     // phase (0,1)
      rdB(0, k, 1, 0);
      mm16(0, 1, 1);
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      __builtin_amdgcn_sched_barrier(0);
      rdB(1, k, 1, 1);                  // phase (1,0)
      mm16(1, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    int ao2 = 0, wo2 = 0;
    if constexpr (ISSUE) src_off(k + 2, ao2, wo2);
    if constexpr (HAS_NEXT) {
      // stage k+1 (requested one K-step ago) has landed; every wave is done reading stage k
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      rdA(0, k + 1, 0);
      rdB(0, k + 1, SPLIT ? 1 : 0, 0);
    }
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)      // phase (1,1) + the LDS-DMA pieces of step k+2 into the buffers just released (split: activations only)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        mm(1, 1, 1, mb, (mb & 1) ? 3 - jj : jj);
        if constexpr (ISSUE) {
          // one LDS-DMA issue behind every second MFMA (see conv3_halo16_kernel)
          const int m = mb * 4 + jj, i = (m & 1) ? -1 : (m >> 1);
          if (i >= 0 && i < 4)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (LDS_AS void*)(smem + (k & 1) * BUF + (w * 4 + i) * 1024), 16,
                                                     (i & 1) ? pao : pae, aq[i] + ao2, 0, 0);
          else if (!SPLIT && i >= 4 && i < 8)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (LDS_AS void*)(smem + W_BASE + (k & 1) * BUF + (w * 4 + i - 4) * 1024),
                                                     16, ((i - 4) & 1) ? pbo : pbe, wq[i - 4] + wo2, 0, 0);
        }
      }
    if constexpr (HAS_NEXT) __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      if (ISSUE && !(i & 1) && (!SPLIT || i < 8)) __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using Tt = std::true_type;
  using Ff = std::false_type;

  issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (nk > 1) {
    if constexpr (SPLIT) {             // A(1) only: W(1) goes out in the first phases of step 0
      int ao, wo;
      src_off(1, ao, wo);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (LDS_AS void*)(smem + BUF + (w * 4 + q) * 1024), 16, (q & 1) ? pao : pae,
                                                 aq[q] + ao, 0, 0);
    } else {
      issue(1);
    }
  }
  rdA(0, 0, 0);
  rdB(0, 0, SPLIT ? 1 : 0, 0);
  for (int k = 0; k < nk - 2; ++k) step(Tt{}, Tt{}, k);
  if (nk >= 2) step(Tt{}, Ff{}, nk - 2);
  step(Ff{}, Ff{}, nk - 1);
  __syncthreads();
  gemm_epilogue16<ET, SPLIT, SHORT>(p, acc, smem, tm, tn, tid, lane, r4, h4, wm, wn);
}
// ---- dispatch ---------------------------------------------------------------------------------
// fmt = storage type | split << 2 (denoise.h).  The 16-bit tiles (halo, gemm16, small Conv2d) exist for bf16 and f16;
// the hi/lo split forms only on the halo / gemm16 / small-Conv2d tiles; f32 runs everything on conv_gemm_kernel<1>.
//
// Every tile kernel instantiation, once: the picker finds its entry here, the launcher takes kernel, LDS size and block from
// it, and the LDS attribute is set from the same rows.
enum { TILE_HALO, TILE_GEMM16, TILE_C2D_SMALL, TILE_GENERIC };
enum { TV_SPLIT = 1,     // hi + lo planes
       TV_SHORT = 2,     // L = 8 / 4: per-lane sample indices in the epilogue
       TV_SPLITK = 4,    // latency mode of the split halo kernel: gridDim.y work-groups per tile
       TV_NP6 = 8,       // L = 4 on the split halo kernel: six activation pieces, all 160 KB of LDS
       TV_C2D = 16,      // implicit Conv2d addressing
       TV_L16 = 32, TV_L32 = 64, TV_L64 = 128 };   // whole-tile halo forms at L = 16, 32, 64: fixed fragment addresses
struct TileVariant {
  void (*kernel)(ConvGemmParams);
  unsigned lds_bytes;    // dynamic LDS of a work-group
  unsigned block;        // threads per work-group
  int family, st;        // TILE_*, storage type ST_*
  unsigned flags;        // TV_*
  int kind;              // what conv_gemm_kind reports: 0 halo kernel, 1 gemm16 / generic, 2 implicit Conv2d
};
static const TileVariant k_tiles[] = {
    {conv3_halo16_kernel<0>, 147456, 512, TILE_HALO, ST_BF16, 0, 0},
    {conv3_halo16_kernel<1>, 147456, 512, TILE_HALO, ST_F16, 0, 0},
    {conv3_halo16x3_kernel<0>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT, 0},
    {conv3_halo16x3_kernel<1>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT, 0},
    {conv3_halo16_fixed_kernel<0, 16>, 147456, 512, TILE_HALO, ST_BF16, TV_L16, 0},
    {conv3_halo16_fixed_kernel<1, 16>, 147456, 512, TILE_HALO, ST_F16, TV_L16, 0},
    {conv3_halo16_fixed_kernel<0, 32>, 147456, 512, TILE_HALO, ST_BF16, TV_L32, 0},
    {conv3_halo16_fixed_kernel<1, 32>, 147456, 512, TILE_HALO, ST_F16, TV_L32, 0},
    {conv3_halo16_fixed_kernel<0, 64>, 147456, 512, TILE_HALO, ST_BF16, TV_L64, 0},
    {conv3_halo16_fixed_kernel<1, 64>, 147456, 512, TILE_HALO, ST_F16, TV_L64, 0},
    {conv3_halo16x3_fixed_kernel<0, 16>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_L16, 0},
    {conv3_halo16x3_fixed_kernel<1, 16>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_L16, 0},
    {conv3_halo16x3_fixed_kernel<0, 32>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_L32, 0},
    {conv3_halo16x3_fixed_kernel<1, 32>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_L32, 0},
    {conv3_halo16x3_fixed_kernel<0, 64>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_L64, 0},
    {conv3_halo16x3_fixed_kernel<1, 64>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_L64, 0},
    {conv3_halo16x3_kernel<0, true>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_SHORT, 0},
    {conv3_halo16x3_kernel<1, true>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_SHORT, 0},
    {conv3_halo16x3_kernel<0, false, true>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_SPLITK, 0},
    {conv3_halo16x3_kernel<1, false, true>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_SPLITK, 0},
    {conv3_halo16x3_kernel<0, true, true>, 147456, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_SHORT | TV_SPLITK, 0},
    {conv3_halo16x3_kernel<1, true, true>, 147456, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_SHORT | TV_SPLITK, 0},
    {conv3_halo16x3_kernel<0, true, false, 6>, 163840, 512, TILE_HALO, ST_BF16, TV_SPLIT | TV_SHORT | TV_NP6, 0},
    {conv3_halo16x3_kernel<1, true, false, 6>, 163840, 512, TILE_HALO, ST_F16, TV_SPLIT | TV_SHORT | TV_NP6, 0},
    {gemm16_kernel<0, false>, 131072, 512, TILE_GEMM16, ST_BF16, 0, 1},
    {gemm16_kernel<1, false>, 131072, 512, TILE_GEMM16, ST_F16, 0, 1},
    {gemm16_kernel<0, true>, 131072, 512, TILE_GEMM16, ST_BF16, TV_SPLIT, 1},
    {gemm16_kernel<1, true>, 131072, 512, TILE_GEMM16, ST_F16, TV_SPLIT, 1},
    {gemm16_kernel<0, false, true>, 131072, 512, TILE_GEMM16, ST_BF16, TV_SHORT, 1},
    {gemm16_kernel<1, false, true>, 131072, 512, TILE_GEMM16, ST_F16, TV_SHORT, 1},
    {gemm16_kernel<0, true, true>, 131072, 512, TILE_GEMM16, ST_BF16, TV_SPLIT | TV_SHORT, 1},
    {gemm16_kernel<1, true, true>, 131072, 512, TILE_GEMM16, ST_F16, TV_SPLIT | TV_SHORT, 1},
    {conv2d_small_kernel<0, false>, 3 * 16384, 256, TILE_C2D_SMALL, ST_BF16, TV_C2D, 2},
    {conv2d_small_kernel<1, false>, 3 * 16384, 256, TILE_C2D_SMALL, ST_F16, TV_C2D, 2},
    {conv2d_small_kernel<0, true>, 3 * 16384, 256, TILE_C2D_SMALL, ST_BF16, TV_C2D | TV_SPLIT, 2},
    {conv2d_small_kernel<1, true>, 3 * 16384, 256, TILE_C2D_SMALL, ST_F16, TV_C2D | TV_SPLIT, 2},
    {conv_gemm_kernel<0, false>, 131072, 512, TILE_GENERIC, ST_BF16, 0, 1},
    {conv_gemm_kernel<1, false>, 131072, 512, TILE_GENERIC, ST_F32, 0, 1},
    {conv_gemm_kernel<2, false>, 131072, 512, TILE_GENERIC, ST_F16, 0, 1},
    {conv_gemm_kernel<0, true>, 131072, 512, TILE_GENERIC, ST_BF16, TV_C2D, 2},
    {conv_gemm_kernel<1, true>, 131072, 512, TILE_GENERIC, ST_F32, TV_C2D, 2},
    {conv_gemm_kernel<2, true>, 131072, 512, TILE_GENERIC, ST_F16, TV_C2D, 2},
};
// (pick_tile only asks for keys that have a row above; a key without one counts as "no tile fits")
static const TileVariant* find_tile(int family, int st, unsigned flags) {
  for (const TileVariant& v : k_tiles)
    if (v.family == family && v.st == st && v.flags == flags) return &v;
  return nullptr;
}

// The tile a GEMM runs on, or null where none fits (split formats only: the other formats fall back to conv_gemm_kernel).
// The eligibility rules live here and nowhere else.
static const TileVariant* pick_tile(const ConvGemmParams& p, int fmt) {
  const int st = fmt_st(fmt);
  const bool split = fmt_split(fmt);
  const unsigned fsplit = split ? TV_SPLIT : 0;
  const bool tile16 = st != ST_F32 && !p.c2d && (p.M & 255) == 0 && (p.N & 255) == 0 && (p.Cin & 63) == 0;
  // halo tile.  L = 8 (the ant network's middle level, split formats): a tile's 32 samples x 10 padded rows are exactly the 320
  // rows the five staging pieces hold; the fragment rows are per-lane offsets already (lrow0), the epilogue is the SHORT
  // instantiation.  L = 4: 64 samples x 6 padded rows = 384 staged rows, the six-piece instantiation (no split-K form).
  const bool l_ok = p.L >= 16 || (p.L == 8 && split) || (p.L == 4 && split && p.splitk <= 1);
  if (tile16 && p.taps == 3 && p.in_stride == 1 && p.in_Lp == p.L + 2 && (256 % p.L) == 0 && l_ok && p.Cin >= 192) {
    const unsigned flen = p.L == 64 ? TV_L64 : (p.L == 32 ? TV_L32 : (p.L == 16 ? TV_L16 : 0));     // L = 128 / 256: run-time form
    if (!split) return find_tile(TILE_HALO, st, flen);
    const unsigned fshort = p.L <= 8 ? TV_SHORT : 0;
    if (p.splitk > 1) return find_tile(TILE_HALO, st, TV_SPLIT | fshort | TV_SPLITK);   // latency mode (denoise.h)
    if (p.L >= 16) return find_tile(TILE_HALO, st, TV_SPLIT | flen);
    return find_tile(TILE_HALO, st, TV_SPLIT | TV_SHORT | (p.L == 4 ? TV_NP6 : 0));
  }
  // gemm16 tile.  L = 8 and 4 (the ant config's lower levels): a 16-row block of the epilogue spans 2 or 4 samples
  const bool short_l = p.L == 8 || p.L == 4;
  if (tile16 && (!p.out_f32 || p.mode == MODE_BIAS) && p.taps >= 1 && p.taps <= 3 && ((p.L & 15) == 0 || short_l) && p.M > 0 &&
      (p.mode == MODE_BIAS || (256 % p.L) == 0))
    return find_tile(TILE_GEMM16, st, fsplit | ((p.L & 15) != 0 ? TV_SHORT : 0));
  if (p.c2d && conv2d_small_eligible(fmt) && (p.N & 63) == 0 && (p.Cin & 63) == 0 && p.out_f32 && p.mode == MODE_BIAS)
    return find_tile(TILE_C2D_SMALL, st, TV_C2D | fsplit);
  if (split) return nullptr;
  return find_tile(TILE_GENERIC, st, p.c2d ? TV_C2D : 0);
}
bool conv2d_small_eligible(int fmt) { return fmt_st(fmt) != ST_F32; }
int conv_gemm_kind(const ConvGemmParams& p, int fmt) {
  const TileVariant* v = pick_tile(p, fmt);
  return v != nullptr ? v->kind : (p.c2d ? 2 : 1);
}
bool conv_gemm_supported(const ConvGemmParams& p, int fmt) { return pick_tile(p, fmt) != nullptr; }

// > 64 KB of dynamic LDS needs the attribute once per kernel AND per device
static void ensure_lds_attrs() {
  static bool done[64] = {};
  int dev = 0;
  hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || done[dev]) return;
  done[dev] = true;
  for (const TileVariant& v : k_tiles)
    if (v.lds_bytes > 65536) hipFuncSetAttribute((const void*)v.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds_bytes);
}

void launch_conv_gemm(const ConvGemmParams& p, int fmt, hipStream_t s) {
  ensure_lds_attrs();
  const TileVariant* v = pick_tile(p, fmt);
  if (v != nullptr && (v->flags & TV_SPLITK) &&
      (p.sk_ws == nullptr || p.sk_cnt == nullptr || ((p.Cin >> 5) % p.splitk) != 0 || (p.Cin >> 5) / p.splitk < 2))
    throw std::runtime_error("conv_gemm: split-K of the halo kernel needs its workspace and splitk | Cin / 32, >= 2 chunks each");
  if ((v == nullptr || v->family == TILE_GENERIC) && p.mode >= MODE_GN_MISH && (p.L & 15) != 0)
    throw std::runtime_error("conv_gemm: a fused GroupNorm epilogue at L = 8 / 4 exists on the gemm16 tile only (whole 256-row tiles)");
  if (v == nullptr) throw std::runtime_error("conv_gemm: a split GEMM of this shape fits no tile (conv_gemm_supported is the contract)");
  // 256 x 256 tiles, 64 x 64 on the small Conv2d kernel; gridDim.y = split-K work-groups where the variant has a split-K form
  dim3 grid(((p.M + 255) >> 8) * ((p.N + 255) >> 8));
  if (v->family == TILE_C2D_SMALL) grid.x = ((p.M + 63) >> 6) * (p.N >> 6);
  if (v->flags & (TV_SPLITK | TV_C2D)) grid.y = p.splitk > 1 ? p.splitk : 1;
  DN_LAUNCH(v->kernel, grid, dim3(v->block), v->lds_bytes, s, p);
}
