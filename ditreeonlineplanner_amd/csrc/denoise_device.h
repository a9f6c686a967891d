// Device helpers shared by the denoiser's kernel units (conv_tiles.hip, denoise_small_kernels.hip): vector types, number
// format conversions, the f16 range guard, MFMA wrappers, Mish, the XCD tile remap, element load / store and the launch macro.
#pragma once
#include <stdexcept>

#include "denoise.h"

// Plan validation (DenoiserState::build): every launcher runs its dispatch and shape contracts, but enqueues nothing while the
// dry-run flag is set -- an unsupported layer shape fails at reserve time, and the validation leaves no launches in a profile.
#define DN_LAUNCH(...) do { if (!denoise_dry_run()) hipLaunchKernelGGL(__VA_ARGS__); } while (0)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 half8_t;
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 half2_t;
typedef __attribute__((ext_vector_type(2))) short short2_t;

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

__device__ __forceinline__ unsigned short f2bf(float f) {
  __bf16 b = (__bf16)f;                       // v_cvt_pk_bf16_f32: RNE, NaN preserved
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short u) {
  unsigned int x = ((unsigned int)u) << 16;
  return __builtin_bit_cast(float, x);
}
__device__ __forceinline__ unsigned short f2h(float f) {
  // f16 has no headroom above 65504: saturate instead of producing inf (a NaN stays a NaN through v_med3)
  _Float16 b = (_Float16)__builtin_amdgcn_fmed3f(f, -65504.0f, 65504.0f);
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float h2f(unsigned short u) { return (float)__builtin_bit_cast(_Float16, u); }
// f16 range guard.  The f16 instantiations saturate at +-65504 silently (v_med3 above / in the epilogues); so that a
// checkpoint whose activations leave the f16 range is REPORTED instead of returning wrong actions with rc 0, every thread
// that converts values to f16 keeps the largest magnitude it was handed (one v_max3_f32 with |.| source modifiers per two
// values; a NaN drops out of the maximum, an infinity does not) and ORs 1 into the launch's flag word when it exceeds the
// range.  The flag of each layer is read by ditree_denoise_status (denoise_host.hip).
__device__ __forceinline__ void sat_see2(float& m, float a, float b) {
  m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(a)), __builtin_fabsf(b));
}
__device__ __forceinline__ void sat_see(float& m, float a) { m = __builtin_fmaxf(m, __builtin_fabsf(a)); }
__device__ __forceinline__ void sat_flush(int* flag, float m) {
  if (flag != nullptr && m > 65504.0f) atomicOr(flag, 1);
}
// The MFMA epilogues have no VGPR to spare for a running maximum (256 of 256 in use: carrying one spilled 70 registers,
// and so did carrying the wave's compare mask): there the maximum of a ROW is formed in a transient register, compared once,
// and the flag is written right away behind a wave-uniform branch that is never taken in a healthy network.
__device__ __forceinline__ void sat_check_row(int* flag, const float (&v)[8]) {
#ifdef DITREE_NO_RANGE_GUARD      // measurement build only: what the guard costs in the MFMA epilogues
  return;
#endif
  float t = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), __builtin_fabsf(v[2]));
  t = __builtin_fmaxf(__builtin_fmaxf(t, __builtin_fabsf(v[3])), __builtin_fabsf(v[4]));
  t = __builtin_fmaxf(__builtin_fmaxf(t, __builtin_fabsf(v[5])), __builtin_fabsf(v[6]));
  t = __builtin_fmaxf(t, __builtin_fabsf(v[7]));
  if (__builtin_amdgcn_ballot_w64(t > 65504.0f) != 0ull) {
    if (flag != nullptr && t > 65504.0f) atomicOr(flag, 1);
  }
}
// 16-bit element types of the MFMA operands.  ET 0: bf16 (8 significand bits, f32 range), ET 1: f16 (11 bits, +-65504).
// SPLIT instantiations carry every operand as two 16-bit planes hi + lo (lo = rnd(x - hi)) and form a product from
// three MFMAs hi*hi + hi*lo + lo*hi with f32 accumulation: 16 (bf16) / 22 (f16) significand bits per operand at a
// third of the 16-bit MFMA rate -- the f32-input MFMA runs at a sixteenth of it (MI355X_MICROARCH.md, Matrix cores).
template <int ET> __device__ __forceinline__ unsigned short f2e(float f) { if constexpr (ET == 0) return f2bf(f); else return f2h(f); }
template <int ET> __device__ __forceinline__ float e2f(unsigned short u) { if constexpr (ET == 0) return bf2f(u); else return h2f(u); }
template <int ET>
__device__ __forceinline__ f32x4_t mfma16(const short8_t& a, const short8_t& b, const f32x4_t& c) {
  if constexpr (ET == 0)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}
template <int ET>
__device__ __forceinline__ f32x16_t mfma32(const short8_t& a, const short8_t& b, const f32x16_t& c) {
  if constexpr (ET == 0)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}

template <int PREC>
__device__ __forceinline__ float mish_f(float x) {
  // x * tanh(softplus(x)) = x * w / (w + 2), w = e^x (e^x + 2)
  if constexpr (PREC == 0) {
    // throughput path: x - 2x / (n (n + 2) + 2); n = inf (x > 88) gives rcp = 0 -> x, n = 0 gives 0,
    // so torch's softplus threshold needs no branch.  5 VALU + exp + rcp.
    const float n = __expf(x);
    const float d = fmaf(n, n + 2.0f, 2.0f);
    return fmaf(-2.0f * x, __builtin_amdgcn_rcpf(d), x);
  } else {
    if (x > 20.0f) return x;                       // softplus threshold as torch
    const float n = expf(x);
    const float w = n * (n + 2.0f);
    return x * (w / (w + 2.0f));
  }
}

// the same on a pair of values (two tile rows of one channel: adjacent accumulator registers, so the packed f32
// instructions v_pk_fma / v_pk_mul / v_pk_add take them without register shuffles).  PREC 0: throughput, 2: f32-class.
template <int PREC>
__device__ __forceinline__ f32x2_t mish2(f32x2_t x) {
  if constexpr (PREC == 0) {
    const f32x2_t n = {__expf(x[0]), __expf(x[1])};
    const f32x2_t d = __builtin_elementwise_fma(n, n + 2.0f, f32x2_t{2.0f, 2.0f});
    const f32x2_t q = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    return __builtin_elementwise_fma(-2.0f * x, q, x);
  } else {
    // f32-class at a third of the instructions of expf + IEEE division (the epilogue of the split kernels is VALU-bound):
    // e^x = 2^t * (1 + r ln 2) with t = rnd(x log2 e) and r its exact residual (fma) plus the low part of the constant,
    // 2^t by v_exp_f32 (1 ulp); 1 / (w + 2) by v_rcp_f32 and one Newton step.  Relative error ~1e-7, no branch.
    const float L2E = 1.44269502162933349609375f, L2E_LO = 1.92596299112661746e-08f, LN2 = 0.693147182464599609375f;
    // exponent of min(x, 20): above torch's softplus threshold w / (w + 2) rounds to 1 and x comes back (no select)
    const f32x2_t xm = {__builtin_fminf(x[0], 20.0f), __builtin_fminf(x[1], 20.0f)};
    const f32x2_t l2e = {L2E, L2E};
    const f32x2_t t = xm * l2e;
    f32x2_t r = __builtin_elementwise_fma(xm, l2e, -t);
    r = __builtin_elementwise_fma(xm, f32x2_t{L2E_LO, L2E_LO}, r);
    const f32x2_t e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    const f32x2_t n = __builtin_elementwise_fma(e, r * LN2, e);
    const f32x2_t w = n * (n + 2.0f);
    const f32x2_t d = w + 2.0f;
    f32x2_t q = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    q = __builtin_elementwise_fma(__builtin_elementwise_fma(-d, q, f32x2_t{1.0f, 1.0f}), q, q);
    return x * (w * q);
  }
}

// s + s of the lane that the row-local DPP control CTRL selects (a VALU add with a DPP operand: no LDS round trip)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float s) {
  return s + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), CTRL, 0xf, 0xf, true));
}

// bijective XCD-aware tile remap (blocks b and b+8 share an XCD): each XCD gets a
// contiguous range of tiles, so concurrently resident tiles share A / W panels in L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  int q = nwg >> 3, r = nwg & 7, x = bid & 7, k = bid >> 3;
  int start = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return start + k;
}
// The same with the walk INSIDE an XCD's range shaped for its L2: the 32 work-groups an XCD runs at a time (one per CU) stream
// the A panels of their tile rows and the W panels of their tile columns together.  With 8 tile columns (C_out = 2048, W panel
// 6.3 MB, A panel 2.1 MB at K = 6144) a group of 4 rows x 8 columns pulls 4 A + 8 W panels = 59 MB through the L2, a group of
// 8 rows x 4 columns 8 A + 4 W = 42 MB: the range is walked in strips of four tile columns.  (Needs whole tile rows per XCD;
// anything else keeps the plain order, and so does strips = 0.)
__device__ __forceinline__ int xcd_remap_strips(int bid, int ntm, int ntn, int strips) {
  const int nwg = ntm * ntn;
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7, k = bid >> 3;
  const int start = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  if (strips && r == 0 && ntn >= 8 && (ntn & 3) == 0 && (q % ntn) == 0) {
    const int per = (q / ntn) * 4, strip = k / per, kk = k - strip * per;
    return start + (kk >> 2) * ntn + strip * 4 + (kk & 3);
  }
  return start + k;
}

// FMT = storage type | split << 2 (denoise.h).  `plane` = bytes from the hi plane to the lo plane of a split buffer.
template <int FMT>
__device__ __forceinline__ void store_elem(void* base, long long idx, float v, long long plane = 0) {
  constexpr int ST = FMT & 3;
  if constexpr (ST == ST_F32) {
    ((float*)base)[idx] = v;
  } else {
    constexpr int ET = ST == ST_F16 ? 1 : 0;
    const unsigned short hi = f2e<ET>(v);
    ((unsigned short*)base)[idx] = hi;
    if constexpr ((FMT & 4) != 0) ((unsigned short*)((char*)base + plane))[idx] = f2e<ET>(v - e2f<ET>(hi));
  }
}
// the same, feeding the f16 range guard of the calling thread
template <int FMT>
__device__ __forceinline__ void store_elem(void* base, long long idx, float v, long long plane, float& satm) {
  if constexpr ((FMT & 3) == ST_F16) sat_see(satm, v);
  store_elem<FMT>(base, idx, v, plane);
}
template <int FMT>
__device__ __forceinline__ float load_elem(const void* base, long long idx, long long plane = 0) {
  constexpr int ST = FMT & 3;
  if constexpr (ST == ST_F32) {
    return ((const float*)base)[idx];
  } else {
    constexpr int ET = ST == ST_F16 ? 1 : 0;
    float v = e2f<ET>(((const unsigned short*)base)[idx]);
    if constexpr ((FMT & 4) != 0) v += e2f<ET>(((const unsigned short*)((const char*)base + plane))[idx]);
    return v;
  }
}
// exact Mish for the f32 and the split (f32-class) formats, the fast form for plain 16-bit storage
#define MISH_OF(FMT) mish_f<((FMT) == ST_BF16 || (FMT) == ST_F16) ? 0 : 1>
// run CALL(FMT) with FMT a compile-time constant
#define DISPATCH_FMT(fmt, CALL)                                   \
  switch (fmt) {                                                  \
    case 0: CALL(0); break;                                       \
    case 1: CALL(1); break;                                       \
    case 2: CALL(2); break;                                       \
    case 4: CALL(4); break;                                       \
    case 6: CALL(6); break;                                       \
    default: throw std::runtime_error("denoiser kernels: unknown activation format"); \
  }
