// MPPI controller, one step as separate launches (gfx950, FP64), on the car model (ditree_mppi_step) and on the higher-DoF
// rollout slot (ditree_mppi_step_ant, BASELINE config 5 as written -- "MPPI antmaze, 65 536 rollouts"): K x T rollouts, costs,
// soft-min weights, control update, one executed step -- the controller `run_scenarios_with_lidar_MPPI.py:10,339-449` imports
// as MPPI.mppi.MPPI.  The reference repository contains NEITHER that module NOR the ant's physics (MuJoCo
// through gymnasium-robotics): cost function, sampling scheme and update rule are this build's own (information-theoretic MPPI,
// Williams et al. 2017), on the reference's car dynamics / collision / goal functions or on the build's stand-in crawler model
// (ant_device.h) with the reference's ant collision test (common/map_utils.py:126-219) and goal radius (0.45 * s_global,
// planners/base_planner.py:296-297); stated in DESIGN.md, restated on the CPU in oracle/mppi.py; PARITY WITH THE REFERENCE IS
// UNPINNED by construction.
//
// Compiled with -ffp-contract=off like geom_kernels.hip (same car_device.h functions, bit-exact collision / goal flags).  The
// controller itself is mppi_device.h; this unit holds the two rollout kernels, the ant's model traits, the update pipeline as
// kernels templated on the model, and the one host launcher behind both entry points.
//
//   rollouts   mppi_rollout_kernel<G>: G = 4 adjacent lanes (a DPP quad) share one rollout.  A rollout is a sequential FP64
//              chain (T x [dynamics, two-ball collision, goal test, nearest reference-path point]); 65 536 rollouts on one lane
//              each are 1 024 waves = ONE wave per SIMD, which leaves the chain's latencies exposed (the round-2 finding on
//              car_rollout_kernel).  With four lanes per rollout there are four waves per SIMD (car_rollout<G>, mppi_device.h).
//              mppi_ant_rollout_kernel: one lane per rollout (the 29-d state and the 8-d noise leave no registers to share a
//              rollout between lanes).  Noise is not read from HBM: it is a counter-based hash (splitmix64 -> Box-Muller) of
//              (seed, call counter, rollout, step) that the update kernel regenerates, so a step moves K x 12 bytes (costs,
//              flags) instead of K x T x NU x 8.  A noise tape in HBM can be passed for tests.
//   update     mppi_partial_kernel<Model>: fixed-order partial sums of w_k and w_k eps[k, t, :] over slices of the rollouts;
//              mppi_finish_kernel<Model>: ordered sum of the partials, U += sum / eta, then one executed env step with U[0]
//              and the shift of the nominal sequence.  All sums have a fixed order: results are reproducible.
#include <algorithm>

#include "ant_device.h"
#include "ditree_internal.h"
#include "mppi_device.h"

namespace {

// ---- the ant model: result [64] = action [16..24), the state after EXECUTE [24..53)
struct AntTail {
  double sigma[ANT_D], goal_radius, ball_radius, s_global;
  AntModelArg model;
};

struct AntModel {
  static constexpr int NX = ANT_S, NU = ANT_D;
  static constexpr int ACTION_AT = 16, STATE_AT = 24;
  using Tail = AntTail;
  // eps[k, t, 0..8) ~ N(0, diag(sigma^2)): pair p = 0..3 of (seed, counter, GLOBAL k, t) gives dims 2p, 2p + 1
  static __device__ __forceinline__ void noise(const MppiArgs& a, const AntTail& m, long long k, int t, double* e) {
    unsigned long long h = splitmix64(a.seed ^ splitmix64(a.counter));
    h = splitmix64(h ^ ((unsigned long long)k * 0xD1B54A32D192ED03ull));
    h = splitmix64(h ^ (unsigned long long)t);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned long long h1 = splitmix64(h ^ ((unsigned long long)(p + 1) * 0xA24BAED4963EE407ull));
      const unsigned long long h2 = splitmix64(h1);
      const double u1 = ((double)(h1 >> 11) + 1.0) * (1.0 / 9007199254740992.0);
      const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);
      const double r = sqrt(-2.0 * log(u1));
      const double ang = 6.283185307179586 * u2;
      double sa, ca;
      sincos(ang, &sa, &ca);
      e[2 * p] = m.sigma[2 * p] * (r * ca);
      e[2 * p + 1] = m.sigma[2 * p + 1] * (r * sa);
    }
  }
  // one model step of `s` with the control `u` clipped to the env's action space -> act: 0, 1 = goal radius, 2 = collided
  static __device__ __forceinline__ int env_step(const MppiArgs& a, const AntTail& m, const unsigned char* maze, int rows, int cols,
                                                 double* s, const double* u, double* act) {
    for (int d = 0; d < ANT_D; ++d) act[d] = fmin(fmax(u[d], -1.0), 1.0);
    ant_model_step(s, act, m.model);
    const double ex = s[0] - a.gx, ey = s[1] - a.gy;
    const bool reached = sqrt(fma(ey, ey, ex * ex)) < m.goal_radius;
    return ant_collides(s, maze, rows, cols, m.s_global, m.ball_radius) ? 2 : (reached ? 1 : 0);
  }
};

// ---- rollouts.  Both kernels stage path, controls and maze in LDS, find i0 block-cooperatively, write costs / flags and fold
// beta = min_k S_k into `minkey` without a second pass over the costs: wave minimum, one atomicMin per wave on an
// order-preserving integer image of the double (min is order-independent: reproducible).
struct RolloutLds {
  double2* path;                       // P points
  double* U;                           // T x NU
  double* red;                         // 2 x 4 (block argmin)
  unsigned char* maze;
};
template <int NU>
__device__ __forceinline__ RolloutLds stage_rollout_inputs(const unsigned char* maze, int ncell, const double* U, const double2* path,
                                                           const MppiArgs& a, unsigned char* lds_raw) {
  RolloutLds l;
  l.path = (double2*)lds_raw;
  l.U = (double*)(l.path + a.P);
  l.red = l.U + NU * a.T;
  l.maze = (unsigned char*)(l.red + 16);
  for (int i = threadIdx.x; i < a.P; i += blockDim.x) l.path[i] = path[i];
  for (int i = threadIdx.x; i < NU * a.T; i += blockDim.x) l.U[i] = U[i];
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) l.maze[i] = maze[i];
  return l;
}
__device__ __forceinline__ void store_rollout(bool mine, int k, double cost, int flag, double* costs, int32_t* flags,
                                              unsigned long long* minkey) {
  if (mine) {
    costs[k] = cost;
    if (flags != nullptr) flags[k] = flag;
  }
  const double m = wave_min(mine ? cost : __builtin_huge_val());
  if ((threadIdx.x & 63) == 0) atomicMin(minkey, mppi_key(m));
}

template <int G>
__global__ void __launch_bounds__(256)
mppi_rollout_kernel(const unsigned char* __restrict__ maze, int rows, int cols, CarTail m, const double* __restrict__ state,
                    const double* __restrict__ U, const double2* __restrict__ path, const double* __restrict__ noise,
                    MppiArgs a, double* __restrict__ costs, int32_t* __restrict__ flags, double* __restrict__ result,
                    unsigned long long* __restrict__ minkey) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RolloutLds l = stage_rollout_inputs<2>(maze, rows * cols, U, path, a, lds_raw);
  const int tid = threadIdx.x;
  double x0[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) x0[j] = state[j];
  __syncthreads();
  const int i0 = block_nearest_index(l.path, a.P, x0[0], x0[1], blockDim.x, l.red, (int*)(l.red + 8));
  const int k = (blockIdx.x * blockDim.x + tid) / G, g = tid & (G - 1);
  if (blockIdx.x == 0 && tid == 0 && result != nullptr) result[5] = (double)i0;
  const bool live = k < a.K;                           // quad-uniform (G lanes share k)
  double cost;
  int flag;
  car_rollout<G>(a, m, l.path, l.U, l.maze, rows, cols, x0, i0, noise, k, g, live, cost, flag);
  store_rollout(live && g == 0, k, cost, flag, costs, flags, minkey);
}

__global__ void __launch_bounds__(256)
mppi_ant_rollout_kernel(const unsigned char* __restrict__ maze, int rows, int cols, AntTail m, const double* __restrict__ state,
                        const double* __restrict__ U, const double2* __restrict__ path, const double* __restrict__ noise,
                        MppiArgs a, double* __restrict__ costs, int32_t* __restrict__ flags, double* __restrict__ result,
                        unsigned long long* __restrict__ minkey) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const RolloutLds l = stage_rollout_inputs<ANT_D>(maze, rows * cols, U, path, a, lds_raw);
  const int tid = threadIdx.x;
  const double x00 = state[0], x01 = state[1];
  __syncthreads();
  const int i0 = block_nearest_index(l.path, a.P, x00, x01, blockDim.x, l.red, (int*)(l.red + 8));
  const int k = blockIdx.x * blockDim.x + tid;
  if (blockIdx.x == 0 && tid == 0 && result != nullptr) result[5] = (double)i0;
  const bool live = k < a.K;
  double s[ANT_S];
#pragma unroll
  for (int j = 0; j < ANT_S; ++j) s[j] = state[j];
  double cost = 0.0;
  int ip = i0, flag = 0;
  for (int t = 0; live && t < a.T; ++t) {
    double e[ANT_D], u[ANT_D];
#pragma unroll
    for (int d = 0; d < ANT_D; ++d) e[d] = 0.0;
    if (a.k0 + k > 0) {                                // GLOBAL rollout 0 is the noise-free nominal sequence
      if (noise != nullptr) {
#pragma unroll
        for (int d = 0; d < ANT_D; ++d) e[d] = noise[((size_t)k * a.T + t) * ANT_D + d];
      } else {
        AntModel::noise(a, m, a.k0 + k, t, e);
      }
    }
    double ctrl = 0.0;
#pragma unroll
    for (int d = 0; d < ANT_D; ++d) {
      const double ud = l.U[ANT_D * t + d];
      u[d] = ud + e[d];
      ctrl = ctrl + (ud * e[d]) / (m.sigma[d] * m.sigma[d]);
    }
    ant_model_step(s, u, m.model);                      // the model clips the action to [-1, 1] as the env's action space does
    const bool coll = ant_collides(s, l.maze, rows, cols, m.s_global, m.ball_radius);
    const double ex = s[0] - a.gx, ey = s[1] - a.gy;
    const bool reached = sqrt(fma(ey, ey, ex * ex)) < m.goal_radius;
    const int lo = max(ip - a.wback, 0), hi = min(ip + a.wfwd, a.P - 1);
    double best = __builtin_huge_val();
    int bi = lo;
    // eight points per trip: independent LDS reads and distances, only the running minimum chains (one read-wait-compare
    // round per point exposed the LDS latency 57 times per step); indices past `hi` are clamped for the read and masked
    for (int i = lo; i <= hi; i += 8) {
      double d[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double2 pt = l.path[min(i + q, hi)];
        const double dx = pt.x - s[0], dy = pt.y - s[1];
        d[q] = dx * dx + dy * dy;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (i + q <= hi && d[q] < best) { best = d[q]; bi = i + q; }
    }
    ip = bi;
    cost = cost + a.w_track * best;
    cost = cost + a.lambda * ctrl;
    if (coll) { cost = cost + a.w_collision; flag = 2; break; }
    if (reached) { cost = cost - a.w_goal; flag = 1; break; }
  }
  cost = cost + a.w_progress * (double)(a.P - 1 - ip);
  store_rollout(live, k, cost, flag, costs, flags, minkey);
}

// ---- update
__global__ void mppi_min_kernel(const unsigned long long* __restrict__ minkey, double* __restrict__ result) {
  result[3] = mppi_unkey(*minkey);                    // the rollout kernel's atomicMin, decoded
}

// Grid (slices, T): slice s owns rollouts [s * per, (s + 1) * per), block (s, t) reduces step t of them (block t = 0 also the
// three scalar sums and the weights).  A thread takes rollout lo + tid (+ 256, ...).  (One block per slice walked all T steps
// before: one wave per SIMD with nothing to hide the latency of the regenerated Box-Muller noise -- 78 us for the ant at
// K = 65 536, T = 16.)
template <class Model>
__global__ void __launch_bounds__(256)
mppi_partial_kernel(const double* __restrict__ costs, const double* __restrict__ noise, MppiArgs a, typename Model::Tail m,
                    const double* __restrict__ result, double* __restrict__ partial /*[slices][3 + NU T]*/,
                    double* __restrict__ weights, const int32_t* __restrict__ flags) {
  constexpr int NU = Model::NU;
  __shared__ double red[4][3 + NU];
  const int t = blockIdx.y;
  const int per = (a.K + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(lo + per, a.K);
  const double beta = result[3];
  const int nacc = 3 + NU * a.T;
  if (threadIdx.x < 4 * (3 + NU)) (&red[0][0])[threadIdx.x] = 0.0;
  __syncthreads();
  for (int kb = lo; kb < hi; kb += 256) {
    const int k = kb + (int)threadIdx.x;
    const bool valid = k < hi;
    const double w = valid ? mppi_weight(costs[k], beta, a.lambda) : 0.0;
    if (t == 0) {
      if (valid && weights != nullptr) weights[k] = w;                 // un-normalised; mppi_weights_kernel divides by eta
      mppi_accumulate_scalars(w, valid && flags != nullptr && flags[k] == 2, red[threadIdx.x >> 6]);
    }
    double e[NU];
#pragma unroll
    for (int d = 0; d < NU; ++d) e[d] = 0.0;
    if (valid && a.k0 + k > 0) {
      if (noise != nullptr) {
#pragma unroll
        for (int d = 0; d < NU; ++d) e[d] = noise[((size_t)k * a.T + t) * NU + d];
      } else {
        Model::noise(a, m, a.k0 + k, t, e);
      }
    }
    mppi_accumulate_noise<NU>(w, e, red[threadIdx.x >> 6]);
  }
  __syncthreads();
  if (t == 0 && threadIdx.x < 3) partial[(size_t)blockIdx.x * nacc + threadIdx.x] = mppi_row_tree(&red[0][0], 3 + NU, threadIdx.x);
  if (threadIdx.x < NU)
    partial[(size_t)blockIdx.x * nacc + 3 + NU * t + threadIdx.x] = mppi_row_tree(&red[0][0], 3 + NU, 3 + threadIdx.x);
}

__global__ void __launch_bounds__(256) mppi_weights_kernel(double* __restrict__ weights, const double* __restrict__ sums, int K) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < K) weights[k] = weights[k] / sums[0];
}

// sums [3 + NU T] = {eta = sum w, sum w^2, collided rollouts, sum_k w_k eps[k, t, d]}: the quantities a sharded controller
// all-reduces (SUM) between its ranks.  do_sums: ordered sum of the slices -> sums;  do_apply: U += sums[3..] / eta,
// result[4], [6], [7] (the weights are normalised by mppi_weights_kernel);  do_execute: one env step with U[0], shift.
template <class Model>
__global__ void __launch_bounds__(256)
mppi_finish_kernel(const unsigned char* __restrict__ maze, int rows, int cols, const double* __restrict__ partial, int slices,
                   MppiArgs a, typename Model::Tail m, double* __restrict__ state_io, double* __restrict__ U,
                   double* __restrict__ sums, double* __restrict__ result, int do_sums, int do_apply, int do_execute) {
  if (do_sums) mppi_sum_slices(partial, slices, 3 + Model::NU * a.T, sums);
  if (do_apply) mppi_apply(sums, Model::NU * a.T, U, result);
  if (do_execute && threadIdx.x == 0) {
    double act[Model::NU], next[Model::NX];
    result[2] = (double)mppi_execute<Model>(a, m, maze, rows, cols, state_io, next, U, act);
    for (int d = 0; d < Model::NU; ++d) result[Model::ACTION_AT + d] = act[d];
    for (int j = 0; j < Model::NX; ++j) { state_io[j] = next[j]; result[Model::STATE_AT + j] = next[j]; }
  }
}

// ---- host: what differs between the models is how the rollouts are launched
struct CarLaunch {
  using Model = CarModel;
  static const void* rollout_fn(int lanes) {
    return lanes == 4 ? (const void*)mppi_rollout_kernel<4> : (lanes == 2 ? (const void*)mppi_rollout_kernel<2> : (const void*)mppi_rollout_kernel<1>);
  }
  static void grid(int K, int lanes, dim3& grid, dim3& block) {
    block = dim3(256);
    grid = dim3((unsigned)(((long long)K * lanes + 255) / 256));
  }
};
struct AntLaunch {
  using Model = AntModel;
  static const void* rollout_fn(int) { return (const void*)mppi_ant_rollout_kernel; }
  static void grid(int K, int, dim3& grid, dim3& block) {
    const int blk = K >= 32768 ? 256 : 64;
    block = dim3(blk);
    grid = dim3((K + blk - 1) / blk);
  }
};

// One controller step (or the stages of one) of either model: `who` names the entry point in messages, `lanes` is 1 for the ant.
template <class L>
int mppi_launch(ditree_ctx* ctx, const char* who, MppiArgs a, typename L::Model::Tail m, int lanes, double* state_io, double* U_io,
                const double* path_xy, const double* noise, int stages, double* costs, double* weights, int32_t* flags,
                double* sums, double* result, void* stream) {
  using Model = typename L::Model;
  constexpr int NU = Model::NU;
  const std::string name(who);
  if (!state_io || !U_io || !path_xy || !costs || !result || !sums || a.T < 1 || a.T > MPPI_MAX_T || a.K < 1 || a.P < 1 ||
      a.P > MPPI_MAX_P || !(a.lambda > 0.0) || a.wback < 0 || a.wfwd < 0 || (stages & ~DITREE_MPPI_ALL) != 0 || stages == 0 ||
      a.k0 < 0)
    return set_err(ctx, DITREE_E_ARG, name + ": bad argument (1 <= T <= 64, 1 <= P <= 4096, lambda, sigma > 0, stages 1..31)");
  for (int d = 0; d < NU; ++d)
    if (!(m.sigma[d] > 0.0)) return set_err(ctx, DITREE_E_ARG, name + ": sigma must be positive");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int slices = std::min(MPPI_SLICES, (a.K + 255) / 256);      // 256 rollouts per slice up to 65 536, more beyond
  if (!ctx->mppi_partial || !ctx->mppi_minkey) {             // both or neither: a failed second allocation is retried, never skipped
    if (!ctx->mppi_partial)
      HIP_TRY(ctx, hipMalloc((void**)&ctx->mppi_partial, (size_t)MPPI_SLICES * (3 + ANT_D * MPPI_MAX_T) * sizeof(double)));
    if (!ctx->mppi_minkey) HIP_TRY(ctx, hipMalloc((void**)&ctx->mppi_minkey, sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->mppi_minkey, 0xFF, sizeof(unsigned long long), s));
  }
  if (stages & DITREE_MPPI_ROLLOUTS) {
    const size_t lds = (size_t)a.P * 16 + (size_t)a.T * NU * 8 + 128 + (((size_t)ctx->rows * ctx->cols + 15) & ~(size_t)15);
    if (lds > 160 * 1024) return set_err(ctx, DITREE_E_ARG, name + ": path + maze exceed the LDS");
    const void* fn = L::rollout_fn(lanes);
    static bool attr_done[64][3] = {};
    if (lds > 64 * 1024 && ctx->device < 64 && !attr_done[ctx->device][lanes >> 1]) {
      HIP_TRY(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_done[ctx->device][lanes >> 1] = true;
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->mppi_minkey, 0xFF, sizeof(unsigned long long), s));
    dim3 grid, block;
    L::grid(a.K, lanes, grid, block);
    const unsigned char* maze = ctx->maze;
    int rows = ctx->rows, cols = ctx->cols;
    const double2* path = (const double2*)path_xy;
    unsigned long long* minkey = ctx->mppi_minkey;
    // both rollout kernels take this list (the tail before the pointers, MppiArgs after them: profiles/NOTES.md "MPPI core")
    void* args[] = {&maze, &rows, &cols, &m, &state_io, &U_io, &path, &noise, &a, &costs, &flags, &result, &minkey};
    HIP_TRY(ctx, hipLaunchKernel(fn, grid, block, args, lds, s));
  }
  if (stages & DITREE_MPPI_MIN) hipLaunchKernelGGL(mppi_min_kernel, dim3(1), dim3(1), 0, s, ctx->mppi_minkey, result);
  if (stages & DITREE_MPPI_SUMS)
    hipLaunchKernelGGL(mppi_partial_kernel<Model>, dim3(slices, a.T), dim3(256), 0, s, costs, noise, a, m, result, ctx->mppi_partial,
                       weights, flags);
  if (stages & (DITREE_MPPI_SUMS | DITREE_MPPI_APPLY | DITREE_MPPI_EXECUTE))
    hipLaunchKernelGGL(mppi_finish_kernel<Model>, dim3(1), dim3(256), 0, s, ctx->maze, ctx->rows, ctx->cols, ctx->mppi_partial,
                       slices, a, m, state_io, U_io, sums, result, (stages & DITREE_MPPI_SUMS) ? 1 : 0,
                       (stages & DITREE_MPPI_APPLY) ? 1 : 0, (stages & DITREE_MPPI_EXECUTE) ? 1 : 0);
  if ((stages & DITREE_MPPI_APPLY) && weights != nullptr)
    hipLaunchKernelGGL(mppi_weights_kernel, dim3((a.K + 255) / 256), dim3(256), 0, s, weights, sums, a.K);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// the fields the two parameter blocks share, by name
template <class Params>
MppiArgs shared_args(const Params* p, int P, const double* goal_xy, uint64_t counter) {
  MppiArgs a;
  a.T = p->T; a.K = p->K; a.P = P;
  a.lambda = p->lambda;
  a.w_track = p->w_track; a.w_progress = p->w_progress; a.w_collision = p->w_collision; a.w_goal = p->w_goal;
  a.seed = p->seed; a.counter = counter;
  a.wback = p->window_back; a.wfwd = p->window_fwd;
  a.gx = goal_xy[0]; a.gy = goal_xy[1];
  a.k0 = p->k_offset;
  return a;
}

}  // namespace

extern "C" int32_t ditree_mppi_step(ditree_ctx* ctx, const ditree_mppi_params* p, double* state_io, double* U_io,
                                    const double* path_xy, int32_t P, const double* goal_xy, const double* noise,
                                    uint64_t counter, int32_t stages, double* costs, double* weights, int32_t* flags,
                                    double* sums, double* result, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "mppi_step: no maze uploaded");
  if (!p || !goal_xy) return set_err(ctx, DITREE_E_ARG, "mppi_step: bad argument (null parameters or goal)");
  if (p->lanes != 0 && p->lanes != 1 && p->lanes != 2 && p->lanes != 4)
    return set_err(ctx, DITREE_E_ARG, "mppi_step: lanes must be 0, 1, 2 or 4");
  const CarTail m{{p->sigma[0], p->sigma[1]}};
  return mppi_launch<CarLaunch>(ctx, "mppi_step", shared_args(p, P, goal_xy, counter), m, p->lanes == 0 ? MPPI_DEFAULT_LANES : p->lanes,
                                state_io, U_io, path_xy, noise, stages, costs, weights, flags, sums, result, stream);
}

extern "C" int32_t ditree_mppi_step_ant(ditree_ctx* ctx, const ditree_mppi_ant_params* p, double* state_io, double* U_io,
                                        const double* path_xy, int32_t P, const double* desired_goal_xy, const double* noise,
                                        uint64_t counter, int32_t stages, double* costs, double* weights, int32_t* flags,
                                        double* sums, double* result, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "mppi_step_ant: no maze uploaded");
  if (!p || !desired_goal_xy || !(p->s_global > 0.0))
    return set_err(ctx, DITREE_E_ARG, "mppi_step_ant: bad argument (null parameters or goal, s_global > 0)");
  AntTail m;
  for (int d = 0; d < ANT_D; ++d) m.sigma[d] = p->sigma[d];
  m.goal_radius = p->goal_radius; m.ball_radius = p->ball_radius; m.s_global = p->s_global;
  if (const int rc = fill_ant_model(ctx, &p->model, &m.model)) return rc;
  return mppi_launch<AntLaunch>(ctx, "mppi_step_ant", shared_args(p, P, desired_goal_xy, counter), m, 1, state_io, U_io, path_xy,
                                noise, stages, costs, weights, flags, sums, result, stream);
}
