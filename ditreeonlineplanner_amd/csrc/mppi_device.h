// The MPPI controller core: every piece of the controller that more than one kernel runs, stated once.  mppi_kernels.hip (one
// controller step as separate launches, car and ant) and mppi_mission_kernels.hip (whole car missions in one work-group) call
// these functions and nothing else for the shared arithmetic, so the mission kernel equals the stepwise controller bit for bit
// because it IS the same code, compiled with the same -ffp-contract=off.
//
// A model is a traits struct with static members (no run-time nu, no function pointers): NX, NU, ACTION_AT / STATE_AT (where the
// executed action and the state stand in the result block), Tail (its kernel arguments after MppiArgs), noise() and env_step().
// CarModel is below; AntModel stands in mppi_kernels.hip next to the one kernel that needs ant_device.h.
//
// Summation orders (fixed: results are reproducible and a sharded controller adds the same numbers): wave butterfly o = 32 .. 1,
// lane 0 adds into its wave's row in loop order, rows as (r0 + r1) + (r2 + r3), slices in index order in groups of 16.
#pragma once
#include <hip/hip_runtime.h>

#include "car_device.h"

constexpr int MPPI_MAX_T = 64;
constexpr int MPPI_MAX_P = 4096;         // reference path points staged in LDS (64 KB of f64 pairs)
constexpr int MPPI_SLICES = 256;         // partial-sum slices of the update
constexpr int MPPI_DEFAULT_LANES = 2;    // lanes per car rollout when the caller does not choose (measured: DESIGN.md "MPPI")

// what every model's kernels take; the model's own constants follow in its Tail
struct MppiArgs {
  int T, K, P;
  double lambda, w_track, w_progress, w_collision, w_goal;
  unsigned long long seed, counter;
  int wback, wfwd;
  double gx, gy;
  long long k0;                       // global index of this rank's first rollout (sharded controller)
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// eps[k, t, :] ~ N(0, diag(sigma^2)): counter-based, a pure function of (seed, counter, k, t)
__device__ __forceinline__ void mppi_noise(unsigned long long seed, unsigned long long counter, long long k, int t, double s0,
                                           double s1, double& e0, double& e1) {
  unsigned long long h = splitmix64(seed ^ splitmix64(counter));
  h = splitmix64(h ^ ((unsigned long long)k * 0xD1B54A32D192ED03ull));
  h = splitmix64(h ^ (unsigned long long)t);
  const unsigned long long h2 = splitmix64(h);
  const double u1 = ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740992.0);      // (0, 1]
  const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);             // [0, 1)
  const double r = sqrt(-2.0 * log(u1));
  const double a = 6.283185307179586 * u2;
  double sa, ca;
  sincos(a, &sa, &ca);
  e0 = s0 * (r * ca);
  e1 = s1 * (r * sa);
}

// order-preserving map double -> unsigned 64-bit (and back): negative values flip all bits, the others the sign bit
__device__ __forceinline__ unsigned long long mppi_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mppi_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

template <int G> __device__ __forceinline__ double quad_min(double v) {
  if constexpr (G >= 2) v = fmin(v, __shfl_xor(v, 1));
  if constexpr (G == 4) v = fmin(v, __shfl_xor(v, 2));
  return v;
}
template <int G> __device__ __forceinline__ int quad_min_i(int v) {
  if constexpr (G >= 2) v = min(v, __shfl_xor(v, 1));
  if constexpr (G == 4) v = min(v, __shfl_xor(v, 2));
  return v;
}
template <int G> __device__ __forceinline__ bool quad_or(bool v) {
  if constexpr (G >= 2) {
    int x = v ? 1 : 0;
    x |= __shfl_xor(x, 1);
    if constexpr (G == 4) x |= __shfl_xor(x, 2);
    return x != 0;
  }
  return v;
}

// nearest path index of `x, y` in [lo, hi] (first occurrence of the minimum, as np.argmin); lane g scans lo + g, lo + g + G, ...
template <int G>
__device__ __forceinline__ void nearest_in_window(const double2* path, int lo, int hi, double x, double y, int g, int& idx,
                                                  double& d2) {
  double best = __builtin_huge_val();
  int bi = 0x7fffffff;
  // four points per trip: their LDS reads and distances are independent (one read-wait-compare round per point left the LDS
  // latency exposed 28 times per step -- the window search was the longest part of a controller step), only the running
  // minimum chains; indices past `hi` are clamped for the read and masked for the compare
  for (int i = lo + g; i <= hi; i += 4 * G) {
    double d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double2 p = path[min(i + u * G, hi)];
      const double dx = p.x - x, dy = p.y - y;
      d[u] = dx * dx + dy * dy;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * G <= hi && d[u] < best) { best = d[u]; bi = i + u * G; }
  }
  const double m = quad_min<G>(best);
  // first index attaining the minimum over the quad (ties -> lowest index)
  idx = quad_min_i<G>(best == m ? bi : 0x7fffffff);
  d2 = m;
}

// i0 = nearest point of the WHOLE staged path to (x, y), ties to the lowest index: block-cooperative over `nthreads` threads
// (whole waves), the same in every block.  s_d / s_i: one LDS slot per wave; contains one barrier.
__device__ __forceinline__ int block_nearest_index(const double2* s_path, int P, double x, double y, int nthreads, double* s_d,
                                                   int* s_i) {
  const int tid = threadIdx.x;
  double best = __builtin_huge_val();
  int bi = 0x7fffffff;
  for (int i = tid; i < P; i += nthreads) {
    const double dx = s_path[i].x - x, dy = s_path[i].y - y;
    const double d = dx * dx + dy * dy;
    if (d < best) { best = d; bi = i; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if ((tid & 63) == 0) { s_d[tid >> 6] = best; s_i[tid >> 6] = bi; }
  __syncthreads();
  best = s_d[0]; bi = s_i[0];
  for (int w = 1; w < (nthreads >> 6); ++w)
    if (s_d[w] < best || (s_d[w] == best && s_i[w] < bi)) { best = s_d[w]; bi = s_i[w]; }
  return bi;
}

// ---- the car model
struct CarTail { double sigma[2]; };

struct CarModel {
  static constexpr int NX = 6, NU = 2;
  static constexpr int ACTION_AT = 0, STATE_AT = 8;          // result [16]: action [0..2), the state after EXECUTE [8..14)
  using Tail = CarTail;
  static __device__ __forceinline__ void noise(const MppiArgs& a, const CarTail& m, long long k, int t, double* e) {
    mppi_noise(a.seed, a.counter, k, t, m.sigma[0], m.sigma[1], e[0], e[1]);
  }
  // one env step of `s` with the control `u`, clipped as the env clips it (car_env.py:371) -> act; collision against the KNOWN
  // maze: 0, 1 = inside the goal radius (car_env.py:346-351), 2 = collided
  static __device__ __forceinline__ int env_step(const MppiArgs& a, const CarTail&, const unsigned char* maze, int rows, int cols,
                                                 double* s, const double* u, double* act) {
    act[0] = fmin(fmax(u[0], -10.0), 10.0);
    act[1] = fmin(fmax(u[1], -2.0), 2.0);
    car_euler_step(s, act[0], act[1]);
    const double ex = s[0] - a.gx, ey = s[1] - a.gy;
    const bool reached = sqrt(fma(ey, ey, ex * ex)) < 0.5;
    return car_collides(s[0], s[1], s[2], maze, rows, cols) ? 2 : (reached ? 1 : 0);
  }
};

// One car rollout: T x [noise, dynamics, two-ball collision, goal test, nearest reference-path point], the stage cost
// q(x) + lambda u^T Sigma^-1 eps term by term.  G adjacent lanes share rollout k (local index; a.k0 + k is the global one, and
// GLOBAL rollout 0 is the noise-free nominal sequence): every lane integrates the identical dynamics, lane g tests ball g & 1
// and scans every G-th point of the path window, the lanes combine by DPP.  `live` is uniform over the G lanes.
template <int G>
__device__ __forceinline__ void car_rollout(const MppiArgs& a, const CarTail& m, const double2* s_path, const double* s_U,
                                            const unsigned char* s_maze, int rows, int cols, const double* x0, int i0,
                                            const double* noise, int k, int g, bool live, double& cost, int& flag) {
  double s[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) s[j] = x0[j];
  cost = 0.0;
  int ip = i0;
  flag = 0;                                            // 1 = reached the goal, 2 = collided
  double n0 = 0.0, n1 = 0.0;                           // G >= 2: the noise this lane generated for step (t & ~1) + (g & 1)
  for (int t = 0; live && t < a.T; ++t) {
    double e0 = 0.0, e1 = 0.0;
    if (a.k0 + k > 0) {
      if (noise != nullptr) {
        e0 = noise[((size_t)k * a.T + t) * 2]; e1 = noise[((size_t)k * a.T + t) * 2 + 1];
      } else if constexpr (G >= 2) {
        // the lanes of a rollout would all evaluate the same Box-Muller pair (log, sqrt, sincos: a quarter of the step): lane
        // parity p generates the pair of step t + p on even t and hands it to its neighbour for the other step (the branches
        // around this are uniform over the lanes of a rollout, so both partners always execute the exchange)
        if ((t & 1) == 0) {
          n0 = 0.0; n1 = 0.0;
          if (t + (g & 1) < a.T) mppi_noise(a.seed, a.counter, a.k0 + k, t + (g & 1), m.sigma[0], m.sigma[1], n0, n1);
        }
        const double o0 = __shfl_xor(n0, 1), o1 = __shfl_xor(n1, 1);
        const bool mine = (t & 1) == (g & 1);
        e0 = mine ? n0 : o0; e1 = mine ? n1 : o1;
      } else {
        mppi_noise(a.seed, a.counter, a.k0 + k, t, m.sigma[0], m.sigma[1], e0, e1);
      }
    }
    const double u0 = s_U[2 * t], u1 = s_U[2 * t + 1];
    car_euler_step(s, u0 + e0, u1 + e1);
    // collision: lane g tests ball g & 1 (front / back), the quad ORs
    bool coll;
    if constexpr (G >= 2) {
      const double off = 0.15 * 0.5;
      const double sgn = (g & 1) ? -1.0 : 1.0;
      double sps, cps;
      sincos(s[2], &sps, &cps);
      const double ox = off * cps, oy = off * sps;
      coll = quad_or<G>(ball_collides(s[0] + sgn * ox, s[1] + sgn * oy, s_maze, rows, cols));
    } else {
      coll = car_collides(s[0], s[1], s[2], s_maze, rows, cols);
    }
    const double ex = s[0] - a.gx, ey = s[1] - a.gy;
    const bool reached = sqrt(fma(ey, ey, ex * ex)) < 0.5;                       // car_env.py:346-351
    const int lo = max(ip - a.wback, 0), hi = min(ip + a.wfwd, a.P - 1);
    double d2;
    nearest_in_window<G>(s_path, lo, hi, s[0], s[1], g, ip, d2);
    cost = cost + a.w_track * d2;
    cost = cost + a.lambda * ((u0 * e0) / (m.sigma[0] * m.sigma[0]) + (u1 * e1) / (m.sigma[1] * m.sigma[1]));
    if (coll) { cost = cost + a.w_collision; flag = 2; break; }
    if (reached) { cost = cost - a.w_goal; flag = 1; break; }
  }
  cost = cost + a.w_progress * (double)(a.P - 1 - ip);
}

// ---- update: beta = min S, w_k = exp(-(S_k - beta) / lambda), eta = sum w, dU[t] = sum_k w_k eps[k, t] / eta
__device__ __forceinline__ double mppi_weight(double cost, double beta, double lambda) { return exp(-(cost - beta) / lambda); }

// One trip of a wave over up to 64 rollouts: `w` is this lane's weight (0 where it holds no rollout), e its noise at step t.
// row [3 + NU] = {eta, sum w^2, collided rollouts (exact: integers), sum w eps[t, 0..NU)} is the wave's running row, zero before
// the first trip; the three scalars are summed with step 0 only.  Lane 0's row is the one that counts.
__device__ __forceinline__ void mppi_accumulate_scalars(double w, bool collided, double* row) {
  const double sw = wave_sum(w), sw2 = wave_sum(w * w);
  const double sc = wave_sum(collided ? 1.0 : 0.0);
  if ((threadIdx.x & 63) == 0) { row[0] += sw; row[1] += sw2; row[2] += sc; }
}
template <int NU> __device__ __forceinline__ void mppi_accumulate_noise(double w, const double* e, double* row) {
#pragma unroll
  for (int d = 0; d < NU; ++d) {
    const double v = wave_sum(w * e[d]);
    if ((threadIdx.x & 63) == 0) row[3 + d] += v;
  }
}
// value j of a slice from the rows of its four waves (`stride` doubles apart)
__device__ __forceinline__ double mppi_row_tree(const double* rows, int stride, int j) {
  return (rows[j] + rows[stride + j]) + (rows[2 * stride + j] + rows[3 * stride + j]);
}

// do_sums: thread j adds value j of the slices in slice order; nacc = 3 + NU T values, <= 256 slices.  The loads of a value
// are independent, only the adds chain (a per-value block reduction with two barriers each took 98 us for the 131 values of
// the ant at T = 16: profiles/r04_mppi_ant_bench_kernel_stats.csv).  Ends with a barrier: `sums` is then visible to the block.
__device__ __forceinline__ void mppi_sum_slices(const double* partial, int slices, int nacc, double* sums) {
  for (int j = threadIdx.x; j < nacc; j += 256) {
    double acc = 0.0;
    for (int s0 = 0; s0 < slices; s0 += 16) {                 // 16 loads in flight, then their adds in slice order
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = s0 + u < slices ? partial[(size_t)(s0 + u) * nacc + j] : 0.0;
#pragma unroll
      for (int u = 0; u < 16; ++u) acc += v[u];
    }
    sums[j] = acc;
  }
  __threadfence_block();
  __syncthreads();
}
// do_apply: U += sums[3..] / eta; result[4] = eta, [6] = collided rollouts, [7] = effective sample size.  Ends with a barrier.
__device__ __forceinline__ void mppi_apply(const double* sums, int n_controls, double* U, double* result) {
  const double eta = sums[0];
  for (int j = threadIdx.x; j < n_controls; j += 256) U[j] = U[j] + sums[3 + j] / eta;
  if (threadIdx.x == 0) {
    result[4] = eta;
    result[6] = sums[2];
    result[7] = (eta * eta) / sums[1];
  }
  __syncthreads();
}
// do_execute (one thread): one env step from the state `x` with the first control -> act; s = the state after it.  A collided
// step leaves the state (s = x) and restarts the nominal sequence from rest, any other shifts it with the last control held.
template <class Model>
__device__ __forceinline__ int mppi_execute(const MppiArgs& a, const typename Model::Tail& m, const unsigned char* maze, int rows,
                                            int cols, const double* x, double* s, double* U, double* act) {
  constexpr int NX = Model::NX, NU = Model::NU;
  for (int j = 0; j < NX; ++j) s[j] = x[j];
  const int status = Model::env_step(a, m, maze, rows, cols, s, U, act);
  if (status == 2) {
    for (int j = 0; j < NU * a.T; ++j) U[j] = 0.0;
    for (int j = 0; j < NX; ++j) s[j] = x[j];
  } else {
    for (int t = 0; t + 1 < a.T; ++t)
      for (int d = 0; d < NU; ++d) U[NU * t + d] = U[NU * (t + 1) + d];
  }
  return status;
}
