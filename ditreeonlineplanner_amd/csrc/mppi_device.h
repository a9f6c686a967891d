// Device functions of the MPPI controller shared by the units that run it (mppi_kernels.hip: one controller step as separate
// launches; mppi_mission_kernels.hip: whole missions in one work-group).  Both units are compiled with -ffp-contract=off and
// must evaluate these expressions identically: the mission kernel is held to the stepwise controller bit for bit.
#pragma once
#include <hip/hip_runtime.h>

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

struct MppiArgs {
  int T, K, P;
  double lambda, s0, s1, w_track, w_progress, w_collision, w_goal;
  unsigned long long seed, counter;
  int wback, wfwd;
  double gx, gy;
  long long k0;                       // global index of this rank's first rollout (sharded controller)
};

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
