// MPPI missions on the device (gfx950, FP64): the MPPI driver's control loop `run_scenarios_with_lidar_MPPI.py:417-452` --
// controller step, collision retries, trace, and a lidar scan with the known-maze update every `scan_time` -- as ONE launch.
// One work-group of 256 threads owns one mission from its first controller step to its terminating event; a launch takes a
// grid of M independent missions (a fleet).  A work-group needs nothing from any other: no grid-wide synchronisation, no
// co-residency requirement, any M.
//
// Compiled with -ffp-contract=off like mppi_kernels.hip and geom_kernels.hip.  BIT-EXACTNESS IS THE CONTRACT: a mission equals
// the same number of ditree_mppi_step / lidar scan / ditree_upload_maze calls bit for bit (tests/test_gpu_mppi_mission.py holds
// it to np.array_equal).  K <= 256 is the stepwise controller's one-slice case, and every sum below takes that case's order:
//   rollouts   thread k runs rollout k with the G = 1 body of mppi_rollout_kernel (block-cooperative nearest index i0 with ties
//              to the lowest index, car_collides, nearest_in_window<1>, the cost expression term by term);
//   beta       an exact minimum (order-independent);
//   sums       mppi_partial_kernel for lo = 0: the 64-lane butterfly v += shfl_xor(v, o), o = 32 .. 1, lane 0 adding into its
//              wave's (zeroed) row, (r0 + r1) + (r2 + r3), then mppi_finish_kernel's acc = 0.0; acc += partial[0];
//   noise      regenerated per (k, t) with mppi_noise (mppi_device.h);
//   execute    mppi_finish_kernel's clip, collision restart and shift with the last control held;
//   scan       follow_plan_kernel's scan block (lidar_ray of lidar_device.h, end cells -> known / scanned, visited = 2).
// Every loop bound and every branch that contains a barrier is uniform over the work-group (flags in LDS, as
// follow_plan_kernel); the step count of a launch is bounded on the host (DITREE_MPPI_MISSION_MAX_STEPS).
#include "car_device.h"
#include "ditree_internal.h"
#include "lidar_device.h"
#include "mppi_device.h"

namespace {

constexpr int MISSION_MAX_T = 64;
constexpr int MISSION_MAX_K = 256;
constexpr int MISSION_MAX_P = 4096;
constexpr int MISSION_MAX_CELLS = 13104;                 // five byte maps of 13 104 cells = 64 KB, as follow_plan_kernel
constexpr int MISSION_NACC = 3 + 2 * MISSION_MAX_T;

struct MissionArgs {
  const unsigned long long* seed;      // (M)
  const unsigned long long* counter0;  // (M)
  double* state_io;                    // (M, 6)
  double* U_io;                        // (M, T, 2)
  const double2* path;                 // packed
  const int32_t* path_off;             // (M) first point of mission m
  const int32_t* path_len;             // (M)
  const double* goal;                  // (M, 2)
  float* known;                        // (M, rows, cols)
  const float* truth;
  float* scanned;
  const int32_t* max_steps;            // (M)
  const int32_t* allowed_trials;       // (M)
  const double* dt;                    // (M)
  const double* scan_time;             // (M)
  double* t_acc_io;                    // (M)
  int32_t* trials_io;                  // (M)
  double* ex_states;                   // (M, trace_steps, 6)
  double* ex_actions;                  // (M, trace_steps, 2)
  double* result;                      // (M, DITREE_MPPI_MISSION_RESULT)
  unsigned char* refresh_codes;        // the ctx's maze copy, refreshed from mission `refresh_mission` (or nullptr)
  int rows, cols, P_max, trace_steps, refresh_mission;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(256) mppi_mission_kernel(MissionArgs g, MppiArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int rows = g.rows, cols = g.cols, ncell = rows * cols, pad = (ncell + 15) & ~15;
  double2* s_path = (double2*)lds_raw;                                   // P_max points
  double* s_U = (double*)(s_path + g.P_max);                             // T x 2
  unsigned char* kn = (unsigned char*)(s_U + 2 * a.T);                   // known maze codes
  unsigned char* tr = kn + pad;                                          // true maze: 1 = occupied
  unsigned char* sc = kn + 2 * pad;                                      // scanned maze codes
  unsigned char* vis = kn + 3 * pad;                                     // cells visited by the current scan
  unsigned char* dirty = kn + 4 * pad;                                   // cells of known / scanned written by this launch
  __shared__ double s_x[6];                                              // the mission's state
  __shared__ double s_amin[4];                                           // block argmin of i0: distance, index per wave
  __shared__ int s_aidx[4];
  __shared__ double s_wmin[4];                                           // per-wave minimum of the costs
  __shared__ double s_rows[4][MISSION_NACC];                             // per-wave sums (mppi_partial_kernel's red rows)
  __shared__ double s_sums[MISSION_NACC];                                // eta, sum w^2, collided rollouts, sum_k w_k eps[k, t, d]
  __shared__ double s_last[5];                                           // beta, eta, i0, collided rollouts, effective samples
  __shared__ int sh_scan, sh_stop;

  a.P = g.path_len[m];
  const int nsteps = g.max_steps[m];
  double* res = g.result + (size_t)m * DITREE_MPPI_MISSION_RESULT;
  if (a.P < 1 || a.P > g.P_max || nsteps < 0 || nsteps > g.trace_steps) {          // uniform: refused before any barrier
    if (tid == 0) {
      for (int j = 0; j < DITREE_MPPI_MISSION_RESULT; ++j) res[j] = 0.0;
      res[0] = (double)DITREE_MEV_REFUSED;
    }
    return;
  }
  a.seed = g.seed[m];
  a.gx = g.goal[2 * m];
  a.gy = g.goal[2 * m + 1];
  a.k0 = 0;
  const unsigned long long counter0 = g.counter0[m];
  const int allowed = g.allowed_trials[m];
  const double dt = g.dt[m], scan_time = g.scan_time[m];
  const size_t mcell = (size_t)m * ncell;
  const double2* path = g.path + g.path_off[m];
  double* U = g.U_io + (size_t)m * 2 * a.T;
  for (int i = tid; i < a.P; i += 256) s_path[i] = path[i];
  for (int i = tid; i < 2 * a.T; i += 256) s_U[i] = U[i];
  for (int i = tid; i < ncell; i += 256) {
    kn[i] = maze_code(g.known[mcell + i]);
    tr[i] = g.truth[mcell + i] == 1.0f ? 1 : 0;
    sc[i] = maze_code(g.scanned[mcell + i]);
    vis[i] = 0;
    dirty[i] = 0;
  }
  if (tid < 6) s_x[tid] = g.state_io[(size_t)m * 6 + tid];
  if (tid < 5) s_last[tid] = 0.0;
  if (tid == 0) { sh_scan = 0; sh_stop = 0; }
  __syncthreads();

  // thread 0's books
  double t_acc = g.t_acc_io[m];
  int trials = g.trials_io[m];
  int event = DITREE_MEV_STEPS_DONE, calls = 0, n_exec = 0, n_scans = 0;
  const int nacc = 3 + 2 * a.T;
  const int wv = tid >> 6;
  const bool lane0 = (tid & 63) == 0;

  bool in_goal;                                                          // the driver's while-condition on the input state
  {
    const double ex = s_x[0] - a.gx, ey = s_x[1] - a.gy;
    in_goal = sqrt(fma(ey, ey, ex * ex)) < 0.5;                          // car_env.py:346-351 (uniform: every thread reads s_x)
  }
  if (in_goal) event = DITREE_MEV_GOAL;

  for (int c = 0; !in_goal && c < nsteps; ++c) {
    a.counter = counter0 + (unsigned long long)c;
    double x0[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) x0[j] = s_x[j];
    // ---- rollouts (mppi_rollout_kernel<1>): i0 = nearest path point of the state over the whole path
    int i0;
    {
      double best = __builtin_huge_val();
      int bi = 0x7fffffff;
      for (int i = tid; i < a.P; i += 256) {
        const double dx = s_path[i].x - x0[0], dy = s_path[i].y - x0[1];
        const double d = dx * dx + dy * dy;
        if (d < best) { best = d; bi = i; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (lane0) { s_amin[wv] = best; s_aidx[wv] = bi; }
      __syncthreads();
      best = s_amin[0]; bi = s_aidx[0];
      for (int w = 1; w < 4; ++w)
        if (s_amin[w] < best || (s_amin[w] == best && s_aidx[w] < bi)) { best = s_amin[w]; bi = s_aidx[w]; }
      i0 = bi;
    }
    const int k = tid;
    const bool live = k < a.K;
    double s[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = x0[j];
    double cost = 0.0;
    int ip = i0;
    int flag = 0;                                        // 1 = reached the goal, 2 = collided
    for (int t = 0; live && t < a.T; ++t) {
      double e0 = 0.0, e1 = 0.0;
      if (k > 0) mppi_noise(a.seed, a.counter, k, t, a.s0, a.s1, e0, e1);        // rollout 0 is the noise-free nominal sequence
      const double u0 = s_U[2 * t], u1 = s_U[2 * t + 1];
      car_euler_step(s, u0 + e0, u1 + e1);
      const bool coll = car_collides(s[0], s[1], s[2], kn, rows, cols);
      const double ex = s[0] - a.gx, ey = s[1] - a.gy;
      const bool reached = sqrt(fma(ey, ey, ex * ex)) < 0.5;
      const int lo = max(ip - a.wback, 0), hi = min(ip + a.wfwd, a.P - 1);
      double d2;
      nearest_in_window<1>(s_path, lo, hi, s[0], s[1], 0, ip, d2);
      cost = cost + a.w_track * d2;
      cost = cost + a.lambda * ((u0 * e0) / (a.s0 * a.s0) + (u1 * e1) / (a.s1 * a.s1));
      if (coll) { cost = cost + a.w_collision; flag = 2; break; }
      if (reached) { cost = cost - a.w_goal; flag = 1; break; }
    }
    cost = cost + a.w_progress * (double)(a.P - 1 - ip);
    // ---- beta = min_k S_k
    double mn = live ? cost : __builtin_huge_val();
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o));
    if (lane0) s_wmin[wv] = mn;
    __syncthreads();
    const double beta = fmin(fmin(s_wmin[0], s_wmin[1]), fmin(s_wmin[2], s_wmin[3]));
    // ---- weights and sums (mppi_partial_kernel, one slice, lo = 0; mppi_finish_kernel's ordered sum of that one slice)
    const double w = live ? exp(-(cost - beta) / a.lambda) : 0.0;
    {
      const double sw = wave_sum(w), sw2 = wave_sum(w * w);
      const double scn = wave_sum((live && flag == 2) ? 1.0 : 0.0);
      if (lane0) {
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        r0 += sw; r1 += sw2; r2 += scn;
        s_rows[wv][0] = r0; s_rows[wv][1] = r1; s_rows[wv][2] = r2;
      }
    }
    for (int t = 0; t < a.T; ++t) {
      double e0 = 0.0, e1 = 0.0;
      if (live && k > 0) mppi_noise(a.seed, a.counter, k, t, a.s0, a.s1, e0, e1);
      const double v0 = wave_sum(w * e0), v1 = wave_sum(w * e1);
      if (lane0) {
        double r3 = 0.0, r4 = 0.0;
        r3 += v0; r4 += v1;
        s_rows[wv][3 + 2 * t] = r3; s_rows[wv][4 + 2 * t] = r4;
      }
    }
    __syncthreads();
    if (tid < nacc) {
      const double partial = (s_rows[0][tid] + s_rows[1][tid]) + (s_rows[2][tid] + s_rows[3][tid]);
      double acc = 0.0;
      acc += partial;
      s_sums[tid] = acc;
    }
    __syncthreads();
    // ---- apply (mppi_finish_kernel): U += sums[3..] / eta
    const double eta = s_sums[0];
    if (tid < 2 * a.T) s_U[tid] = s_U[tid] + s_sums[3 + tid] / eta;
    __syncthreads();
    // ---- execute: one env step with the first control against the KNOWN maze, then the driver's books
    if (tid == 0) {
      s_last[0] = beta;
      s_last[1] = eta;
      s_last[2] = (double)i0;
      s_last[3] = s_sums[2];
      s_last[4] = (eta * eta) / s_sums[1];
      ++calls;
      double st[6];
      for (int j = 0; j < 6; ++j) st[j] = s_x[j];
      const double a0 = fmin(fmax(s_U[0], -10.0), 10.0), a1 = fmin(fmax(s_U[1], -2.0), 2.0);
      car_euler_step(st, a0, a1);
      const double ex = st[0] - a.gx, ey = st[1] - a.gy;
      const bool reached = sqrt(fma(ey, ey, ex * ex)) < 0.5;
      const bool coll = car_collides(st[0], st[1], st[2], kn, rows, cols);
      int scan = 0, stop = 0;
      if (coll) {                                        // the state stays; the nominal sequence restarts from rest
        for (int j = 0; j < 2 * a.T; ++j) s_U[j] = 0.0;
        ++trials;
        if (trials >= allowed) { event = DITREE_MEV_TRIALS; stop = 1; }
      } else {
        trials = 0;
        double* eo = g.ex_states + ((size_t)m * g.trace_steps + n_exec) * 6;
        double* ao = g.ex_actions + ((size_t)m * g.trace_steps + n_exec) * 2;
        for (int j = 0; j < 6; ++j) { s_x[j] = st[j]; eo[j] = st[j]; }
        ao[0] = a0; ao[1] = a1;
        ++n_exec;
        for (int t = 0; t + 1 < a.T; ++t) { s_U[2 * t] = s_U[2 * t + 2]; s_U[2 * t + 1] = s_U[2 * t + 3]; }   // last control held
        t_acc += dt;
        if (t_acc > scan_time) { scan = 1; t_acc = 0.0; ++n_scans; }
        if (reached) { event = DITREE_MEV_GOAL; stop = 1; }      // after the scan: the driver's loop body ends before is_done
      }
      sh_scan = scan;
      sh_stop = stop;
    }
    __syncthreads();
    if (sh_scan) {
      // scan_and_update_maze (run_scenarios_with_lidar_DiTree.py:112-127): pose in fractional cell units (col, row), yaw in radians
      const double px = (s_x[0] + (double)cols / 2.0) / 1.0, py = ((double)rows / 2.0 - s_x[1]) / 1.0, yaw = s_x[2];
      double d, ex = 0.0, ey = 0.0;
      bool h;
      if (tid < DITREE_LIDAR_RAYS) lidar_ray(px, py, yaw, tid, tr, rows, cols, vis, &d, &ex, &ey, &h);
      __syncthreads();
      for (int i = tid; i < ncell; i += 256) {                                   // scanned[visited] = 2 (:121)
        if (vis[i]) { sc[i] = 2; dirty[i] = 1; vis[i] = 0; }
      }
      __syncthreads();
      if (tid < DITREE_LIDAR_RAYS) {                                             // end cells -> occupied (:119-122)
        const double fx = floor(ex), fy = floor(ey);
        if (fx >= 0.0 && fx < (double)cols && fy >= 0.0 && fy < (double)rows) {
          const int cidx = (int)fy * cols + (int)fx;
          kn[cidx] = 1;
          sc[cidx] = 1;
          dirty[cidx] = 1;
        }
      }
      __syncthreads();
    }
    if (sh_stop) break;
    // (thread 0 rewrites sh_scan / sh_stop / s_x only after the barriers of the next step's rollouts and sums)
  }
  __syncthreads();
  for (int i = tid; i < ncell; i += 256) {
    if (dirty[i]) {
      g.known[mcell + i] = (float)kn[i];
      g.scanned[mcell + i] = (float)sc[i];
    }
    if (g.refresh_codes != nullptr && m == g.refresh_mission) g.refresh_codes[i] = kn[i];
  }
  for (int i = tid; i < 2 * a.T; i += 256) U[i] = s_U[i];
  if (tid < 6) g.state_io[(size_t)m * 6 + tid] = s_x[tid];
  if (tid == 0) {
    g.t_acc_io[m] = t_acc;
    g.trials_io[m] = trials;
    res[0] = (double)event;
    res[1] = (double)calls;
    res[2] = (double)n_exec;
    res[3] = (double)n_scans;
    for (int j = 0; j < 5; ++j) res[4 + j] = s_last[j];
    for (int j = 9; j < DITREE_MPPI_MISSION_RESULT; ++j) res[j] = 0.0;
  }
}

}  // namespace

extern "C" int32_t ditree_mppi_missions(ditree_ctx* ctx, const ditree_mppi_params* p, int32_t M, const uint64_t* seed,
                                        const uint64_t* counter0, double* state_io, double* U_io, const double* path_xy,
                                        const int32_t* path_off, const int32_t* path_len, int32_t P_max, const double* goal_xy,
                                        float* known_maze, const float* true_maze, float* scanned_maze, int32_t rows,
                                        int32_t cols, const int32_t* max_steps, int32_t trace_steps,
                                        const int32_t* allowed_trials, const double* dt, const double* scan_time,
                                        double* t_acc_io, int32_t* trials_io, double* executed_states,
                                        double* executed_actions, double* result, int32_t refresh_mission, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!p || !seed || !counter0 || !state_io || !U_io || !path_xy || !path_off || !path_len || !goal_xy || !known_maze ||
      !true_maze || !scanned_maze || !max_steps || !allowed_trials || !dt || !scan_time || !t_acc_io || !trials_io ||
      !executed_states || !executed_actions || !result)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: null pointer");
  if (M < 1) return set_err(ctx, DITREE_E_ARG, "mppi_missions: M < 1 (at least one mission)");
  if (p->K < 1 || p->K > MISSION_MAX_K)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: 1 <= K <= 256 (one rollout per thread of the mission's work-group; larger "
                                      "controllers keep ditree_mppi_step)");
  if (p->T < 1 || p->T > MISSION_MAX_T) return set_err(ctx, DITREE_E_ARG, "mppi_missions: 1 <= T <= 64");
  if (P_max < 1 || P_max > MISSION_MAX_P)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: 1 <= P <= 4096 (the reference path is staged in LDS)");
  if (rows < 1 || cols < 1 || (int64_t)rows * cols > MISSION_MAX_CELLS)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: rows * cols <= 13104 (five byte maps of the maze stay in LDS)");
  if (p->k_offset != 0) return set_err(ctx, DITREE_E_ARG, "mppi_missions: k_offset != 0 (a sharded controller has no mission form)");
  if (trace_steps < 0 || trace_steps > DITREE_MPPI_MISSION_MAX_STEPS)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: 0 <= max_steps <= 2048 per launch (issue further launches for longer missions)");
  if (!(p->lambda > 0.0) || !(p->sigma[0] > 0.0) || !(p->sigma[1] > 0.0) || p->window_back < 0 || p->window_fwd < 0)
    return set_err(ctx, DITREE_E_ARG, "mppi_missions: bad argument (lambda, sigma > 0, windows >= 0)");
  if (refresh_mission >= M) return set_err(ctx, DITREE_E_ARG, "mppi_missions: refresh_mission >= M");
  if (refresh_mission >= 0 && (!ctx->maze || ctx->rows != rows || ctx->cols != cols))
    return set_err(ctx, DITREE_E_STATE, "mppi_missions: refresh_mission needs an uploaded maze of the same shape");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MppiArgs a;
  a.T = p->T; a.K = p->K; a.P = 0;
  a.lambda = p->lambda; a.s0 = p->sigma[0]; a.s1 = p->sigma[1];
  a.w_track = p->w_track; a.w_progress = p->w_progress; a.w_collision = p->w_collision; a.w_goal = p->w_goal;
  a.seed = 0; a.counter = 0;
  a.wback = p->window_back; a.wfwd = p->window_fwd;
  a.gx = 0.0; a.gy = 0.0;
  a.k0 = 0;
  MissionArgs g;
  g.seed = (const unsigned long long*)seed; g.counter0 = (const unsigned long long*)counter0;
  g.state_io = state_io; g.U_io = U_io;
  g.path = (const double2*)path_xy; g.path_off = path_off; g.path_len = path_len; g.goal = goal_xy;
  g.known = known_maze; g.truth = true_maze; g.scanned = scanned_maze;
  g.max_steps = max_steps; g.allowed_trials = allowed_trials; g.dt = dt; g.scan_time = scan_time;
  g.t_acc_io = t_acc_io; g.trials_io = trials_io;
  g.ex_states = executed_states; g.ex_actions = executed_actions; g.result = result;
  g.refresh_codes = refresh_mission >= 0 ? ctx->maze : nullptr;
  g.rows = rows; g.cols = cols; g.P_max = P_max; g.trace_steps = trace_steps; g.refresh_mission = refresh_mission;
  const size_t pad = ((size_t)rows * cols + 15) & ~(size_t)15;
  const size_t lds = (size_t)P_max * 16 + (size_t)a.T * 16 + 5 * pad;
  static bool attr_done[64] = {};
  if (lds > 64 * 1024 && (ctx->device >= 64 || !attr_done[ctx->device])) {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)mppi_mission_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
    if (ctx->device < 64) attr_done[ctx->device] = true;
  }
  hipLaunchKernelGGL(mppi_mission_kernel, dim3(M), dim3(256), lds, s, g, a);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}
