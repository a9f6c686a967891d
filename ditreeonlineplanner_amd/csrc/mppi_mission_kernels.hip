// MPPI missions on the device (gfx950, FP64): the MPPI driver's control loop `run_scenarios_with_lidar_MPPI.py:417-452` --
// controller step, collision retries, trace, and a lidar scan with the known-maze update every `scan_time` -- as ONE launch.
// One work-group of 256 threads owns one mission from its first controller step to its terminating event; a launch takes a
// grid of M independent missions (a fleet).  A work-group needs nothing from any other: no grid-wide synchronisation, no
// co-residency requirement, any M.
//
// Compiled with -ffp-contract=off like mppi_kernels.hip and geom_kernels.hip.  BIT-EXACTNESS IS THE CONTRACT: a mission equals
// the same number of ditree_mppi_step / lidar scan / ditree_upload_maze calls bit for bit (tests/test_gpu_mppi_mission.py holds
// it to np.array_equal).  K <= 256 is the stepwise controller's one-slice case, and a controller step below is the calls the
// stepwise kernels make into mppi_device.h, in their order, with thread k on rollout k, one lane per rollout, a one-slice
// `partial` in LDS and k0 = 0; beta is an exact minimum (order-independent).  The scan is follow_plan_kernel's scan block
// (lidar_ray of lidar_device.h, end cells -> known / scanned, visited = 2).
// Every loop bound and every branch that contains a barrier is uniform over the work-group (flags in LDS, as
// follow_plan_kernel); the step count of a launch is bounded on the host (DITREE_MPPI_MISSION_MAX_STEPS).
#include "ditree_internal.h"
#include "lidar_device.h"
#include "mppi_device.h"

namespace {

constexpr int MISSION_MAX_K = 256;
constexpr int MISSION_MAX_CELLS = 13104;                 // five byte maps of 13 104 cells = 64 KB, as follow_plan_kernel
constexpr int MISSION_NACC = 3 + 2 * MPPI_MAX_T;

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

__global__ void __launch_bounds__(256) mppi_mission_kernel(MissionArgs g, MppiArgs a, CarTail cm) {
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
  __shared__ double s_rows[4][MISSION_NACC];                             // per-wave rows of the sums
  __shared__ double s_partial[MISSION_NACC];                             // the one slice
  __shared__ double s_sums[MISSION_NACC];                                // eta, sum w^2, collided rollouts, sum_k w_k eps[k, t, d]
  __shared__ double s_res[8];                                            // the last step's result [3..8): beta, eta, i0, collided
                                                                         // rollouts, effective samples
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
  if (tid < 8) s_res[tid] = 0.0;
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
    // ---- rollouts: thread k runs rollout k against the KNOWN maze
    const int i0 = block_nearest_index(s_path, a.P, x0[0], x0[1], 256, s_amin, s_aidx);
    const int k = tid;
    const bool live = k < a.K;
    double cost;
    int flag;
    car_rollout<1>(a, cm, s_path, s_U, kn, rows, cols, x0, i0, nullptr, k, 0, live, cost, flag);
    // ---- beta = min_k S_k
    const double mn = wave_min(live ? cost : __builtin_huge_val());
    if (lane0) s_wmin[wv] = mn;
    __syncthreads();
    const double beta = fmin(fmin(s_wmin[0], s_wmin[1]), fmin(s_wmin[2], s_wmin[3]));
    // ---- weights and sums: one trip of one slice per step t, the wave's row in registers until lane 0 stores it
    const double w = live ? mppi_weight(cost, beta, a.lambda) : 0.0;
    for (int t = 0; t < a.T; ++t) {
      double row[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (t == 0) mppi_accumulate_scalars(w, live && flag == 2, row);
      double e[2] = {0.0, 0.0};
      if (live && k > 0) CarModel::noise(a, cm, k, t, e);
      mppi_accumulate_noise<2>(w, e, row);
      if (lane0) {
        if (t == 0) { s_rows[wv][0] = row[0]; s_rows[wv][1] = row[1]; s_rows[wv][2] = row[2]; }
        s_rows[wv][3 + 2 * t] = row[3]; s_rows[wv][4 + 2 * t] = row[4];
      }
    }
    __syncthreads();
    if (tid < nacc) s_partial[tid] = mppi_row_tree(&s_rows[0][0], MISSION_NACC, tid);
    __syncthreads();
    mppi_sum_slices(s_partial, 1, nacc, s_sums);
    if (tid == 0) { s_res[3] = beta; s_res[5] = (double)i0; }
    mppi_apply(s_sums, 2 * a.T, s_U, s_res);
    // ---- execute: one env step with the first control against the KNOWN maze, then the driver's books
    if (tid == 0) {
      ++calls;
      double act[2], st[6];
      const int status = mppi_execute<CarModel>(a, cm, kn, rows, cols, s_x, st, s_U, act);
      int scan = 0, stop = 0;
      if (status == 2) {
        ++trials;
        if (trials >= allowed) { event = DITREE_MEV_TRIALS; stop = 1; }
      } else {
        trials = 0;
        double* eo = g.ex_states + ((size_t)m * g.trace_steps + n_exec) * 6;
        double* ao = g.ex_actions + ((size_t)m * g.trace_steps + n_exec) * 2;
        for (int j = 0; j < 6; ++j) { s_x[j] = st[j]; eo[j] = st[j]; }
        ao[0] = act[0]; ao[1] = act[1];
        ++n_exec;
        t_acc += dt;
        if (t_acc > scan_time) { scan = 1; t_acc = 0.0; ++n_scans; }
        if (status == 1) { event = DITREE_MEV_GOAL; stop = 1; }      // after the scan: the driver's loop body ends before is_done
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
    for (int j = 0; j < 5; ++j) res[4 + j] = s_res[3 + j];
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
  if (p->T < 1 || p->T > MPPI_MAX_T) return set_err(ctx, DITREE_E_ARG, "mppi_missions: 1 <= T <= 64");
  if (P_max < 1 || P_max > MPPI_MAX_P)
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
  a.lambda = p->lambda;
  a.w_track = p->w_track; a.w_progress = p->w_progress; a.w_collision = p->w_collision; a.w_goal = p->w_goal;
  a.seed = 0; a.counter = 0;
  a.wback = p->window_back; a.wfwd = p->window_fwd;
  a.gx = 0.0; a.gy = 0.0;
  a.k0 = 0;
  const CarTail cm{{p->sigma[0], p->sigma[1]}};
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
  hipLaunchKernelGGL(mppi_mission_kernel, dim3(M), dim3(256), lds, s, g, a, cm);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}
