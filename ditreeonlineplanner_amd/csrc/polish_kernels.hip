// Plan polishing (include/ditree.h "plan polishing"): a found plan's action tape is shortened by sampled roll-outs.  Compiled
// with -ffp-contract=off like every unit that includes car_device.h: the collision and goal flags of a rolled tape must be
// those of the CPU oracle, and the roll-out launch and the commit launch must give one candidate the same bits.
//
// The design is the rollout kernels' (DESIGN.md section 5 "The rollout kernels against their roofline"): what a row costs is ONE
// sequential FP64 chain per lane -- Euler step -> norm -> two-ball test -- so one candidate per lane, one wave per SIMD, and
// nothing else inside the loop that waits.  The plan's maze is staged into LDS once per work-group.  The lanes of a wave walk
// the rows t together (a lane whose first perturbed row lies further on sits out until then: the wave runs max (T* - a) rows
// either way), so the incumbent's row U*[t] is one address for the whole wave -- a scalar / broadcast load through L2 -- and the
// noise of a block of `hold` rows is generated once per block.
#include "ditree_internal.h"
#include "mppi_device.h"

namespace {

constexpr int POLISH_BLK = 256;                 // lanes of a roll-out work-group: K is cut into slices of this many candidates
constexpr int POLISH_COMMIT_BLK = 64;

// what a work-group of the roll-out launch leaves for the commit launch: its best arriving candidate (k = -1: none) and how many arrived
struct PolishPartial {
  double tau;
  int32_t k, arriving;
};

struct PolishArgs {
  int capacity, K, N, hold, noise_blocks, slices;
  double s0, s1;
  unsigned long long seed;
  const SceneTable* table;                      // NULL: `maze` for every plan
  const unsigned char* maze;
  int rows, cols;
  const int32_t* scene;
  const double* x0;
  const double* goal;
  double* tape;
  int32_t* n_rows;
  double* states;
  double* arrival;
  int32_t* status;
  double* trace;
  const double* noise;
  const int32_t* first_row;
  PolishPartial* partial;
};

__device__ __forceinline__ double polish_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// the plan's maze -> LDS (whole work-group; ends with a barrier)
__device__ __forceinline__ void polish_stage_maze(const PolishArgs& g, int plan, unsigned char* lds, int& H, int& W) {
  const unsigned char* src = g.maze;
  H = g.rows;
  W = g.cols;
  if (g.table != nullptr) {
    const int id = min(max(g.scene[plan], 0), g.table->n - 1);       // validated on the host from scene_host
    const SceneRec sc = g.table->rec[id];
    src = scene_atlas(g.table) + sc.offset;
    H = sc.rows;
    W = sc.cols;
  }
  const int cells = min(H * W, DITREE_POLISH_MAX_CELLS);
  for (int i = threadIdx.x; i < cells; i += blockDim.x) lds[i] = src[i];
  __syncthreads();
}

// the rounds' goal norm: np.linalg.norm of a 2-vector
__device__ __forceinline__ double polish_goal_norm(const double* s, double gx, double gy) {
  const double ex = s[0] - gx, ey = s[1] - gy;
  return sqrt(fma(ey, ey, ex * ex));
}

// np.clip (NaN propagates), then the rounding to float32 that makes every stored row f32-exact
__device__ __forceinline__ double polish_action(double u, double lo, double hi) {
  const double c = u < lo ? lo : (u > hi ? hi : u);
  return (double)(float)c;
}

// One row of a rolled tape: the step, then the tests in the reference's order -> 0 goes on, 1 inside the radius, 2 collided.
__device__ __forceinline__ int polish_row(double* s, double u0, double u1, const unsigned char* mz, int H, int W, double gx,
                                          double gy, double& d) {
  car_euler_step(s, u0, u1);                    // clips the action as the env does (car_env.py:371)
  d = polish_goal_norm(s, gx, gy);
  return car_collides(s[0], s[1], s[2], mz, H, W) ? 2 : (d < 0.5 ? 1 : 0);
}

__device__ __forceinline__ int polish_first_row(const PolishArgs& g, int n, int k, int T) {
  if (g.first_row != nullptr) {
    const int r = g.first_row[(size_t)n * g.K + k];
    return r >= 0 ? r % T : max(T + r, 0);
  }
  unsigned long long h = splitmix64(g.seed ^ splitmix64((unsigned long long)n));
  h = splitmix64(h ^ ((unsigned long long)k * 0xD1B54A32D192ED03ull));
  return (int)(splitmix64(h ^ 0xA24BAED4963EE407ull) % (unsigned long long)T);
}

// Candidate k of iteration n on the incumbent (U, X, T rows): rows [a, T) from X[a].  -> 0 ran out of rows, 1 arrived (n_rows,
// tau set), 2 collided.  WAVE: the roll-out launch -- the loop starts at the wave-uniform row t0 <= a and ends when no lane of the
// wave is still rolling (`dead` lanes hold no candidate); else one thread re-rolls the winner and writes its rows into U / X
// in place (row t of U is read before it is written, X[a] before any row behind it).
template <bool WAVE>
__device__ __forceinline__ int polish_candidate(const PolishArgs& g, int n, int k, int T, int a, int t0, bool dead, double* U,
                                                double* X, const unsigned char* mz, int H, int W, double gx, double gy,
                                                int& n_rows, double& tau) {
  double s[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) s[j] = X[(size_t)a * 6 + j];
  double dprev = polish_goal_norm(s, gx, gy);
  double e0 = 0.0, e1 = 0.0;
  int eb = -1, res = dead ? 3 : 0;
  n_rows = 0;
  tau = polish_inf();
  for (int t = t0; t < T; ++t) {
    if constexpr (WAVE) {
      if (__ballot(res == 0) == 0) break;
    } else {
      if (res != 0) break;
    }
    const double ur0 = U[2 * (size_t)t], ur1 = U[2 * (size_t)t + 1];
    if (t >= a && res == 0) {
      const int b = t / g.hold;
      if (b != eb) {
        eb = b;
        if (g.noise != nullptr) {
          const size_t at = (((size_t)n * g.K + k) * g.noise_blocks + b) * 2;
          e0 = g.noise[at];
          e1 = g.noise[at + 1];
        } else {
          mppi_noise(g.seed, (unsigned long long)n, k, b, g.s0, g.s1, e0, e1);
        }
      }
      const double u0 = polish_action(ur0 + e0, -10.0, 10.0), u1 = polish_action(ur1 + e1, -2.0, 2.0);
      double d;
      const int r = polish_row(s, u0, u1, mz, H, W, gx, gy, d);
      if constexpr (!WAVE) {
        U[2 * (size_t)t] = u0;
        U[2 * (size_t)t + 1] = u1;
#pragma unroll
        for (int j = 0; j < 6; ++j) X[(size_t)(t + 1) * 6 + j] = s[j];
      }
      if (r == 2) {
        res = 2;
      } else if (r == 1) {
        res = 1;
        n_rows = t + 1;
        tau = (double)t + (dprev - 0.5) / (dprev - d);
      }
      dprev = d;
    }
  }
  return res == 3 ? 0 : res;
}

// Replay: one work-group per plan stages the maze, one thread rolls the input tape -- once without a store to find the status,
// then (status OK) again to write the states.
__global__ void __launch_bounds__(POLISH_COMMIT_BLK) polish_replay_kernel(PolishArgs g) {
  __shared__ unsigned char s_maze[DITREE_POLISH_MAX_CELLS];
  const int plan = blockIdx.x;
  int H, W;
  polish_stage_maze(g, plan, s_maze, H, W);
  if (threadIdx.x != 0) return;
  const double gx = g.goal[2 * plan], gy = g.goal[2 * plan + 1];
  const double* U = g.tape + (size_t)plan * g.capacity * 2;
  double* X = g.states + (size_t)plan * (g.capacity + 1) * 6;
  const int T = min(g.n_rows[plan], g.capacity);            // rows_host's value, validated on the host
  int status = DITREE_POLISH_NO_ARRIVAL, n_rows = 0;
  double tau = polish_inf();
  for (int pass = 0; pass < 2; ++pass) {
    double s[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = g.x0[(size_t)plan * 6 + j];
    double dprev = polish_goal_norm(s, gx, gy);
    if (pass == 0 && dprev < 0.5) {
      status = DITREE_POLISH_START_IN_GOAL;
      break;
    }
    if (pass == 1) {
#pragma unroll
      for (int j = 0; j < 6; ++j) X[j] = s[j];
    }
    const int rows = pass == 0 ? T : n_rows;
    for (int t = 0; t < rows; ++t) {
      const double u0 = U[2 * (size_t)t], u1 = U[2 * (size_t)t + 1];
      if (pass == 0 && (u0 != (double)(float)u0 || u1 != (double)(float)u1)) {
        status = DITREE_POLISH_NOT_F32;
        break;
      }
      double d;
      const int r = polish_row(s, u0, u1, s_maze, H, W, gx, gy, d);
      if (pass == 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) X[(size_t)(t + 1) * 6 + j] = s[j];
      } else if (r == 2) {
        status = DITREE_POLISH_COLLIDES;
        break;
      } else if (r == 1) {
        status = DITREE_POLISH_OK;
        n_rows = t + 1;
        tau = (double)t + (dprev - 0.5) / (dprev - d);
        break;
      }
      dprev = d;
    }
    if (status != DITREE_POLISH_OK) break;
  }
  g.status[plan] = status;
  if (status == DITREE_POLISH_OK) {
    g.n_rows[plan] = n_rows;
    g.arrival[2 * plan] = tau;
    g.arrival[2 * plan + 1] = tau;
  }
}

// (tau, k) minimum, ties to the lower k; k = -1 holds no candidate
__device__ __forceinline__ void polish_take_min(double& bt, int& bk, double ot, int ok) {
  if (ok >= 0 && (bk < 0 || ot < bt || (ot == bt && ok < bk))) {
    bt = ot;
    bk = ok;
  }
}

// The roll-out launch of iteration n: grid (K-slices, plans), one candidate per lane.
__global__ void __launch_bounds__(POLISH_BLK) polish_rollout_kernel(PolishArgs g, int n) {
  __shared__ unsigned char s_maze[DITREE_POLISH_MAX_CELLS];
  __shared__ PolishPartial s_part[POLISH_BLK / 64];
  const int plan = blockIdx.y;
  if (g.status[plan] != DITREE_POLISH_OK) return;           // the whole work-group: a refused plan runs nothing
  int H, W;
  polish_stage_maze(g, plan, s_maze, H, W);
  const double gx = g.goal[2 * plan], gy = g.goal[2 * plan + 1];
  double* U = g.tape + (size_t)plan * g.capacity * 2;
  double* X = g.states + (size_t)plan * (g.capacity + 1) * 6;
  const int T = g.n_rows[plan];
  const int k = blockIdx.x * POLISH_BLK + threadIdx.x;
  const bool live = k < g.K;
  const int a = live ? polish_first_row(g, n, k, T) : 0;
  int t0 = live ? a : T;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t0 = min(t0, __shfl_xor(t0, o));
  t0 = __builtin_amdgcn_readfirstlane(t0);
  int n_rows;
  double tau;
  const int res = polish_candidate<true>(g, n, k, T, a, t0, !live, U, X, s_maze, H, W, gx, gy, n_rows, tau);
  const bool arrived = live && res == 1;
  double bt = arrived ? tau : polish_inf();
  int bk = arrived ? k : -1;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ot = __shfl_xor(bt, o);
    const int ok = __shfl_xor(bk, o);
    polish_take_min(bt, bk, ot, ok);
  }
  const int cnt = __popcll(__ballot(arrived));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = PolishPartial{bt, bk, cnt};
  __syncthreads();
  if (threadIdx.x == 0) {
    PolishPartial p = s_part[0];
    for (int w = 1; w < POLISH_BLK / 64; ++w) {
      polish_take_min(p.tau, p.k, s_part[w].tau, s_part[w].k);
      p.arriving += s_part[w].arriving;
    }
    g.partial[(size_t)plan * g.slices + blockIdx.x] = p;
  }
}

// The commit launch of iteration n: one work-group per plan.  One thread reduces the slices in index order, applies the strict
// test and re-rolls the winner once -- the same polish_candidate, hence the same bits -- into tape, states, rows and the trace.
__global__ void __launch_bounds__(POLISH_COMMIT_BLK) polish_commit_kernel(PolishArgs g, int n) {
  __shared__ unsigned char s_maze[DITREE_POLISH_MAX_CELLS];
  const int plan = blockIdx.x;
  if (g.status[plan] != DITREE_POLISH_OK) return;
  int H, W;
  polish_stage_maze(g, plan, s_maze, H, W);
  if (threadIdx.x != 0) return;
  double bt = polish_inf();
  int bk = -1, arriving = 0;
  for (int sl = 0; sl < g.slices; ++sl) {
    const PolishPartial p = g.partial[(size_t)plan * g.slices + sl];
    polish_take_min(bt, bk, p.tau, p.k);
    arriving += p.arriving;
  }
  int T = g.n_rows[plan];
  double tau_star = g.arrival[2 * plan + 1];
  const bool accept = bk >= 0 && bt < tau_star;
  if (accept) {
    double* U = g.tape + (size_t)plan * g.capacity * 2;
    double* X = g.states + (size_t)plan * (g.capacity + 1) * 6;
    const int a = polish_first_row(g, n, bk, T);
    // the rule clips EVERY row of a candidate's tape: the rows in front of a are the incumbent's own, which the replay kept as
    // given -- a row outside the env's range (the planner's actions are the sampler's, unclipped) is stored clipped from here on
    for (int t = 0; t < 2 * a; t += 2) {
      U[t] = polish_action(U[t], -10.0, 10.0);
      U[t + 1] = polish_action(U[t + 1], -2.0, 2.0);
    }
    int n_rows;
    double tau;
    polish_candidate<false>(g, n, bk, T, a, a, false, U, X, s_maze, H, W, g.goal[2 * plan], g.goal[2 * plan + 1], n_rows, tau);
    T = n_rows;
    tau_star = tau;
    g.n_rows[plan] = T;
    g.arrival[2 * plan + 1] = tau_star;
  }
  double* tr = g.trace + ((size_t)plan * g.N + n) * DITREE_POLISH_TRACE;
  tr[0] = (double)bk;
  tr[1] = bt;
  tr[2] = accept ? 1.0 : 0.0;
  tr[3] = (double)T;
  tr[4] = tau_star;
  tr[5] = (double)arriving;
}

}  // namespace

extern "C" int32_t ditree_polish_plans(ditree_ctx* ctx, const ditree_polish* p, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!p) return set_err(ctx, DITREE_E_ARG, "polish_plans: null descriptor");
  if (p->state_dim != 6 || p->action_dim != 2)
    return set_err(ctx, DITREE_E_ARG, "polish_plans: the car only (state_dim 6, action_dim 2); the ant (29 / 8) is not built");
  if (p->n_plans < 1) return set_err(ctx, DITREE_E_ARG, "polish_plans: n_plans < 1 (at least one plan)");
  if (!p->x0 || !p->goal_xy || !p->tape || !p->rows || !p->rows_host || !p->states || !p->arrival || !p->status ||
      (p->N > 0 && !p->trace))
    return set_err(ctx, DITREE_E_ARG, "polish_plans: null pointer (x0, goal_xy, tape, rows, rows_host, states, arrival, status, trace)");
  if (p->K < 64 || p->K % 64 != 0)
    return set_err(ctx, DITREE_E_ARG, "polish_plans: K = " + std::to_string(p->K) + " is not a positive multiple of 64");
  if (p->N < 0) return set_err(ctx, DITREE_E_ARG, "polish_plans: N < 0 (iterations)");
  if (p->hold < 1) return set_err(ctx, DITREE_E_ARG, "polish_plans: hold < 1 (rows per noise block)");
  for (int d = 0; d < 2; ++d)
    if (!(p->sigma[d] >= 0.0) || !(p->sigma[d] <= 1.7976931348623157e308))
      return set_err(ctx, DITREE_E_ARG, "polish_plans: sigma must be finite and >= 0");
  if (p->capacity < 1) return set_err(ctx, DITREE_E_ARG, "polish_plans: capacity < 1");
  for (int i = 0; i < p->n_plans; ++i)
    if (p->rows_host[i] < 1 || p->rows_host[i] > p->capacity)
      return set_err(ctx, DITREE_E_ARG, "polish_plans: plan " + std::to_string(i) + " has a tape of " + std::to_string(p->rows_host[i]) +
                     " rows, outside 1 .. capacity = " + std::to_string(p->capacity));
  if (p->noise && (p->noise_blocks < 1 || (int64_t)p->noise_blocks * p->hold < p->capacity))
    return set_err(ctx, DITREE_E_ARG, "polish_plans: noise needs noise_blocks * hold >= capacity");
  if (p->scene) {
    if (ctx->n_scenes < 1) return set_err(ctx, DITREE_E_STATE, "polish_plans: no scene table uploaded (ditree_upload_scenes)");
    if (!p->scene_host) return set_err(ctx, DITREE_E_ARG, "polish_plans: scene needs scene_host");
    for (int i = 0; i < p->n_plans; ++i)
      if (p->scene_host[i] < 0 || p->scene_host[i] >= ctx->n_scenes)
        return set_err(ctx, DITREE_E_ARG, "polish_plans: plan " + std::to_string(i) + " has scene id " + std::to_string(p->scene_host[i]) +
                       ", out of range [0, " + std::to_string(ctx->n_scenes) + ")");
    if (ctx->max_scene_cells > DITREE_POLISH_MAX_CELLS)
      return set_err(ctx, DITREE_E_ARG, "polish_plans: a scene's maze holds more than " + std::to_string(DITREE_POLISH_MAX_CELLS) +
                     " cells (the maze is staged in LDS)");
  } else {
    if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "polish_plans: no maze uploaded (ditree_upload_maze)");
    if ((int64_t)ctx->rows * ctx->cols > DITREE_POLISH_MAX_CELLS)
      return set_err(ctx, DITREE_E_ARG, "polish_plans: the maze holds " + std::to_string((int64_t)ctx->rows * ctx->cols) +
                     " cells, more than " + std::to_string(DITREE_POLISH_MAX_CELLS) + " (the maze is staged in LDS)");
  }
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  PolishArgs g;
  g.capacity = p->capacity; g.K = p->K; g.N = p->N; g.hold = p->hold; g.noise_blocks = p->noise_blocks;
  g.slices = (p->K + POLISH_BLK - 1) / POLISH_BLK;
  g.s0 = p->sigma[0]; g.s1 = p->sigma[1];
  g.seed = p->seed;
  g.table = p->scene ? ctx->scene_tab : nullptr;
  g.maze = ctx->maze; g.rows = ctx->rows; g.cols = ctx->cols;
  g.scene = p->scene;
  g.x0 = p->x0; g.goal = p->goal_xy;
  g.tape = p->tape; g.n_rows = p->rows; g.states = p->states; g.arrival = p->arrival; g.status = p->status; g.trace = p->trace;
  g.noise = p->noise; g.first_row = p->first_row;
  const size_t need = (size_t)p->n_plans * g.slices * sizeof(PolishPartial);
  if (ctx->polish_partial_cap < need) {
    if (ctx->polish_partial) HIP_TRY(ctx, hipFree(ctx->polish_partial));
    ctx->polish_partial = nullptr;
    ctx->polish_partial_cap = 0;
    HIP_TRY(ctx, hipMalloc(&ctx->polish_partial, need));
    ctx->polish_partial_cap = need;
  }
  g.partial = (PolishPartial*)ctx->polish_partial;
  hipLaunchKernelGGL(polish_replay_kernel, dim3(p->n_plans), dim3(POLISH_COMMIT_BLK), 0, s, g);
  for (int n = 0; n < p->N; ++n) {
    hipLaunchKernelGGL(polish_rollout_kernel, dim3(g.slices, p->n_plans), dim3(POLISH_BLK), 0, s, g, n);
    hipLaunchKernelGGL(polish_commit_kernel, dim3(p->n_plans), dim3(POLISH_COMMIT_BLK), 0, s, g, n);
  }
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}
