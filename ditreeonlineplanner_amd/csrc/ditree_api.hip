// C-ABI entry points of libditree_hip.so (see include/ditree.h for the contract and the
// reference call sites each entry point replaces).
#include <dlfcn.h>

#include <algorithm>
#include <cmath>

#include <cstdio>
#include <cstring>

#include "ant_device.h"
#include "ditree_internal.h"

void launch_car_rollout_ex(const unsigned char* maze, int rows, int cols, double* state_io, const double* actions,
                           int64_t act_stride, int32_t* status_io, int B, int A, double gx, double gy,
                           double* states_out, ditree_strides states_stride, double* actions_out, ditree_strides actout_stride,
                           int32_t* steps_out, int64_t steps_stride, int32_t* chunks_run, double* prev_action_io,
                           uint8_t* has_prev_io, const int32_t* idx, int act_dense, hipStream_t s, const int32_t* budget,
                           int chunk_j, ChunkStrides cs = ChunkStrides{0, 0, 0}, const SceneArg* scenes = nullptr);
int denoise_run(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx, const float* local_map,
                const float* cond, int B, int K, const float* t0, const float* dt, const double* act_norm, double* actions,
                float* x_out, hipStream_t s);
int denoise_run_ddpm(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* noise_idx, const float* local_map,
                     const float* cond, int B, int K, const float* timesteps, const float* coef, const float* z, int64_t z_row,
                     int64_t z_step, const double* act_norm, double* actions, float* x_out, hipStream_t s);
void denoise_destroy(ditree_ctx* ctx);

// One sampler call of a round: K flow steps, or (coef != NULL) the DDPM loop with the round's (B, n_chunks, K, P, D) step noise.
// row_noise_stride: floats between the noise rows the index list (or the dense row number) addresses.
static int round_sampler(ditree_ctx* ctx, const float* noise, int64_t noise_stride, const int32_t* nidx, const float* lmap,
                         const float* cond, int n, int K, const float* t0, const float* dt, const float* coef, const float* z,
                         int64_t z_row, int64_t PD, const double* act_norm, double* actions, hipStream_t s) {
  if (coef)
    return denoise_run_ddpm(ctx, noise, noise_stride, nidx, lmap, cond, n, K, t0, coef, z, z_row, PD, act_norm, actions, nullptr, s);
  return denoise_run(ctx, noise, noise_stride, nidx, lmap, cond, n, K, t0, dt, act_norm, actions, nullptr, s);
}

int set_err(ditree_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// The pool scheduler of an early-exit round (car and ant; the rule is explained in expand_round_impl): rebuild the ready list
// (idx / nrow, furthest behind first), read its length back, take the largest multiple of `quantum` from its head -- everything,
// once less than one quantum is left -- and run `body(take)`, which launches one call for those rows, until nothing is ready.
// Calls and tile-waves of a drained round go to ctx->ee_calls / ee_waves (ditree_round_stats).
template <class Body>
static int run_ready_pool(ditree_ctx* ctx, const char* who, const ditree_round* round, const int32_t* budget, int nC, int quantum,
                          int32_t* idx, int32_t* nrow, hipStream_t s, Body body) {
  const int B = round->B;
  int calls = 0, waves = 0;
  for (;;) {
    launch_compact_ready(round->status, round->chunks_run, budget, nC, B, idx, nrow, ctx->alive_cnt, s);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->alive_cnt_host, ctx->alive_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const int n_ready = *ctx->alive_cnt_host;
    if (n_ready <= 0) break;
    const int take = n_ready < quantum ? n_ready : (n_ready / quantum) * quantum;
    if (++calls > nC * (B / quantum + 2) + 8)
      return set_err(ctx, DITREE_E_STATE, std::string(who) + ": early-exit scheduler did not drain");
    waves += (take + quantum - 1) / quantum;
    const int rc = body(take);
    if (rc) return rc;
  }
  ctx->ee_calls = calls;
  ctx->ee_waves = waves;
  return DITREE_OK;
}

// The rows one launch of a chunk half works on: candidates idx[0..n) (NULL: 0..n) whose noise rows are nrow[0..n) (NULL: the
// dense row number), all at chunk j -- or, j < 0 (the pool), each at the chunk its chunks_run counter names.
struct RowSet {
  const int32_t* idx;
  const int32_t* nrow;
  int n, j;
  size_t jo() const { return j < 0 ? 0 : (size_t)j; }     // the chunk offset the host adds to the round's arrays
  // noise rows per step of nrow: the pool's lists index the (B * n_chunks, ...) row view, a chunk loop's the candidates
  int64_t noise_rows(int n_chunks) const { return j < 0 ? 1 : n_chunks; }
};

// ---- round scratch (ditree_internal.h RoundScratch)
static hipError_t free_round_scratch(RoundScratch* rs) {
  void** ptrs[] = {(void**)&rs->state, (void**)&rs->hist, (void**)&rs->hist_n, (void**)&rs->prev_action, (void**)&rs->has_prev,
                   (void**)&rs->lmap,  (void**)&rs->cond, (void**)&rs->act,    (void**)&rs->idx,         (void**)&rs->nrow};
  hipError_t first = hipSuccess;
  for (void** p : ptrs) {
    const hipError_t e = *p ? hipFree(*p) : hipSuccess;
    if (first == hipSuccess) first = e;
    *p = nullptr;
  }
  rs->B = rs->lm = rs->P = 0;
  return first;
}

// Reserve `rs` for B candidates, an lm x lm local map and P predicted actions of a robot with S-wide states, D-wide actions and a
// C-wide conditioning vector; hist_rows > 0: that many history rows per candidate instead of the live state.  Sizes only grow, and
// growing waits for the device first: launches in flight may still read the old buffers.
static int ensure_round_scratch(ditree_ctx* ctx, RoundScratch* rs, int B, int lm, int P, int S, int D, int C, int hist_rows) {
  if (!ctx->alive_cnt) HIP_TRY(ctx, hipMalloc((void**)&ctx->alive_cnt, 16));
  if (!ctx->alive_cnt_host) HIP_TRY(ctx, hipHostMalloc((void**)&ctx->alive_cnt_host, 16, hipHostMallocDefault));
  if (B <= rs->B && lm <= rs->lm && P <= rs->P) return DITREE_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t nb = (size_t)std::max(B, rs->B), nl = (size_t)std::max(lm, rs->lm), np = (size_t)std::max(P, rs->P);
  HIP_TRY(ctx, free_round_scratch(rs));                   // B = lm = P = 0: a failed allocation below leaves "nothing reserved"
  const struct { void** p; size_t bytes; } bufs[] = {
      {(void**)&rs->state, hist_rows ? 0 : nb * S * sizeof(double)},
      {(void**)&rs->hist, nb * hist_rows * S * sizeof(double)},
      {(void**)&rs->hist_n, hist_rows ? nb * sizeof(int32_t) : 0},
      {(void**)&rs->prev_action, nb * D * sizeof(double)},
      {(void**)&rs->has_prev, nb},
      {(void**)&rs->lmap, nb * nl * nl * sizeof(float)},
      {(void**)&rs->cond, nb * C * sizeof(float)},
      {(void**)&rs->act, nb * np * D * sizeof(double)},
      {(void**)&rs->idx, nb * sizeof(int32_t)},
      {(void**)&rs->nrow, nb * sizeof(int32_t)}};
  for (const auto& b : bufs)
    if (b.bytes) HIP_TRY(ctx, hipMalloc(b.p, b.bytes));
  rs->B = (int)nb;
  rs->lm = (int)nl;
  rs->P = (int)np;
  return DITREE_OK;
}
static int ensure_car_scratch(ditree_ctx* ctx, int B, int lm, int P) { return ensure_round_scratch(ctx, &ctx->car, B, lm, P, 6, 2, 7, 0); }

// The nearest-node search among the first n_nodes nodes of one tree, or (f != NULL) for every query in its own tree of a forest,
// each up to its counter row's node count.  bd != NULL: the masked search of the "anytime_pruned" mode.  out_state != NULL: the
// chosen node's state, last action and flag are gathered into the three outputs.  nr != NULL: the near-parent rule
// (include/ditree.h "near parent") over the same candidates instead of the nearest node.  sp != NULL: only the active nodes of the
// sparse tree (include/ditree.h "sparse tree") are candidates.
static void search_nodes(const ditree_tree* tree, const ditree_forest* f, int n_nodes, const ditree_bound* bd, const double* queries,
                         int q_stride, int B, int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev,
                         hipStream_t s, const ditree_near* nr = nullptr, const ditree_sparse* sp = nullptr) {
  const NnArg a{queries, q_stride, B, (const double2*)tree->xy, out_state ? tree->state : nullptr, tree->last_action,
                tree->has_prev, tree->state_dim, tree->action_dim, out_idx, out_state, out_prev_action, out_has_prev,
                bd ? bd->key : nullptr, bd ? bd->cost : nullptr, sp ? sp->active : nullptr, nr ? nr->cost : nullptr,
                nr ? nr->radius : 0.0, nr ? nr->reach : 0.0};
  if (f) launch_nn(a, NnForest{f->off, f->n_trees, f->counters, f->tree_capacity, 0, false}, s);
  else launch_nn(a, NnTree{n_nodes, tree->counters}, s);
}

// What a call that runs the sampler refuses before anything is launched: an incomplete schedule (t0 with dt, or with ddpm_coef
// for the DDPM branch, whose K > 1 steps need step noise) and a loaded denoiser other than the one the caller's buffers are sized
// for (P, lm_n, D-wide actions, C-wide conditioning).  who: the entry point's name in the messages; noise_shape: the tail of the
// step-noise message; car_needs: the tail of the car's mismatch message (NULL: the ant's own text).
static int check_sampler(ditree_ctx* ctx, const char* who, const float* t0, const float* dt, const float* ddpm_coef,
                         const float* step_noise, int K, int P, int lm_n, int D, int C, const char* noise_shape,
                         const char* car_needs) {
  const std::string w(who);
  if (!t0 || (!dt && !ddpm_coef) || K < 1) return set_err(ctx, DITREE_E_ARG, w + ": flow schedule missing");
  if (ddpm_coef && !step_noise && K > 1) return set_err(ctx, DITREE_E_ARG, w + ": the DDPM branch needs step_noise" + noise_shape);
  // the scratch buffers are sized from the caller's P / lm_n; the denoiser strides them by ITS dimensions
  int32_t d5[5];
  if (ditree_denoise_dims(ctx, d5) != DITREE_OK) return DITREE_E_STATE;
  if (P == d5[0] && lm_n == d5[2] && d5[1] == D && d5[3] == C) return DITREE_OK;
  const std::string p0 = std::to_string(d5[0]), ad = std::to_string(d5[1]), map = std::to_string(d5[2]), cond = std::to_string(d5[3]);
  if (!car_needs)
    return set_err(ctx, DITREE_E_ARG, w + ": the loaded denoiser is not the ant network (P " + p0 + ", action_dim " + ad + ", cond " +
                   cond + ", map " + map + "; need P = params.P, 8, 97, map = params.lm_n)");
  return set_err(ctx, DITREE_E_ARG, w + ": pred_horizon " + std::to_string(P) + " / local map " + std::to_string(lm_n) +
                 " do not match the loaded denoiser (P " + p0 + ", action_dim " + ad + ", map " + map + ", cond " + cond + car_needs);
}

// checked copy of the caller's ant model into the kernels' argument block (also mppi_kernels.hip)
int fill_ant_model(ditree_ctx* ctx, const ditree_ant_model* m, AntModelArg* a) {
  if (!(m->h > 0.0) || !(m->frame_skip >= 1.0) || m->frame_skip > 64.0 || m->frame_skip != (double)(int)m->frame_skip)
    return set_err(ctx, DITREE_E_ARG, "ant model: need h > 0 and an integral frame_skip in 1..64");
  a->h = m->h; a->frame_skip = (int)m->frame_skip;
  a->k_act = m->k_act; a->k_spr = m->k_spr; a->k_dmp = m->k_dmp; a->k_lim = m->k_lim; a->hip_lim = m->hip_lim;
  a->ank_lo = m->ank_lo; a->ank_hi = m->ank_hi; a->ank_rest = m->ank_rest; a->contact_gain = m->contact_gain;
  a->leg_r = m->leg_r; a->k_push = m->k_push; a->c_lin = m->c_lin; a->z0 = m->z0; a->z_gain = m->z_gain; a->k_z = m->k_z;
  a->c_z = m->c_z; a->k_lift = m->k_lift; a->c_ang = m->c_ang; a->k_up = m->k_up; a->k_yaw = m->k_yaw; a->cphi = m->cphi;
  a->sphi = m->sphi;
  return DITREE_OK;
}

extern "C" {

int32_t ditree_version(void) { return DITREE_VERSION; }

#ifndef DITREE_BUILD_ID_STR
#define DITREE_BUILD_ID_STR "0000000000000000"          // a build outside ditreeonlineplanner_amd/build.py
#endif
// the marker is what build.py greps for in the binary; the id itself starts behind the '='
static const char k_build_marker[] = "DITREE_BUILD_ID=" DITREE_BUILD_ID_STR;
const char* ditree_build_id(void) { return k_build_marker + sizeof("DITREE_BUILD_ID=") - 1; }

int32_t ditree_ctx_create(int32_t device, ditree_ctx** out) {
  if (!out) return DITREE_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return DITREE_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return DITREE_E_HIP;
  ditree_ctx* c = new (std::nothrow) ditree_ctx();
  if (!c) return DITREE_E_NOMEM;
  c->device = device;
  *out = c;
  return DITREE_OK;
}

void ditree_ctx_destroy(ditree_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  ditree_comm_destroy(ctx);
  denoise_destroy(ctx);
  if (ctx->maze) hipFree(ctx->maze);
  free_round_scratch(&ctx->car);
  free_round_scratch(&ctx->ant);
  if (ctx->alive_cnt) hipFree(ctx->alive_cnt);
  if (ctx->alive_cnt_host) hipHostFree(ctx->alive_cnt_host);
  if (ctx->path_dev) hipFree(ctx->path_dev);
  if (ctx->mppi_partial) hipFree(ctx->mppi_partial);
  if (ctx->mppi_minkey) hipFree(ctx->mppi_minkey);
  if (ctx->polish_partial) hipFree(ctx->polish_partial);
  if (ctx->scene_tab) hipFree(ctx->scene_tab);
  if (ctx->row_scene) hipFree(ctx->row_scene);
  delete ctx;
}

const char* ditree_last_error(ditree_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int32_t ditree_upload_maze(ditree_ctx* ctx, const float* maze, int32_t rows, int32_t cols, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!maze || rows <= 0 || cols <= 0 || (int64_t)rows * cols > 60000)
    return set_err(ctx, DITREE_E_ARG, "upload_maze: need 0 < rows*cols <= 60000 (LDS-staged)");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t n = (size_t)rows * cols;
  if (ctx->maze_cap < n) {
    if (ctx->maze) HIP_TRY(ctx, hipFree(ctx->maze));
    ctx->maze = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->maze, n));
    ctx->maze_cap = n;
  }
  // host-side conversion to byte cell codes (same rule as maze_convert_kernel), then one async copy
  std::vector<unsigned char> codes(n);
  for (size_t i = 0; i < n; ++i) {
    float v = maze[i];
    int c = (int)v;
    codes[i] = (v == (float)c && c >= 0 && c < 256) ? (unsigned char)c : (unsigned char)255;
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->maze, codes.data(), n, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));       // `codes` is a temporary; the maze changes rarely
  ctx->rows = rows;
  ctx->cols = cols;
  return DITREE_OK;
}

int32_t ditree_nn_argmin(ditree_ctx* ctx, const double* queries, int32_t q_stride, int32_t B, const double* node_xy,
                         int32_t N, int32_t* out_idx, const double* node_state, const double* node_last_action,
                         const uint8_t* node_has_prev, double* out_state, double* out_prev_action,
                         uint8_t* out_has_prev, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (B == 0) return DITREE_OK;                       // empty batch: nothing to do (pointers may be null)
  if (!queries || !node_xy || !out_idx || B < 0 || N <= 0 || q_stride < 2)
    return set_err(ctx, DITREE_E_ARG, "nn_argmin: bad argument");
  if (node_state && (!node_last_action || !node_has_prev || !out_state || !out_prev_action || !out_has_prev))
    return set_err(ctx, DITREE_E_ARG, "nn_argmin: gather outputs incomplete");
  if (B == 0) return DITREE_OK;
  const NnArg a{queries, q_stride, B, (const double2*)node_xy, node_state, node_last_action, node_has_prev, 6, 2, out_idx,
                out_state, out_prev_action, out_has_prev, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0};
  launch_nn(a, NnTree{N, nullptr}, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

static int fill_axis(ditree_ctx* ctx, const double* axis, int n, AxisArg* a) {
  if (!axis || n <= 0 || n > DITREE_MAX_AXIS) return set_err(ctx, DITREE_E_ARG, "local map size must be 1..64");
  for (int i = 0; i < n; ++i) a->v[i] = axis[i];
  for (int i = n; i < DITREE_MAX_AXIS; ++i) a->v[i] = 0.0;
  return DITREE_OK;
}

int32_t ditree_local_map(ditree_ctx* ctx, const double* state, int32_t state_stride, const int32_t* active, int32_t B, int32_t n,
                         const double* axis, double s_global, int32_t scaled, float* out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "local_map: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state || !out || B < 0 || state_stride < 3) return set_err(ctx, DITREE_E_ARG, "local_map: bad argument");
  AxisArg a;
  int rc = fill_axis(ctx, axis, n, &a);
  if (rc) return rc;
  if (B == 0) return DITREE_OK;
  launch_local_map(ctx->maze, ctx->rows, ctx->cols, state, active, nullptr, B, n, a, s_global, scaled, out,
                   (hipStream_t)stream, state_stride);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

static void fill_norm(const double* norm, NormArg* nm) {
  for (int i = 0; i < 6; ++i) nm->obs_mean[i] = norm[i];
  for (int i = 0; i < 6; ++i) nm->obs_std[i] = norm[6 + i];
  for (int i = 0; i < 2; ++i) nm->act_mean[i] = norm[12 + i];
  for (int i = 0; i < 2; ++i) nm->act_std[i] = norm[14 + i];
}

static void fill_ant_norm(const double* norm, AntNormArg* nm) {
  for (int i = 0; i < 27; ++i) { nm->obs_mean[i] = norm[i]; nm->obs_std[i] = norm[27 + i]; }
  for (int i = 0; i < 8; ++i) { nm->act_mean[i] = norm[54 + i]; nm->act_std[i] = norm[62 + i]; }
}

int32_t ditree_cond_vector_ant(ditree_ctx* ctx, const double* obs, int32_t n_hist, const double* prev_action,
                               const uint8_t* has_prev, const double* cond_goal, int32_t B, const double* norm,
                               double local_map_size, float* out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (B == 0) return DITREE_OK;
  if (!obs || !prev_action || !has_prev || !cond_goal || !norm || !out || B < 0 || n_hist < 1 || n_hist > 3)
    return set_err(ctx, DITREE_E_ARG, "cond_vector_ant: bad argument (1 <= n_hist <= 3)");
  AntNormArg nm;
  fill_ant_norm(norm, &nm);
  launch_cond_vector_ant(obs, n_hist, nullptr, prev_action, has_prev, cond_goal, nullptr, B, nm, local_map_size, out, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_cond_vector(ditree_ctx* ctx, const double* state, const double* prev_action, const uint8_t* has_prev,
                           const double* cond_goal, int32_t B, const double* norm, double local_map_size, float* out,
                           void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (B == 0) return DITREE_OK;
  if (!state || !prev_action || !has_prev || !cond_goal || !norm || !out || B < 0)
    return set_err(ctx, DITREE_E_ARG, "cond_vector: bad argument");
  if (B == 0) return DITREE_OK;
  NormArg nm;
  fill_norm(norm, &nm);
  launch_cond_vector(state, prev_action, has_prev, cond_goal, nullptr, B, nm, local_map_size, out, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_car_rollout(ditree_ctx* ctx, double* state_io, const double* actions, int64_t act_stride,
                           int32_t* status_io, int32_t B, int32_t A, const double* goal_xy, double* states_out,
                           int64_t states_stride, double* actions_out, int64_t actout_stride, int32_t* steps_out,
                           double* prev_action_io, uint8_t* has_prev_io, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "car_rollout: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state_io || !actions || !status_io || !goal_xy || B < 0 || A <= 0 || act_stride < 2 * (int64_t)A)
    return set_err(ctx, DITREE_E_ARG, "car_rollout: bad argument");
  if (states_out && states_stride < 6 * (int64_t)(A + 1)) return set_err(ctx, DITREE_E_ARG, "car_rollout: states_stride");
  if (actions_out && actout_stride < 2 * (int64_t)A) return set_err(ctx, DITREE_E_ARG, "car_rollout: actout_stride");
  if (B == 0) return DITREE_OK;
  launch_car_rollout(ctx->maze, ctx->rows, ctx->cols, state_io, actions, act_stride, status_io, B, A, goal_xy[0],
                     goal_xy[1], states_out, states_stride, actions_out, actout_stride, steps_out, prev_action_io,
                     has_prev_io, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_car_rollout_ld(ditree_ctx* ctx, double* state_io, const double* actions, int64_t act_stride, int32_t* status_io,
                              int32_t B, int32_t A, const double* goal_xy, double* states_out, const ditree_strides* states_ld,
                              double* actions_out, const ditree_strides* actions_ld, int32_t* steps_out, double* prev_action_io,
                              uint8_t* has_prev_io, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "car_rollout: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state_io || !actions || !status_io || !goal_xy || B < 0 || A <= 0 || act_stride < 2 * (int64_t)A)
    return set_err(ctx, DITREE_E_ARG, "car_rollout: bad argument");
  const ditree_strides sl = states_ld ? *states_ld : ditree_strides{6 * (int64_t)(A + 1), 6, 1};
  const ditree_strides al = actions_ld ? *actions_ld : ditree_strides{2 * (int64_t)A, 2, 1};
  if (sl.cand < 1 || sl.row < 1 || sl.comp < 1 || al.cand < 1 || al.row < 1 || al.comp < 1)
    return set_err(ctx, DITREE_E_ARG, "car_rollout: strides must be positive");
  launch_car_rollout_ex(ctx->maze, ctx->rows, ctx->cols, state_io, actions, act_stride, status_io, B, A, goal_xy[0], goal_xy[1],
                        states_out, sl, actions_out, al, steps_out, 1, nullptr, prev_action_io, has_prev_io, nullptr, 1,
                        (hipStream_t)stream, nullptr, 0);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_ant_collision(ditree_ctx* ctx, const double* state, int32_t stride, int32_t B, double ball_radius, double s_global,
                             uint8_t* out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "ant_collision: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state || !out || B < 0 || stride < 7 || !(s_global > 0.0) || !(ball_radius >= 0.0))
    return set_err(ctx, DITREE_E_ARG, "ant_collision: bad argument (stride >= 7, s_global > 0)");
  launch_ant_collision(ctx->maze, ctx->rows, ctx->cols, state, stride, B, ball_radius, s_global, out, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_ant_rollout(ditree_ctx* ctx, const ditree_ant_model* model, double* state_io, const double* actions,
                           int64_t act_stride, const double* next_obs_tape, int64_t tape_stride, int32_t* status_io, int32_t B,
                           int32_t A, const double* desired_goal_xy, double goal_radius, double ball_radius, double s_global,
                           double* states_out, const ditree_strides* states_ld, double* actions_out,
                           const ditree_strides* actions_ld, int32_t* steps_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "ant_rollout: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state_io || !actions || !status_io || !desired_goal_xy || B < 0 || A <= 0 || act_stride < ANT_D * (int64_t)A ||
      !(s_global > 0.0))
    return set_err(ctx, DITREE_E_ARG, "ant_rollout: bad argument");
  if (!model && (!next_obs_tape || tape_stride < ANT_S * (int64_t)A))
    return set_err(ctx, DITREE_E_ARG, "ant_rollout: neither a model nor a next-observation tape of A rows");
  const ditree_strides sl = states_ld ? *states_ld : ditree_strides{ANT_S * (int64_t)(A + 1), ANT_S, 1};
  const ditree_strides al = actions_ld ? *actions_ld : ditree_strides{ANT_D * (int64_t)A, ANT_D, 1};
  if (sl.cand < 1 || sl.row < 1 || sl.comp < 1 || al.cand < 1 || al.row < 1 || al.comp < 1)
    return set_err(ctx, DITREE_E_ARG, "ant_rollout: strides must be positive");
  AntModelArg ma;
  if (model) { const int rc = fill_ant_model(ctx, model, &ma); if (rc) return rc; }
  launch_ant_rollout(ctx->maze, ctx->rows, ctx->cols, model ? &ma : nullptr, state_io, actions, act_stride, next_obs_tape,
                     tape_stride, status_io, B, A, desired_goal_xy[0], desired_goal_xy[1], goal_radius, ball_radius, s_global,
                     states_out, sl, actions_out, al, steps_out, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                     (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_lidar_scan(ditree_ctx* ctx, const double* poses, int32_t B, const float* maze, int32_t rows,
                          int32_t cols, double* dist, double* endpoints, uint8_t* hit, uint8_t* visited,
                          void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (B == 0) return DITREE_OK;
  if (!poses || !maze || !dist || !endpoints || !hit || B < 0 || rows <= 0 || cols <= 0 ||
      (int64_t)rows * cols > 30000)
    return set_err(ctx, DITREE_E_ARG, "lidar_scan: bad argument (rows*cols <= 30000)");
  if (B == 0) return DITREE_OK;
  launch_lidar_scan(poses, B, maze, rows, cols, dist, endpoints, hit, visited, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

static AheadArg ahead_samples() {               // np.linspace(0, 1.5, 30): arange(30) * (1.5 / 29), endpoint forced
  AheadArg a;
  const double step = 1.5 / 29.0;
  for (int i = 0; i < 30; ++i) a.t[i] = (double)i * step;
  a.t[29] = 1.5;
  return a;
}

int32_t ditree_obstacle_ahead(ditree_ctx* ctx, const double* state, int32_t stride, int32_t B, uint8_t* out,
                              void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "obstacle_ahead: no maze uploaded");
  if (B == 0) return DITREE_OK;
  if (!state || !out || B < 0 || stride < 3) return set_err(ctx, DITREE_E_ARG, "obstacle_ahead: bad argument");
  const AheadArg a = ahead_samples();
  launch_obstacle_ahead(ctx->maze, ctx->rows, ctx->cols, state, stride, B, a, out, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_follow_plan(ditree_ctx* ctx, double* state_io, const float* actions, int32_t n_actions,
                           int32_t action_idx, const float* path_xy, int32_t P, float* known_maze,
                           const float* true_maze, float* scanned_maze, const double* goal_xy, double dt,
                           double scan_time, double* executed, int32_t* result, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "follow_plan: no maze uploaded");
  if (!state_io || !known_maze || !true_maze || !scanned_maze || !goal_xy || !result || n_actions < 0 ||
      action_idx < 0 || action_idx > n_actions || P < 0 || (n_actions > 0 && !actions) || (P > 0 && !path_xy) ||
      (n_actions > action_idx && !executed))
    return set_err(ctx, DITREE_E_ARG, "follow_plan: bad argument");
  if (5 * (((size_t)ctx->rows * ctx->cols + 15) & ~(size_t)15) > 64 * 1024)
    return set_err(ctx, DITREE_E_ARG, "follow_plan: maze too large for the LDS-resident loop (<= 13104 cells)");
  launch_follow_plan(state_io, actions, n_actions, action_idx, path_xy, P, known_maze, true_maze, scanned_maze,
                     ctx->maze, ctx->rows, ctx->cols, goal_xy[0], goal_xy[1], dt, scan_time, executed, result,
                     (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_path_after_obstacle(ditree_ctx* ctx, const float* path, int32_t stride, int32_t P, const double* cur_xy,
                                   int32_t f32_state, int32_t* out2, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "path_after_obstacle: no maze uploaded");
  if (!path || !cur_xy || !out2 || P < 1 || stride < 2) return set_err(ctx, DITREE_E_ARG, "path_after_obstacle: bad argument");
  launch_path_after_obstacle(path, stride, P, cur_xy[0], cur_xy[1], f32_state != 0, ctx->maze, ctx->rows, ctx->cols, out2,
                             (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

static int check_tree(ditree_ctx* ctx, const ditree_tree* t);

int32_t ditree_fallback_select(ditree_ctx* ctx, const ditree_tree* tree, int32_t n_nodes, const double* goal_xy,
                               const double* path, int32_t P, int32_t* out_node, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  if (!goal_xy || !out_node || n_nodes < 1 || n_nodes > tree->capacity || (path && P <= 0))
    return set_err(ctx, DITREE_E_ARG, "fallback_select: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const double* pd = nullptr;
  if (path) {
    if (P > ctx->path_cap) {
      if (ctx->path_dev) HIP_TRY(ctx, hipFree(ctx->path_dev));
      ctx->path_dev = nullptr;
      HIP_TRY(ctx, hipMalloc((void**)&ctx->path_dev, (size_t)P * 2 * sizeof(double)));
      ctx->path_cap = P;
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->path_dev, path, (size_t)P * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));            // `path` is caller-owned host memory
    pd = ctx->path_dev;
  }
  launch_fallback_select(*tree, n_nodes, goal_xy[0], goal_xy[1], pd, P, out_node, s);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

static int check_tree(ditree_ctx* ctx, const ditree_tree* t) {
  if (!t || !t->state || !t->xy || !t->parent || !t->last_action || !t->has_prev || !t->num_visit ||
      !t->edge_states || !t->edge_actions || !t->edge_nstates || !t->edge_nactions || !t->counters ||
      t->capacity <= 0 || t->n_chunks <= 0 || t->A <= 0)
    return set_err(ctx, DITREE_E_ARG, "tree descriptor incomplete");
  if (t->state_dim < 3 || t->state_dim > 64 || t->action_dim < 1 || t->action_dim > 32)
    return set_err(ctx, DITREE_E_ARG, "tree: state_dim must be 3..64 and action_dim 1..32 (car 6 / 2, ant 29 / 8)");
  if ((t->hist == nullptr) != (t->hist_n == nullptr)) return set_err(ctx, DITREE_E_ARG, "tree: hist and hist_n come together");
  return DITREE_OK;
}
static int check_round(ditree_ctx* ctx, const ditree_round* r) {
  if (!r || r->B < 0 || !r->parent || !r->status || !r->chunks_run || !r->end_state || !r->states || !r->actions ||
      !r->chunk_steps || !r->node_id)
    return set_err(ctx, DITREE_E_ARG, "round descriptor incomplete");
  return DITREE_OK;
}

// The tail of every accept entry point, after its own checks: the accept of one tree, or (f != NULL, validated by the caller)
// of a forest.  cost: the cost column of the best and the bounded mode (bounded: bound->cost), NULL in the first mode.
static int accept_impl(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, const ditree_round* round, AcceptMode mode,
                       int emulate_sticky, int32_t* cost, const ditree_bound* bound, void* stream,
                       const ditree_sparse* sparse = nullptr) {
  if (round->B == 0) return DITREE_OK;
  const TreeSet ts = f ? TreeSet{f->off, f->counters, f->n_trees, f->tree_capacity}
                       : TreeSet{nullptr, tree->counters, 1, tree->capacity};
  launch_accept(*tree, *round, ts, mode, emulate_sticky, cost, bound, ctx->maze, ctx->rows, ctx->cols, ahead_samples(),
                (hipStream_t)stream, sparse);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// ---- re-planning on a kept tree (include/ditree.h): every host-side check runs before anything is launched; the node count
// and the anchor's row counts live on the device and are checked there (dst->counters[0]).
int32_t ditree_tree_rebase(ditree_ctx* ctx, const ditree_tree* src, const ditree_tree* dst, int32_t anchor,
                           const double* root_state, int32_t drop_states, int32_t drop_actions, const int32_t* cost_src,
                           int32_t* cost_dst, int32_t* scratch, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_tree(ctx, src);
  if (rc) return rc;
  rc = check_tree(ctx, dst);
  if (rc) return rc;
  if (src->hist || dst->hist || src->state_dim != 6 || src->action_dim != 2)
    return set_err(ctx, DITREE_E_ARG, "tree_rebase: the car (a tree with state_dim 6, action_dim 2 and no hist)");
  if (src->n_chunks != dst->n_chunks || src->A != dst->A || src->state_dim != dst->state_dim || src->action_dim != dst->action_dim)
    return set_err(ctx, DITREE_E_ARG, "tree_rebase: src and dst differ in shape");
  if (dst->capacity < src->capacity) return set_err(ctx, DITREE_E_ARG, "tree_rebase: dst->capacity below src->capacity");
  if ((src->obstacle_ahead == nullptr) != (dst->obstacle_ahead == nullptr))
    return set_err(ctx, DITREE_E_ARG, "tree_rebase: obstacle_ahead in one tree only");
  const void* a[] = {src->state, src->xy, src->parent, src->last_action, src->has_prev, src->num_visit, src->edge_states,
                     src->edge_actions, src->edge_nstates, src->edge_nactions, src->obstacle_ahead, src->edge_owner,
                     src->counters, cost_src};
  const void* b[] = {dst->state, dst->xy, dst->parent, dst->last_action, dst->has_prev, dst->num_visit, dst->edge_states,
                     dst->edge_actions, dst->edge_nstates, dst->edge_nactions, dst->obstacle_ahead, dst->edge_owner,
                     dst->counters, cost_dst};
  for (const void* p : a)
    for (const void* q : b)
      if (p != nullptr && p == q) return set_err(ctx, DITREE_E_ARG, "tree_rebase: src and dst share a buffer");
  if (anchor < 0 || anchor >= src->capacity) return set_err(ctx, DITREE_E_ARG, "tree_rebase: anchor out of range");
  if (!root_state && (drop_states != 0 || drop_actions != 0))
    return set_err(ctx, DITREE_E_ARG, "tree_rebase: drop counts belong to a root_state");
  if ((cost_src == nullptr) != (cost_dst == nullptr))
    return set_err(ctx, DITREE_E_ARG, "tree_rebase: cost_src and cost_dst come together");
  if (!scratch) return set_err(ctx, DITREE_E_ARG, "tree_rebase: scratch missing");
  if (!ctx->maze) return set_err(ctx, DITREE_E_STATE, "tree_rebase: no maze uploaded");
  RebaseArg arg{anchor, root_state != nullptr, drop_states, drop_actions, {0}};
  if (root_state)
    for (int k = 0; k < src->state_dim; ++k) arg.root[k] = root_state[k];
  launch_tree_rebase(*src, *dst, arg, cost_src, cost_dst, scratch, ctx->maze, ctx->rows, ctx->cols, ahead_samples(),
                     (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_round_pack(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, double* records_out,
                          void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  rc = check_round(ctx, round);
  if (rc) return rc;
  if (round->B == 0) return DITREE_OK;
  if (!records_out) return set_err(ctx, DITREE_E_ARG, "round_pack: no output");
  launch_round_pack(*tree, *round, records_out, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_record_doubles(const ditree_tree* tree) { return tree ? record_doubles(*tree) : DITREE_E_ARG; }

int32_t ditree_round_unpack(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const double* records,
                            void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  rc = check_round(ctx, round);
  if (rc) return rc;
  if (round->B == 0) return DITREE_OK;
  if (!records || !round->last_action || !round->first_action)
    return set_err(ctx, DITREE_E_ARG, "round_unpack: records and the round's last_action / first_action arrays are required");
  if (tree->hist && (!round->hist || !round->hist_n))
    return set_err(ctx, DITREE_E_ARG, "round_unpack: a tree with `hist` needs the round's hist / hist_n arrays");
  launch_round_unpack(*tree, *round, records, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// ---- RCCL communicator inside the ctx.  librccl is opened at run time (a host that already maps one -- torch does --
// keeps using that copy), so the library has no link-time dependency on it.
namespace {
struct RcclUniqueId { char internal[128]; };
using fn_get_id = int (*)(RcclUniqueId*);
using fn_init_rank = int (*)(void**, int, RcclUniqueId, int);
using fn_allgather = int (*)(const void*, void*, size_t, int, void*, hipStream_t);
using fn_destroy = int (*)(void*);
using fn_errstr = const char* (*)(int);
void* rccl_open(ditree_ctx* ctx) {
  if (ctx->rccl_lib) return ctx->rccl_lib;
  const char* names[] = {"librccl.so.1", "librccl.so"};
  for (const char* n : names)
    if ((ctx->rccl_lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) return ctx->rccl_lib;       // already mapped by the host
  for (const char* n : names)
    if ((ctx->rccl_lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) return ctx->rccl_lib;
  const char* rocm[] = {"/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : rocm)
    if ((ctx->rccl_lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) return ctx->rccl_lib;
  return nullptr;
}
int rccl_fail(ditree_ctx* ctx, const char* what, int rc) {
  fn_errstr es = (fn_errstr)dlsym(ctx->rccl_lib, "ncclGetErrorString");
  return set_err(ctx, DITREE_E_HIP, std::string(what) + ": " + (es ? es(rc) : "rccl error") + " (" + std::to_string(rc) + ")");
}
}  // namespace

int32_t ditree_comm_unique_id(ditree_ctx* ctx, uint8_t* id128) {
  if (!ctx) return DITREE_E_ARG;
  if (!id128) return set_err(ctx, DITREE_E_ARG, "comm_unique_id: no output");
  if (!rccl_open(ctx)) return set_err(ctx, DITREE_E_STATE, std::string("comm: cannot open librccl: ") + dlerror());
  fn_get_id f = (fn_get_id)dlsym(ctx->rccl_lib, "ncclGetUniqueId");
  if (!f) return set_err(ctx, DITREE_E_STATE, "comm: ncclGetUniqueId not found");
  RcclUniqueId id;
  const int rc = f(&id);
  if (rc) return rccl_fail(ctx, "ncclGetUniqueId", rc);
  std::memcpy(id128, id.internal, 128);
  return DITREE_OK;
}

int32_t ditree_comm_init(ditree_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id128) {
  if (!ctx) return DITREE_E_ARG;
  if (!id128 || world < 1 || rank < 0 || rank >= world) return set_err(ctx, DITREE_E_ARG, "comm_init: bad argument");
  if (ctx->comm) return set_err(ctx, DITREE_E_STATE, "comm_init: communicator already exists");
  if (!rccl_open(ctx)) return set_err(ctx, DITREE_E_STATE, std::string("comm: cannot open librccl: ") + dlerror());
  fn_init_rank f = (fn_init_rank)dlsym(ctx->rccl_lib, "ncclCommInitRank");
  if (!f) return set_err(ctx, DITREE_E_STATE, "comm: ncclCommInitRank not found");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  RcclUniqueId id;
  std::memcpy(id.internal, id128, 128);
  const int rc = f(&ctx->comm, world, id, rank);
  if (rc) { ctx->comm = nullptr; return rccl_fail(ctx, "ncclCommInitRank", rc); }
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  return DITREE_OK;
}

int32_t ditree_allgather_nodes(ditree_ctx* ctx, const double* send, double* recv, int64_t count_doubles, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (!ctx->comm) return set_err(ctx, DITREE_E_STATE, "allgather_nodes: call ditree_comm_init first");
  if (!send || !recv || count_doubles < 0) return set_err(ctx, DITREE_E_ARG, "allgather_nodes: bad argument");
  if (count_doubles == 0) return DITREE_OK;
  fn_allgather f = (fn_allgather)dlsym(ctx->rccl_lib, "ncclAllGather");
  if (!f) return set_err(ctx, DITREE_E_STATE, "comm: ncclAllGather not found");
  const int rc = f(send, recv, (size_t)count_doubles, 8 /* ncclDouble */, ctx->comm, (hipStream_t)stream);
  if (rc) return rccl_fail(ctx, "ncclAllGather", rc);
  return DITREE_OK;
}

int32_t ditree_comm_destroy(ditree_ctx* ctx) {
  if (!ctx) return DITREE_E_ARG;
  if (ctx->comm) {
    fn_destroy f = (fn_destroy)dlsym(ctx->rccl_lib, "ncclCommDestroy");
    if (f) f(ctx->comm);
    ctx->comm = nullptr;
  }
  return DITREE_OK;
}

static SceneArg scene_arg(const ditree_ctx* ctx) { return SceneArg{ctx->scene_tab, ctx->atlas_cells, ctx->max_scene_cells}; }

// The (B,) row -> scene scratch of scene-forest rounds; its address lives in the device scene table's header.
static int ensure_row_scene(ditree_ctx* ctx, int B, hipStream_t s) {
  if (B <= ctx->row_scene_cap) return DITREE_OK;
  HIP_TRY(ctx, hipStreamSynchronize(s));                // the previous scratch may still be read
  if (ctx->row_scene) HIP_TRY(ctx, hipFree(ctx->row_scene));
  ctx->row_scene = nullptr;
  ctx->row_scene_cap = 0;
  HIP_TRY(ctx, hipMalloc((void**)&ctx->row_scene, (size_t)B * sizeof(int32_t)));
  ctx->row_scene_cap = B;
  HIP_TRY(ctx, hipMemcpyAsync(&ctx->scene_tab->row_scene, &ctx->row_scene, sizeof(ctx->row_scene), hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));                // the source is a ctx field that the next growth overwrites
  return DITREE_OK;
}

// The scene argument of a scene forest's round (forest and tree_scene validated by the caller): the table, and every row's scene
// id written into the row -> scene scratch.
static int round_scenes(ditree_ctx* ctx, const ditree_forest* f, const int32_t* tree_scene, int B, hipStream_t s, SceneArg* sc) {
  *sc = scene_arg(ctx);
  if (B == 0) return DITREE_OK;
  const int rc = ensure_row_scene(ctx, B, s);
  if (rc) return rc;
  launch_row_scene(f->off, f->n_trees, tree_scene, B, ctx->row_scene, s);
  return DITREE_OK;
}

// ---- BASELINE config 3: the ant round (include/ditree.h "One expansion round of the ANT").
// scenes (an ant scene forest, validated by the caller): each row's maze and desired goal come from the scene table, so neither
// an uploaded single maze nor p->desired_goal is required.
static int check_ant_round(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_ant_round_params* p,
                           int need_sampler, bool scenes = false) {
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  rc = check_round(ctx, round);
  if (rc) return rc;
  if (!scenes && !ctx->maze) return set_err(ctx, DITREE_E_STATE, "expand_round_ant: no maze uploaded");
  if (tree->state_dim != ANT_S || tree->action_dim != ANT_D || !tree->hist)
    return set_err(ctx, DITREE_E_ARG, "expand_round_ant: the tree must have state_dim 29, action_dim 8 and hist / hist_n");
  if (!p || !p->cond_goal || !p->norm || (!scenes && !p->desired_goal) || !p->axis || !(p->s_global > 0.0) || p->P < tree->A)
    return set_err(ctx, DITREE_E_ARG, "expand_round_ant: bad parameters");
  if (!need_sampler) return DITREE_OK;
  if (!p->noise && !p->inject_actions) return set_err(ctx, DITREE_E_ARG, "expand_round_ant: neither noise nor inject_actions");
  if (p->inject_actions) return DITREE_OK;
  return check_sampler(ctx, "expand_round_ant", p->t0, p->dt, p->ddpm_coef, p->step_noise, p->K, p->P, p->lm_n, ANT_D, 97, "", nullptr);
}

// The begin step of an ant round on one tree, or (f != NULL, validated by the caller) on a forest: only the nearest-node search
// differs -- the first p->n_nodes nodes, or each candidate's own tree up to its counter row's node count.
static int ant_round_begin_impl(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, const ditree_round* round,
                                const ditree_ant_round_params* p, void* stream, bool scenes = false) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_ant_round(ctx, tree, round, p, 0, scenes);
  if (rc) return rc;
  if (!p->samples || (!f && (p->n_nodes <= 0 || p->n_nodes > tree->capacity)))
    return set_err(ctx, DITREE_E_ARG, "ant_round_begin: samples / n_nodes");
  const int B = round->B;
  if (B == 0) return DITREE_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  RoundScratch& a = ctx->ant;
  rc = ensure_round_scratch(ctx, &a, B, p->lm_n, p->P, ANT_S, ANT_D, 97, 3);
  if (rc) return rc;
  launch_round_begin(round->status, round->chunks_run, round->chunk_steps, B, tree->n_chunks, s);
  // RRT.py:141-147: nearest node -> curr_state (the live state of the round: round->end_state), prev_actions, prev_states
  search_nodes(tree, f, p->n_nodes, nullptr, p->samples, ANT_S, B, round->parent, round->end_state, a.prev_action, a.has_prev, s);
  launch_ant_gather_hist(round->parent, tree->hist, tree->hist_n, B, a.hist, a.hist_n, s);   // parents are global ids
  ctx->ant_n_run = B;
  ctx->ant_run_idx = nullptr;
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_ant_round_begin(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                               const ditree_ant_round_params* p, void* stream) {
  return ant_round_begin_impl(ctx, tree, nullptr, round, p, stream);
}

// A chunk of the ant round is a sample half and a step half, each on a row set (RowSet).  The plain round runs them for
// j = 0..n_chunks-1 on every row, the pool at j = -1 on the ready list, and the stepped API hands the caller's simulator the
// actions in between.
// The sample half: local map -> conditioning -> sampler, or the action tape.  scp != NULL (an ant scene forest): the local map is
// cut from each row's own scene.
static int ant_sample_half(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_ant_round_params* p,
                           const SceneArg* scp, const RowSet& rows, hipStream_t s) {
  if (rows.n == 0) return DITREE_OK;
  RoundScratch& a = ctx->ant;
  const int nC = tree->n_chunks, A = tree->A, P = p->P;
  const size_t jo = rows.jo();
  // A chunk loop leaves the chunk's actions in round->actions, where the caller of the stepped API reads them between the halves;
  // the pool's rollout takes them from where they are.
  double* chunk_actions = rows.j < 0 ? nullptr : round->actions + jo * A * ANT_D;
  const int64_t ac_stride = (int64_t)nC * A * ANT_D;
  if (p->inject_actions && chunk_actions)
    launch_ant_copy_actions(p->inject_actions + jo * P * ANT_D, (int64_t)nC * P * ANT_D, 0, rows.idx, round->status, rows.n, A,
                            chunk_actions, ac_stride, s);
  if (p->inject_actions && !p->cond_out) {               // action tapes need neither the map nor the conditioning
    HIP_TRY(ctx, hipGetLastError());
    return DITREE_OK;
  }
  AxisArg ax;
  int rc = fill_axis(ctx, p->axis, p->lm_n, &ax);
  if (rc) return rc;
  AntNormArg nm;
  fill_ant_norm(p->norm, &nm);
  // RRT.py:158-166: the local map is cut at the chunk's start state (x, y, element 2)
  if (scp)
    launch_local_map_scenes(*scp, round->end_state, round->status, rows.idx, rows.n, p->lm_n, ax, p->s_global, a.lmap, s, ANT_S);
  else
    launch_local_map(ctx->maze, ctx->rows, ctx->cols, round->end_state, round->status, rows.idx, rows.n, p->lm_n, ax, p->s_global, 1,
                     a.lmap, s, ANT_S);
  launch_cond_vector_ant(a.hist, 3, a.hist_n, a.prev_action, a.has_prev, p->cond_goal, rows.idx, rows.n, nm, p->lm_size, a.cond, s);
  if (p->cond_out) {
    if (rows.idx) return set_err(ctx, DITREE_E_ARG, "expand_round_ant: cond_out is a test output of rounds without early_exit");
    HIP_TRY(ctx, hipMemcpy2DAsync(p->cond_out + jo * 97, (size_t)nC * 97 * sizeof(float), a.cond, 97 * sizeof(float),
                                  97 * sizeof(float), (size_t)rows.n, hipMemcpyDeviceToDevice, s));
  }
  if (p->inject_actions) {
    HIP_TRY(ctx, hipGetLastError());
    return DITREE_OK;
  }
  // start noise rows of (P, 8) and, for the DDPM branch, step noise rows of (K, P, 8)
  const int64_t nrows = rows.noise_rows(nC);
  rc = round_sampler(ctx, p->noise + jo * P * ANT_D, nrows * P * ANT_D, rows.nrow, a.lmap, a.cond, rows.n, p->K, p->t0, p->dt,
                     p->ddpm_coef, p->step_noise ? p->step_noise + jo * p->K * P * ANT_D : nullptr, nrows * p->K * P * ANT_D,
                     (int64_t)P * ANT_D, p->norm + 54, a.act, s);
  if (rc) return rc;
  if (chunk_actions)
    launch_ant_copy_actions(a.act, (int64_t)P * ANT_D, 1, rows.idx, round->status, rows.n, A, chunk_actions, ac_stride, s);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// The step half: the rollout of the chunk's A actions.  model != NULL: the stand-in dynamics; else `tape` holds the observations,
// (A, 29) rows tape_stride doubles apart per candidate, already offset to chunk j by the caller (the pool: the round's whole tape).
static int ant_step_half(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_ant_round_params* p,
                         const SceneArg* scp, const AntModelArg* model, const double* tape, int64_t tape_stride, const RowSet& rows,
                         hipStream_t s) {
  if (rows.n == 0) return DITREE_OK;
  RoundScratch& a = ctx->ant;
  const int nC = tree->n_chunks, A = tree->A, P = p->P;
  const size_t jo = rows.jo();
  const double* acts = p->inject_actions ? p->inject_actions + jo * P * ANT_D : a.act;    // (B, n_chunks, P, 8) by candidate, or dense
  const int64_t act_stride = p->inject_actions ? (int64_t)nC * P * ANT_D : (int64_t)P * ANT_D;
  const int64_t st_stride = (int64_t)nC * (A + 1) * ANT_S, ac_stride = (int64_t)nC * A * ANT_D;
  const double gx = scp ? 0.0 : p->desired_goal[0], gy = scp ? 0.0 : p->desired_goal[1];   // scenes: each row's own goal
  // rows at different chunks: the per-chunk strides the kernel then adds itself
  const AntChunkStrides cs = rows.j < 0 ? AntChunkStrides{(int64_t)(A + 1) * ANT_S, (int64_t)A * ANT_D, (int64_t)P * ANT_D, (int64_t)A * ANT_S}
                                        : AntChunkStrides{0, 0, 0, 0};
  launch_ant_rollout(ctx->maze, ctx->rows, ctx->cols, model, round->end_state, acts, act_stride, tape, tape_stride, round->status,
                     rows.n, A, gx, gy, p->goal_radius, p->ball_radius, p->s_global, round->states + jo * (A + 1) * ANT_S,
                     ditree_strides{st_stride, ANT_S, 1}, round->actions + jo * A * ANT_D, ditree_strides{ac_stride, ANT_D, 1},
                     round->chunk_steps + jo, nC, round->chunks_run, a.prev_action, a.has_prev, a.hist, a.hist_n, rows.idx,
                     p->inject_actions ? 0 : 1, s, rows.j < 0, cs, scp);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// What both stepped chunk calls check first; `who` names the entry point in its own messages.
static int check_ant_chunk_call(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_ant_round_params* p,
                                int j, const char* who) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_ant_round(ctx, tree, round, p, 1);
  if (rc) return rc;
  if (j < 0 || j >= tree->n_chunks) return set_err(ctx, DITREE_E_ARG, std::string(who) + ": chunk index out of range");
  if (round->B > ctx->ant.B) return set_err(ctx, DITREE_E_STATE, std::string(who) + ": call ditree_ant_round_begin first");
  return DITREE_OK;
}

int32_t ditree_ant_chunk_sample(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                const ditree_ant_round_params* p, int32_t j, void* stream) {
  const int rc = check_ant_chunk_call(ctx, tree, round, p, j, "ant_chunk_sample");
  if (rc) return rc;
  const int B = round->B;
  if (B == 0) return DITREE_OK;
  hipStream_t s = (hipStream_t)stream;
  if (p->early_exit && j > 0) {
    // RRT.py:179-184: a collided edge is abandoned -- the chunk runs on the candidates that are still alive
    launch_compact_alive(round->status, B, ctx->ant.idx, ctx->alive_cnt, s);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->alive_cnt_host, ctx->alive_cnt, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->ant_n_run = *ctx->alive_cnt_host;
    ctx->ant_run_idx = ctx->ant.idx;
  } else if (j == 0) {
    ctx->ant_n_run = B;
    ctx->ant_run_idx = nullptr;
  }
  return ant_sample_half(ctx, tree, round, p, nullptr, RowSet{ctx->ant_run_idx, ctx->ant_run_idx, ctx->ant_n_run, j}, s);
}

int32_t ditree_ant_chunk_step(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                              const ditree_ant_round_params* p, int32_t j, const double* next_obs, void* stream) {
  const int rc = check_ant_chunk_call(ctx, tree, round, p, j, "ant_chunk_step");
  if (rc) return rc;
  if (round->B == 0) return DITREE_OK;
  if (!next_obs) return set_err(ctx, DITREE_E_ARG, "ant_chunk_step: next_obs (B, A, 29) is required");
  return ant_step_half(ctx, tree, round, p, nullptr, nullptr, next_obs, (int64_t)tree->A * ANT_S,
                       RowSet{ctx->ant_run_idx, ctx->ant_run_idx, ctx->ant_n_run, j}, (hipStream_t)stream);
}

// The ant round of one tree, or (f != NULL, validated by the caller) of a forest: only the begin step differs.  An ant scene
// forest (tree_scene != NULL, validated by the caller) reads each row's maze and desired goal from the scene table instead.
static int expand_round_ant_impl(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, const ditree_round* round,
                                 const ditree_ant_round_params* p, void* stream, const int32_t* tree_scene = nullptr) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_ant_round(ctx, tree, round, p, 1, tree_scene != nullptr);
  if (rc) return rc;
  AntModelArg ma;
  const AntModelArg* model = nullptr;
  if (p->dynamics == DITREE_ANT_DYN_MODEL) {
    if (!p->model) return set_err(ctx, DITREE_E_ARG, "expand_round_ant: DITREE_ANT_DYN_MODEL without a model");
    rc = fill_ant_model(ctx, p->model, &ma);
    if (rc) return rc;
    model = &ma;
  } else if (p->dynamics == DITREE_ANT_DYN_TAPE) {
    if (!p->next_obs_tape) return set_err(ctx, DITREE_E_ARG, "expand_round_ant: DITREE_ANT_DYN_TAPE without next_obs_tape");
  } else {
    return set_err(ctx, DITREE_E_ARG, "expand_round_ant: dynamics must be DITREE_ANT_DYN_TAPE or DITREE_ANT_DYN_MODEL");
  }
  const int B = round->B, nC = tree->n_chunks, A = tree->A;
  hipStream_t s = (hipStream_t)stream;
  if (p->early_exit && B > 0 && p->cond_out)
    return set_err(ctx, DITREE_E_ARG, "expand_round_ant: cond_out is a test output of rounds without early_exit");
  SceneArg sc{};
  const SceneArg* scp = nullptr;
  if (tree_scene) {
    rc = round_scenes(ctx, f, tree_scene, B, s, &sc);
    if (rc) return rc;
    scp = &sc;
  }
  rc = ant_round_begin_impl(ctx, tree, f, round, p, stream, scp != nullptr);
  if (rc || B == 0) return rc;
  const int64_t tape_stride = (int64_t)nC * A * ANT_S;
  if (p->early_exit) {
    // the pool-scheduled form of the car round's early exit (ditree_expand_round): calls packed to whole tile-waves (2048
    // candidates for the ant network) from the ready list, rows of one launch at different chunks of their edges
    const int quantum = p->inject_actions ? 64 : denoise_wave_quantum(ctx);
    rc = run_ready_pool(ctx, "expand_round_ant", round, nullptr, nC, quantum, ctx->ant.idx, ctx->ant.nrow, s, [&](int take) -> int {
      const RowSet rows{ctx->ant.idx, ctx->ant.nrow, take, -1};
      const int src = ant_sample_half(ctx, tree, round, p, scp, rows, s);
      return src ? src : ant_step_half(ctx, tree, round, p, scp, model, p->next_obs_tape, tape_stride, rows, s);
    });
    return rc;
  }
  for (int j = 0; j < nC; ++j) {
    const RowSet rows{nullptr, nullptr, B, j};
    rc = ant_sample_half(ctx, tree, round, p, scp, rows, s);
    if (rc) return rc;
    rc = ant_step_half(ctx, tree, round, p, scp, model, model ? nullptr : p->next_obs_tape + (size_t)j * A * ANT_S, tape_stride, rows, s);
    if (rc) return rc;
  }
  return DITREE_OK;
}

int32_t ditree_expand_round_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                const ditree_ant_round_params* p, void* stream) {
  return expand_round_ant_impl(ctx, tree, nullptr, round, p, stream);
}

// planners/RRT.py:149-152 for the B candidates of a round, behind both chunk-budget entry points (`who` in the messages) after
// their tree / forest check.  f != NULL: parents are global node ids, so "earlier candidates with the same parent" never crosses trees.
static int chunk_budget_impl(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* f, int n_nodes,
                             const double* samples, int B, const int32_t* schedule_chunks, int n_schedule, int32_t* parent_scratch,
                             int32_t* budget_out, void* stream, const ditree_bound* bd = nullptr,
                             const ditree_sparse* sp = nullptr) {
  const std::string w(who);
  if (B == 0) return DITREE_OK;
  if (!samples || !schedule_chunks || !parent_scratch || !budget_out || B < 0 || n_schedule < 1 || n_schedule > 16 ||
      (!f && (n_nodes <= 0 || n_nodes > tree->capacity)))
    return set_err(ctx, DITREE_E_ARG, w + ": bad argument (1..16 schedule entries)");
  for (int i = 0; i < n_schedule; ++i)
    if (schedule_chunks[i] < 1 || schedule_chunks[i] > tree->n_chunks)
      return set_err(ctx, DITREE_E_ARG, w + ": a schedule entry exceeds the tree's edge capacity (n_chunks)");
  hipStream_t s = (hipStream_t)stream;
  search_nodes(tree, f, n_nodes, bd, samples, tree->state_dim, B, parent_scratch, nullptr, nullptr, nullptr, s, nullptr, sp);
  launch_chunk_budget(parent_scratch, B, tree->num_visit, schedule_chunks, n_schedule, budget_out, s);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_chunk_budget(ditree_ctx* ctx, const ditree_tree* tree, const double* samples, int32_t B, int32_t n_nodes,
                            const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch, int32_t* budget_out,
                            void* stream) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_tree(ctx, tree);
  if (rc) return rc;
  return chunk_budget_impl(ctx, "chunk_budget", tree, nullptr, n_nodes, samples, B, schedule_chunks, n_schedule, parent_scratch,
                           budget_out, stream);
}

int32_t ditree_round_stats(ditree_ctx* ctx, int32_t* stats4) {
  if (!ctx || !stats4) return DITREE_E_ARG;
  stats4[0] = ctx->ee_calls;
  stats4[1] = ctx->ee_waves;
  stats4[2] = denoise_wave_quantum(ctx);
  stats4[3] = 0;
  return DITREE_OK;
}

// The car round behind car_round_entry, which has checked ctx, tree or forest, round and every descriptor passed on here: the
// round of one tree, or (f != NULL) of a forest: only the nearest-node step differs.  A scene forest (tree_scene != NULL) reads
// each row's maze and goal from the scene table instead.  bd != NULL: the masked nearest-node search of the "anytime_pruned"
// mode.  nr != NULL: the near-parent rule in that search.  sp != NULL: that search over the active nodes of the sparse tree.
static int expand_round_impl(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, const ditree_round* round,
                             const ditree_round_params* p, void* stream, const int32_t* tree_scene = nullptr,
                             const ditree_bound* bd = nullptr, const ditree_near* nr = nullptr, const ditree_sparse* sp = nullptr) {
  if (!tree_scene && !ctx->maze) return set_err(ctx, DITREE_E_STATE, "expand_round: no maze uploaded");
  if (!p || !p->samples || !p->cond_goal || !p->norm || (!tree_scene && !p->goal_xy) || !p->axis ||
      (!f && (p->n_nodes <= 0 || p->n_nodes > tree->capacity)) || p->P < tree->A || (!p->noise && !p->inject_actions))
    return set_err(ctx, DITREE_E_ARG, "expand_round: bad parameters");
  if (tree->state_dim != 6 || tree->action_dim != 2)
    return set_err(ctx, DITREE_E_ARG, "expand_round: the car round needs a tree with state_dim 6 / action_dim 2 (ant: ditree_expand_round_ant)");
  const int B = round->B, A = tree->A, nC = tree->n_chunks, P = p->P;
  int rc = p->inject_actions ? DITREE_OK
                              : check_sampler(ctx, "expand_round", p->t0, p->dt, p->ddpm_coef, p->step_noise, p->K, P, p->lm_n, 2, 7,
                                              " (B, n_chunks, K, P, 2)", "; the car engine needs action_dim 2, cond 7)");
  if (rc) return rc;
  if (B == 0) return DITREE_OK;
  hipStream_t s = (hipStream_t)stream;
  rc = ensure_car_scratch(ctx, B, p->lm_n, P);
  if (rc) return rc;
  RoundScratch& c = ctx->car;
  AxisArg ax;
  rc = fill_axis(ctx, p->axis, p->lm_n, &ax);
  if (rc) return rc;
  NormArg nm;
  fill_norm(p->norm, &nm);
  SceneArg sc{};
  const SceneArg* scp = nullptr;
  if (tree_scene) {
    rc = round_scenes(ctx, f, tree_scene, B, s, &sc);
    if (rc) return rc;
    scp = &sc;
  }
  const double gx = tree_scene ? 0.0 : p->goal_xy[0], gy = tree_scene ? 0.0 : p->goal_xy[1];   // scenes: each row's own goal
  launch_round_begin(round->status, round->chunks_run, round->chunk_steps, B, nC, s);
  search_nodes(tree, f, p->n_nodes, bd, p->samples, 6, B, round->parent, c.state, c.prev_action, c.has_prev, s, nr, sp);
  const int64_t st_stride = (int64_t)nC * (A + 1) * 6, ac_stride = (int64_t)nC * A * 2;
  // One call of the round's chunk body on a row set: local map -> conditioning -> sampler (or the action tape) -> rollout.  Plain
  // chunk loop: every row at chunk j.  Pool: the ready list, each row at the chunk its chunks_run counter names (j = -1; the
  // kernel then adds the per-chunk strides itself).
  auto chunk_body = [&](const RowSet& rows) -> int {
    const size_t jo = rows.jo();
    const int64_t nrows = rows.noise_rows(nC);
    const double* acts;
    int64_t act_stride;
    int act_dense = 1;
    if (p->inject_actions) {
      acts = p->inject_actions + jo * P * 2;              // (B, n_chunks, P, 2), indexed by candidate
      act_stride = (int64_t)nC * P * 2;
      act_dense = 0;
    } else {
      if (scp)
        launch_local_map_scenes(sc, c.state, round->status, rows.idx, rows.n, p->lm_n, ax, p->s_global, c.lmap, s, 6);
      else
        launch_local_map(ctx->maze, ctx->rows, ctx->cols, c.state, round->status, rows.idx, rows.n, p->lm_n, ax, p->s_global, 1,
                         c.lmap, s);
      launch_cond_vector(c.state, c.prev_action, c.has_prev, p->cond_goal, rows.idx, rows.n, nm, p->lm_size, c.cond, s);
      double an[4] = {p->norm[12], p->norm[13], p->norm[14], p->norm[15]};
      // start noise rows of (P, 2) and, for the DDPM branch, step noise rows of (K, P, 2)
      const int src = round_sampler(ctx, p->noise + jo * P * 2, nrows * P * 2, rows.nrow, c.lmap, c.cond, rows.n, p->K, p->t0, p->dt,
                                    p->ddpm_coef, p->step_noise ? p->step_noise + jo * p->K * P * 2 : nullptr,
                                    nrows * p->K * P * 2, (int64_t)P * 2, an, c.act, s);
      if (src) return src;
      acts = c.act;
      act_stride = (int64_t)P * 2;
    }
    const ChunkStrides cs = rows.j < 0 ? ChunkStrides{(int64_t)(A + 1) * 6, (int64_t)A * 2, (int64_t)P * 2} : ChunkStrides{0, 0, 0};
    launch_car_rollout_ex(ctx->maze, ctx->rows, ctx->cols, c.state, acts, act_stride, round->status, rows.n, A, gx, gy,
                          round->states + jo * (A + 1) * 6, ditree_strides{st_stride, 6, 1}, round->actions + jo * A * 2,
                          ditree_strides{ac_stride, 2, 1}, round->chunk_steps + jo, nC, round->chunks_run, c.prev_action,
                          c.has_prev, rows.idx, act_dense, s, p->chunk_budget, rows.j, cs, scp);
    return DITREE_OK;
  };
  // Early exit (p->early_exit): what the reference does by abandoning a collided edge (planners/RRT.py:179-184) -- a chunk runs
  // only for candidates that are still alive.  A denoiser call costs whole WAVES of tiles (every layer has rows / quantum
  // tile-waves on the 256 CUs, quantum = 512 candidates for the car network), so the calls are packed to whole waves from a
  // POOL of ready (candidate, next chunk) items instead of one ragged call per chunk: after every call the ready list --
  // ordered by chunks finished, the candidates furthest behind first -- is rebuilt on the device, and the next call takes the
  // largest multiple of the quantum from its head (everything, once less than one quantum is left).  Rows of one launch may
  // sit at different chunks of their edges (chunk index = the candidate's chunks_run counter).  All candidates of a round see
  // the same tree snapshot and every kernel treats rows independently, so the results are bit-identical to the plain chunk
  // loop (tests: traces, rounds, full-size rounds).  Costs one 4-byte D2H per call.
  if (p->early_exit) {
    const int quantum = p->inject_actions ? 64 : denoise_wave_quantum(ctx);
    rc = run_ready_pool(ctx, "expand_round", round, p->chunk_budget, nC, quantum, c.idx, c.nrow, s,
                        [&](int take) { return chunk_body(RowSet{c.idx, c.nrow, take, -1}); });
  } else {
    for (int j = 0; j < nC && !rc; ++j) rc = chunk_body(RowSet{nullptr, nullptr, B, j});
  }
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(round->end_state, c.state, (size_t)B * 6 * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// ---- forests (include/ditree.h "forests"): every check runs on the host before anything is launched.
// B >= 0: the round's candidate count must equal off[T]; B < 0: the offsets are not read.
// ant: the tree must be an ant forest's (check_ant_forest) instead of a car tree.
static int check_forest(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, int B, const char* what, bool ant = false) {
  const std::string w(what);
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  if (!f || f->n_trees < 1 || f->tree_capacity < 1 || !f->counters)
    return set_err(ctx, DITREE_E_ARG, w + ": forest descriptor incomplete (n_trees >= 1, tree_capacity >= 1, counters)");
  if ((int64_t)f->n_trees * f->tree_capacity > tree->capacity)
    return set_err(ctx, DITREE_E_ARG, w + ": n_trees * tree_capacity = " + std::to_string((int64_t)f->n_trees * f->tree_capacity) +
                   " exceeds the tree's capacity " + std::to_string(tree->capacity));
  if (ant) {
    if (tree->state_dim != ANT_S || tree->action_dim != ANT_D || !tree->hist || !tree->hist_n)
      return set_err(ctx, DITREE_E_ARG, w + ": an ant forest is an ant tree (state_dim 29, action_dim 8, hist and hist_n present)");
    if (tree->obstacle_ahead)
      return set_err(ctx, DITREE_E_ARG, w + ": an ant forest is one rank's run_type-0 tree (no obstacle flags)");
  } else if (tree->state_dim != 6 || tree->action_dim != 2) {
    return set_err(ctx, DITREE_E_ARG, w + ": a forest is a car tree (state_dim 6, action_dim 2)");
  }
  if (B < 0) return DITREE_OK;
  if (!f->off || !f->off_host) return set_err(ctx, DITREE_E_ARG, w + ": forest offsets (off, off_host) missing");
  if (f->off_host[0] != 0) return set_err(ctx, DITREE_E_ARG, w + ": off[0] must be 0");
  for (int t = 0; t < f->n_trees; ++t)
    if (f->off_host[t + 1] < f->off_host[t])
      return set_err(ctx, DITREE_E_ARG, w + ": candidate offsets are not monotone at tree " + std::to_string(t));
  if (f->off_host[f->n_trees] != B)
    return set_err(ctx, DITREE_E_ARG, w + ": off[T] = " + std::to_string(f->off_host[f->n_trees]) + " but the round has " +
                   std::to_string(B) + " candidates");
  return DITREE_OK;
}

int32_t ditree_forest_chunk_budget(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* samples,
                                   int32_t B, const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch,
                                   int32_t* budget_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_forest(ctx, tree, forest, B, "forest_chunk_budget");
  if (rc) return rc;
  return chunk_budget_impl(ctx, "forest_chunk_budget", tree, forest, 0, samples, B, schedule_chunks, n_schedule, parent_scratch,
                           budget_out, stream);
}

int32_t ditree_forest_nn_argmin(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* queries,
                                int32_t q_stride, int32_t B, int32_t* out_idx, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_forest(ctx, tree, forest, B, "forest_nn_argmin");
  if (rc) return rc;
  if (B == 0) return DITREE_OK;
  if (!queries || !out_idx || q_stride < 2) return set_err(ctx, DITREE_E_ARG, "forest_nn_argmin: bad argument");
  search_nodes(tree, forest, 0, nullptr, queries, q_stride, B, out_idx, nullptr, nullptr, nullptr, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// planners/RRT.py:227-254 for every tree of a forest, behind the four fallback entry points (`who` in the messages).  ant: an ant
// forest's check instead of a car forest's.  per_tree: goal_xy is (T, 2), one goal per tree; else one goal, copied T times.  The T
// query rows travel from the host (a temporary or the caller's memory, hence the sync) to the car scratch's state rows -> one launch.
static int forest_fallback_impl(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* forest, bool ant,
                                bool per_tree, const double* goal_xy, int32_t* out_node, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_forest(ctx, tree, forest, -1, who, ant);
  if (rc) return rc;
  const std::string w(who);
  if (per_tree) {
    if (!goal_xy) return set_err(ctx, DITREE_E_ARG, w + ": goals array (T, 2) missing");
    if (!out_node) return set_err(ctx, DITREE_E_ARG, w + ": out_node missing");
  } else if (!goal_xy || !out_node) {
    return set_err(ctx, DITREE_E_ARG, w + ": bad argument");
  }
  const int T = forest->n_trees;
  std::vector<double> copies;
  if (!per_tree) {
    copies.resize((size_t)T * 2);
    for (int t = 0; t < T; ++t) { copies[(size_t)t * 2] = goal_xy[0]; copies[(size_t)t * 2 + 1] = goal_xy[1]; }
    goal_xy = copies.data();
  }
  hipStream_t s = (hipStream_t)stream;
  rc = ensure_car_scratch(ctx, T, 1, 1);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->car.state, goal_xy, (size_t)T * 2 * sizeof(double), hipMemcpyHostToDevice, s));
  launch_forest_fallback(ctx->car.state, T, tree->xy, forest->counters, forest->tree_capacity, out_node, s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return DITREE_OK;
}

int32_t ditree_forest_fallback(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                               int32_t* out_node, void* stream) {
  return forest_fallback_impl(ctx, "forest_fallback", tree, forest, false, false, goal_xy, out_node, stream);
}

// ---- scene forests (include/ditree.h "scene forests")
int32_t ditree_upload_scenes(ditree_ctx* ctx, int32_t n, const float* mazes, const int32_t* rows, const int32_t* cols,
                             const double* goal_xy, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  if (n < 1 || n > DITREE_MAX_SCENES)
    return set_err(ctx, DITREE_E_ARG, "upload_scenes: " + std::to_string(n) + " scenes (need 1.." + std::to_string(DITREE_MAX_SCENES) + ")");
  if (!mazes || !rows || !cols || !goal_xy) return set_err(ctx, DITREE_E_ARG, "upload_scenes: mazes, rows, cols and goal_xy are required");
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 1 || cols[i] < 1)
      return set_err(ctx, DITREE_E_ARG, "upload_scenes: scene " + std::to_string(i) + " has rows / cols < 1");
    total += (int64_t)rows[i] * cols[i];
  }
  if (total > DITREE_MAX_ATLAS_CELLS)
    return set_err(ctx, DITREE_E_ARG, "upload_scenes: the mazes hold " + std::to_string(total) + " cells, more than the atlas's " +
                   std::to_string(DITREE_MAX_ATLAS_CELLS));
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->scene_tab) HIP_TRY(ctx, hipMalloc((void**)&ctx->scene_tab, sizeof(SceneTable) + DITREE_MAX_ATLAS_CELLS));
  // the host image of the whole block: header, records, atlas; a map equal to an earlier scene's (dims and codes) shares its bytes
  std::vector<unsigned char> blk(sizeof(SceneTable) + (size_t)total, 0);
  SceneTable* tab = reinterpret_cast<SceneTable*>(blk.data());
  unsigned char* atlas = blk.data() + sizeof(SceneTable);
  tab->row_scene = ctx->row_scene;
  tab->n = n;
  int used = 0, max_cells = 0;
  const float* src = mazes;
  for (int i = 0; i < n; ++i) {
    const int cells = rows[i] * cols[i];
    unsigned char* dst = atlas + used;
    for (int k = 0; k < cells; ++k) {                  // ditree_upload_maze's rule
      const float v = src[k];
      const int c = (int)v;
      dst[k] = (v == (float)c && c >= 0 && c < 256) ? (unsigned char)c : (unsigned char)255;
    }
    src += cells;
    int offset = used;
    for (int j = 0; j < i; ++j)
      if (rows[j] == rows[i] && cols[j] == cols[i] && memcmp(atlas + tab->rec[j].offset, dst, cells) == 0) {
        offset = tab->rec[j].offset;
        break;
      }
    if (offset == used) used += cells;
    tab->rec[i] = SceneRec{offset, rows[i], cols[i], 0, goal_xy[2 * i], goal_xy[2 * i + 1]};
    max_cells = cells > max_cells ? cells : max_cells;
  }
  tab->atlas_cells = used;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->scene_tab, blk.data(), sizeof(SceneTable) + used, hipMemcpyHostToDevice, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));               // `blk` is a temporary
  ctx->n_scenes = n;
  ctx->atlas_cells = used;
  ctx->max_scene_cells = max_cells;
  return DITREE_OK;
}

static int check_scenes(ditree_ctx* ctx, const ditree_forest* f, const ditree_forest_scenes* sc, const char* what) {
  const std::string w(what);
  if (ctx->n_scenes < 1) return set_err(ctx, DITREE_E_STATE, w + ": no scene table uploaded (ditree_upload_scenes)");
  if (!sc || !sc->tree_scene || !sc->tree_scene_host)
    return set_err(ctx, DITREE_E_ARG, w + ": scene descriptor incomplete (tree_scene, tree_scene_host)");
  for (int t = 0; t < f->n_trees; ++t)
    if (sc->tree_scene_host[t] < 0 || sc->tree_scene_host[t] >= ctx->n_scenes)
      return set_err(ctx, DITREE_E_ARG, w + ": tree " + std::to_string(t) + " has scene id " + std::to_string(sc->tree_scene_host[t]) +
                     ", out of range [0, " + std::to_string(ctx->n_scenes) + ")");
  return DITREE_OK;
}

// ---- branch and bound (include/ditree.h "branch and bound"): what every call of the section refuses by name before anything
// is launched.  round: the calls that take one (NULL otherwise); search: the nearest-node calls read key, cost and counters only.
static int check_bound(ditree_ctx* ctx, const ditree_bound* bd, const ditree_round* round, bool search = false) {
  if (!bd) return set_err(ctx, DITREE_E_ARG, "bound: descriptor missing");
  if (!bd->cost) return set_err(ctx, DITREE_E_ARG, "bound: cost array missing");
  if (!bd->key) return set_err(ctx, DITREE_E_ARG, "bound: key column missing");
  if (round && round->shard != 0) return set_err(ctx, DITREE_E_ARG, "bound: one rank (round->shard must be 0)");
  if (search) return DITREE_OK;
  if (!bd->goal_xy) return set_err(ctx, DITREE_E_ARG, "bound: goal_xy missing");
  if (!bd->stats) return set_err(ctx, DITREE_E_ARG, "bound: stats rows missing");
  if (!(bd->reach > 0.0) || !std::isfinite(bd->reach)) return set_err(ctx, DITREE_E_ARG, "bound: reach must be > 0");
  if (!(bd->goal_radius >= 0.0) || !std::isfinite(bd->goal_radius))
    return set_err(ctx, DITREE_E_ARG, "bound: goal_radius must be >= 0 and finite");
  return DITREE_OK;
}

int32_t ditree_bound_keys(ditree_ctx* ctx, const ditree_tree* tree, const ditree_bound* bound, int32_t first, int32_t n,
                          int32_t tree_capacity, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_tree(ctx, tree);
  if (rc) return rc;
  rc = check_bound(ctx, bound, nullptr);
  if (rc) return rc;
  if (first < 0 || n < 0 || tree_capacity < 0 || (int64_t)first + n > tree->capacity)
    return set_err(ctx, DITREE_E_ARG, "bound_keys: nodes [first, first + n) must lie in the tree; tree_capacity >= 0");
  if (n == 0) return DITREE_OK;
  // a single tree (tree_capacity 0) is the forest of one tree: every node of it lies in tree 0
  launch_bound_keys(tree->xy, first, n, tree_capacity > 0 ? tree_capacity : tree->capacity, *bound, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// ---- near parent (include/ditree.h "near parent"): what every call of the section refuses by name before anything is launched.
// round: the calls that take one (NULL otherwise).
static int check_near(ditree_ctx* ctx, const ditree_near* nr, const ditree_round* round) {
  if (!nr) return set_err(ctx, DITREE_E_ARG, "near: descriptor missing");
  if (!nr->cost) return set_err(ctx, DITREE_E_ARG, "near: cost array missing");
  if (!(nr->radius > 0.0) || !std::isfinite(nr->radius)) return set_err(ctx, DITREE_E_ARG, "near: radius must be > 0 and finite");
  if (!(nr->reach > 0.0) || !std::isfinite(nr->reach)) return set_err(ctx, DITREE_E_ARG, "near: reach must be > 0 and finite");
  if (round && round->shard != 0) return set_err(ctx, DITREE_E_ARG, "near: one rank (round->shard must be 0)");
  return DITREE_OK;
}

// ---- sparse tree (include/ditree.h "sparse tree"): what every call of the section refuses by name before anything is
// launched.  T: the trees the descriptor's per-tree rows must cover; cost: the cost column of the calls that read one (the
// rebuild and the accepts; `needs_cost`); accept: the accepts need the candidate scratch too.
static int check_sparse(ditree_ctx* ctx, const ditree_sparse* sp, int T, const ditree_round* round = nullptr,
                        bool needs_cost = false, const int32_t* cost = nullptr, bool accept = false) {
  if (!sp) return set_err(ctx, DITREE_E_ARG, "sparse: descriptor missing");
  if (!(sp->cell > 0.0) || !std::isfinite(sp->cell)) return set_err(ctx, DITREE_E_ARG, "sparse: cell must be > 0 and finite");
  if (sp->nh < 1 || sp->nh > 64 || !(sp->w > 0.0) || !std::isfinite(sp->w))
    return set_err(ctx, DITREE_E_ARG, "sparse: nh must be 1..64 and w > 0");
  if (!sp->extent || !sp->dims || !sp->dims_host) return set_err(ctx, DITREE_E_ARG, "sparse: extent / dims missing");
  if (!sp->table || !sp->scratch || !sp->active || !sp->stats)
    return set_err(ctx, DITREE_E_ARG, "sparse: table, scratch, active or stats missing");
  if (sp->stride < 1 || sp->stride > (1 << 22)) return set_err(ctx, DITREE_E_ARG, "sparse: stride must be 1..2^22");
  for (int t = 0; t < T; ++t) {
    const int64_t nx = sp->dims_host[2 * t], ny = sp->dims_host[2 * t + 1];
    if (nx < 1 || ny < 1 || nx > sp->stride || ny > sp->stride || nx * ny * sp->nh > sp->stride)
      return set_err(ctx, DITREE_E_ARG, "sparse: nx * ny * nh of tree " + std::to_string(t) + " exceeds the stride");
  }
  if (needs_cost && !cost) return set_err(ctx, DITREE_E_ARG, "sparse: cost array missing");
  if (accept && !sp->cand) return set_err(ctx, DITREE_E_ARG, "sparse: cand scratch missing");
  if (round && round->shard != 0) return set_err(ctx, DITREE_E_ARG, "sparse: one rank (round->shard must be 0)");
  return DITREE_OK;
}

int32_t ditree_sparse_rebuild(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_sparse* sparse,
                              const int32_t* cost, int32_t first, int32_t n, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = forest ? check_forest(ctx, tree, forest, -1, "sparse_rebuild") : check_tree(ctx, tree);
  if (rc) return rc;
  const int T = forest ? forest->n_trees : 1;
  rc = check_sparse(ctx, sparse, T, nullptr, true, cost);
  if (rc) return rc;
  if (tree->state_dim != 6 || tree->action_dim != 2 || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "sparse: a run_type-0 car tree (no obstacle flags or hist)");
  if (first < 0 || n < 0 || (int64_t)first + n > T)
    return set_err(ctx, DITREE_E_ARG, "sparse_rebuild: trees [first, first + n) must lie in the forest");
  if (n == 0) return DITREE_OK;
  const TreeSet ts = forest ? TreeSet{nullptr, forest->counters, T, forest->tree_capacity}
                            : TreeSet{nullptr, tree->counters, 1, tree->capacity};
  launch_sparse_rebuild(*tree, ts, cost, *sparse, first, n, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

// ---- the entry points of the car's searches, rounds and accepts: one check each, in the order of include/ditree.h "check order".
// What an entry requires: REQ_FOREST a forest in place of the one tree, the others a descriptor that is checked even when NULL
// (its check names it missing); a descriptor the entry does not require is checked when present.
enum : unsigned { REQ_FOREST = 1, REQ_SCENES = 2, REQ_SPARSE = 4, REQ_NEAR = 8, REQ_BOUND = 16 };

static int check_trees(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* f, unsigned required, int B) {
  return (required & REQ_FOREST) ? check_forest(ctx, tree, f, B, who) : check_tree(ctx, tree);
}
// sparse, near, bound over T trees.  round: the calls that take one (NULL: a search or a budget, which read key, cost and counters
// of the bound only); accept: the accepts, whose sparse rule needs the cost column and the candidate scratch.
static int check_descriptors(ditree_ctx* ctx, const ditree_sparse* sparse, const ditree_near* near, const ditree_bound* bound,
                             unsigned required, int T, const ditree_round* round, const int32_t* cost = nullptr,
                             bool accept = false) {
  int rc = DITREE_OK;
  if (sparse || (required & REQ_SPARSE)) rc = check_sparse(ctx, sparse, T, round, accept, cost, accept);
  if (!rc && (near || (required & REQ_NEAR))) rc = check_near(ctx, near, round);
  if (!rc && (bound || (required & REQ_BOUND))) rc = check_bound(ctx, bound, round, round == nullptr);
  return rc;
}

// The six searches with descriptors (`who` in the messages; f == NULL: the first n_nodes nodes of the one tree).
static int nn_entry(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* f, int n_nodes,
                    const ditree_sparse* sparse, const ditree_near* near, const ditree_bound* bound, unsigned required,
                    const double* queries, int q_stride, int B, int32_t* out_idx, double* out_state, double* out_prev_action,
                    uint8_t* out_has_prev, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_trees(ctx, who, tree, f, required, B);
  if (rc) return rc;
  rc = check_descriptors(ctx, sparse, near, bound, required, f ? f->n_trees : 1, nullptr);
  if (rc) return rc;
  if (B == 0) return DITREE_OK;
  const bool gather = out_state || out_prev_action || out_has_prev;
  if (!queries || !out_idx || B < 0 || q_stride < 2 || (!f && (n_nodes <= 0 || n_nodes > tree->capacity)) ||
      (gather && (!out_state || !out_prev_action || !out_has_prev)))
    return set_err(ctx, DITREE_E_ARG, std::string(who) + ": bad argument (the three gather outputs come together)");
  search_nodes(tree, f, n_nodes, bound, queries, q_stride, B, out_idx, out_state, out_prev_action, out_has_prev, (hipStream_t)stream,
               near, sparse);
  HIP_TRY(ctx, hipGetLastError());
  return DITREE_OK;
}

int32_t ditree_nn_argmin_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_bound* bound, const double* queries,
                                 int32_t q_stride, int32_t B, int32_t n_nodes, int32_t* out_idx, double* out_state,
                                 double* out_prev_action, uint8_t* out_has_prev, void* stream) {
  return nn_entry(ctx, "nn_argmin_bounded", tree, nullptr, n_nodes, nullptr, nullptr, bound, REQ_BOUND, queries, q_stride, B, out_idx,
                  out_state, out_prev_action, out_has_prev, stream);
}
int32_t ditree_forest_nn_argmin_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                        const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B,
                                        int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev,
                                        void* stream) {
  return nn_entry(ctx, "forest_nn_argmin_bounded", tree, forest, 0, nullptr, nullptr, bound, REQ_FOREST | REQ_BOUND, queries, q_stride,
                  B, out_idx, out_state, out_prev_action, out_has_prev, stream);
}
int32_t ditree_nn_argmin_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_near* near, const ditree_bound* bound,
                              const double* queries, int32_t q_stride, int32_t B, int32_t n_nodes, int32_t* out_idx,
                              double* out_state, double* out_prev_action, uint8_t* out_has_prev, void* stream) {
  return nn_entry(ctx, "nn_argmin_near", tree, nullptr, n_nodes, nullptr, near, bound, REQ_NEAR, queries, q_stride, B, out_idx,
                  out_state, out_prev_action, out_has_prev, stream);
}
int32_t ditree_forest_nn_argmin_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_near* near,
                                     const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B,
                                     int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev,
                                     void* stream) {
  return nn_entry(ctx, "forest_nn_argmin_near", tree, forest, 0, nullptr, near, bound, REQ_FOREST | REQ_NEAR, queries, q_stride, B,
                  out_idx, out_state, out_prev_action, out_has_prev, stream);
}
int32_t ditree_nn_argmin_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_sparse* sparse, const ditree_near* near,
                                const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B, int32_t n_nodes,
                                int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev, void* stream) {
  return nn_entry(ctx, "nn_argmin_sparse", tree, nullptr, n_nodes, sparse, near, bound, REQ_SPARSE, queries, q_stride, B, out_idx,
                  out_state, out_prev_action, out_has_prev, stream);
}
int32_t ditree_forest_nn_argmin_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                       const ditree_sparse* sparse, const ditree_near* near, const ditree_bound* bound,
                                       const double* queries, int32_t q_stride, int32_t B, int32_t* out_idx, double* out_state,
                                       double* out_prev_action, uint8_t* out_has_prev, void* stream) {
  return nn_entry(ctx, "forest_nn_argmin_sparse", tree, forest, 0, sparse, near, bound, REQ_FOREST | REQ_SPARSE, queries, q_stride, B,
                  out_idx, out_state, out_prev_action, out_has_prev, stream);
}

int32_t ditree_chunk_budget_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                   const ditree_sparse* sparse, const ditree_bound* bound, const double* samples, int32_t B,
                                   int32_t n_nodes, const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch,
                                   int32_t* budget_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = forest ? check_forest(ctx, tree, forest, B, "chunk_budget_sparse") : check_tree(ctx, tree);
  if (rc) return rc;
  rc = check_descriptors(ctx, sparse, nullptr, bound, REQ_SPARSE, forest ? forest->n_trees : 1, nullptr);
  if (rc) return rc;
  return chunk_budget_impl(ctx, "chunk_budget_sparse", tree, forest, n_nodes, samples, B, schedule_chunks, n_schedule,
                           parent_scratch, budget_out, stream, bound, sparse);
}

// The nine car rounds.  who: the family's name without the forest's prefix, as the chunk-budget refusal of the rounds with a
// descriptor spells it; the forest's and the scenes' messages carry "forest_" + who.
static int car_round_entry(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* forest,
                           const ditree_forest_scenes* scenes, const ditree_round* round, const ditree_round_params* p,
                           const ditree_bound* bound, const ditree_near* near, const ditree_sparse* sparse, unsigned required,
                           void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_round(ctx, round);
  if (rc) return rc;
  const std::string fw = (required & REQ_FOREST) ? std::string("forest_") + who : std::string();   // a single tree has no use for it
  rc = check_trees(ctx, fw.c_str(), tree, forest, required, round->B);
  if (rc) return rc;
  if (scenes || (required & REQ_SCENES)) {
    rc = check_scenes(ctx, forest, scenes, fw.c_str());
    if (rc) return rc;
  }
  rc = check_descriptors(ctx, sparse, near, bound, required, forest ? forest->n_trees : 1, round);
  if (rc) return rc;
  if ((required & (REQ_SPARSE | REQ_NEAR | REQ_BOUND)) && p && p->chunk_budget)
    return set_err(ctx, DITREE_E_ARG, std::string(who) + ": chunk budgets are not built (p->chunk_budget must be NULL)");
  return expand_round_impl(ctx, tree, forest, round, p, stream, scenes ? scenes->tree_scene : nullptr, bound, near, sparse);
}

int32_t ditree_expand_round(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                            const ditree_round_params* p, void* stream) {
  return car_round_entry(ctx, "expand_round", tree, nullptr, nullptr, round, p, nullptr, nullptr, nullptr, 0, stream);
}
int32_t ditree_forest_expand_round(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                   const ditree_round* round, const ditree_round_params* p, void* stream) {
  return car_round_entry(ctx, "expand_round", tree, forest, nullptr, round, p, nullptr, nullptr, nullptr, REQ_FOREST, stream);
}
int32_t ditree_forest_expand_round_scenes(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                          const ditree_forest_scenes* scenes, const ditree_round* round,
                                          const ditree_round_params* p, void* stream) {
  return car_round_entry(ctx, "expand_round_scenes", tree, forest, scenes, round, p, nullptr, nullptr, nullptr, REQ_FOREST | REQ_SCENES,
                         stream);
}
int32_t ditree_expand_round_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                    const ditree_round_params* p, const ditree_bound* bound, void* stream) {
  return car_round_entry(ctx, "expand_round_bounded", tree, nullptr, nullptr, round, p, bound, nullptr, nullptr, REQ_BOUND, stream);
}
int32_t ditree_forest_expand_round_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                           const ditree_forest_scenes* scenes, const ditree_round* round,
                                           const ditree_round_params* p, const ditree_bound* bound, void* stream) {
  return car_round_entry(ctx, "expand_round_bounded", tree, forest, scenes, round, p, bound, nullptr, nullptr, REQ_FOREST | REQ_BOUND,
                         stream);
}
int32_t ditree_expand_round_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_round_params* p,
                                 const ditree_bound* bound, const ditree_near* near, void* stream) {
  return car_round_entry(ctx, "expand_round_near", tree, nullptr, nullptr, round, p, bound, near, nullptr, REQ_NEAR, stream);
}
int32_t ditree_forest_expand_round_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                        const ditree_forest_scenes* scenes, const ditree_round* round,
                                        const ditree_round_params* p, const ditree_bound* bound, const ditree_near* near,
                                        void* stream) {
  return car_round_entry(ctx, "expand_round_near", tree, forest, scenes, round, p, bound, near, nullptr, REQ_FOREST | REQ_NEAR, stream);
}
int32_t ditree_expand_round_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_round_params* p,
                                   const ditree_bound* bound, const ditree_near* near, const ditree_sparse* sparse, void* stream) {
  return car_round_entry(ctx, "expand_round_sparse", tree, nullptr, nullptr, round, p, bound, near, sparse, REQ_SPARSE, stream);
}
int32_t ditree_forest_expand_round_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                          const ditree_forest_scenes* scenes, const ditree_round* round,
                                          const ditree_round_params* p, const ditree_bound* bound, const ditree_near* near,
                                          const ditree_sparse* sparse, void* stream) {
  return car_round_entry(ctx, "expand_round_sparse", tree, forest, scenes, round, p, bound, near, sparse, REQ_FOREST | REQ_SPARSE,
                         stream);
}

// The eight car accepts: the shared part of their check (`who` in the forest's messages); each adds its family's own rules.
static int accept_entry(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* forest,
                        const ditree_round* round, unsigned required, const int32_t* cost = nullptr,
                        const ditree_bound* bound = nullptr, const ditree_sparse* sparse = nullptr) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_round(ctx, round);
  if (rc) return rc;
  rc = check_trees(ctx, who, tree, forest, required, round->B);
  if (rc) return rc;
  return check_descriptors(ctx, sparse, nullptr, bound, required, forest ? forest->n_trees : 1, round, cost, true);
}
// What ditree_accept_best and ditree_forest_accept_best refuse by name before anything is launched.
static int check_accept_best(ditree_ctx* ctx, const ditree_round* round, const int32_t* cost) {
  if (!cost) return set_err(ctx, DITREE_E_ARG, "accept_best: cost array missing");
  if (round->shard != 0) return set_err(ctx, DITREE_E_ARG, "accept_best: one rank (round->shard must be 0)");
  return DITREE_OK;
}

int32_t ditree_accept(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, int32_t emulate_sticky,
                      void* stream) {
  const int rc = accept_entry(ctx, "accept", tree, nullptr, round, 0);
  if (rc) return rc;
  if (round->B == 0) return DITREE_OK;
  if (tree->obstacle_ahead && !ctx->maze) return set_err(ctx, DITREE_E_STATE, "accept: obstacle-ahead flags need the maze");
  if (tree->hist && round->shard > 0 && (!round->hist || !round->hist_n))
    return set_err(ctx, DITREE_E_ARG, "accept: a sharded round on a tree with `hist` needs the round's hist / hist_n arrays");
  if (emulate_sticky && (tree->state_dim != 6 || tree->action_dim != 2))
    return set_err(ctx, DITREE_E_ARG, "accept: the sticky-done emulation is the car env's (car_env.py:254,266)");
  return accept_impl(ctx, tree, nullptr, round, AcceptMode::first, emulate_sticky, nullptr, nullptr, stream);
}
int32_t ditree_forest_accept(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                             int32_t emulate_sticky, void* stream) {
  const int rc = accept_entry(ctx, "forest_accept", tree, forest, round, REQ_FOREST);
  if (rc) return rc;
  if (round->shard > 0 || tree->obstacle_ahead || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "forest_accept: a forest is one rank's run_type-0 car tree (no shards, obstacle flags or hist)");
  return accept_impl(ctx, tree, forest, round, AcceptMode::first, emulate_sticky, nullptr, nullptr, stream);
}
int32_t ditree_accept_best(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, int32_t* cost, void* stream) {
  int rc = accept_entry(ctx, "accept_best", tree, nullptr, round, 0);
  if (rc) return rc;
  rc = check_accept_best(ctx, round, cost);
  if (rc) return rc;
  if (round->B == 0) return DITREE_OK;
  if (tree->obstacle_ahead && !ctx->maze) return set_err(ctx, DITREE_E_STATE, "accept_best: obstacle-ahead flags need the maze");
  return accept_impl(ctx, tree, nullptr, round, AcceptMode::best, 0, cost, nullptr, stream);
}
int32_t ditree_forest_accept_best(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                                  int32_t* cost, void* stream) {
  int rc = accept_entry(ctx, "forest_accept_best", tree, forest, round, REQ_FOREST);
  if (rc) return rc;
  rc = check_accept_best(ctx, round, cost);
  if (rc) return rc;
  if (tree->obstacle_ahead || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "forest_accept_best: a forest is one rank's run_type-0 car tree (no obstacle flags or hist)");
  return accept_impl(ctx, tree, forest, round, AcceptMode::best, 0, cost, nullptr, stream);
}
int32_t ditree_accept_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_bound* bound,
                              void* stream) {
  const int rc = accept_entry(ctx, "accept_bounded", tree, nullptr, round, REQ_BOUND, nullptr, bound);
  if (rc) return rc;
  if (tree->obstacle_ahead || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "accept_bounded: a run_type-0 car tree (no obstacle flags or hist)");
  return accept_impl(ctx, tree, nullptr, round, AcceptMode::bounded, 0, bound->cost, bound, stream);
}
int32_t ditree_forest_accept_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                     const ditree_round* round, const ditree_bound* bound, void* stream) {
  const int rc = accept_entry(ctx, "forest_accept_bounded", tree, forest, round, REQ_FOREST | REQ_BOUND, nullptr, bound);
  if (rc) return rc;
  if (tree->obstacle_ahead || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "forest_accept_bounded: a forest is one rank's run_type-0 car tree (no obstacle flags or hist)");
  return accept_impl(ctx, tree, forest, round, AcceptMode::bounded, 0, bound->cost, bound, stream);
}
// The tail of both sparse accepts (`who` in the messages; f == NULL: the one tree).
static int accept_sparse(ditree_ctx* ctx, const char* who, const ditree_tree* tree, const ditree_forest* f, unsigned required,
                         const ditree_round* round, int32_t* cost, const ditree_bound* bound, const ditree_sparse* sparse,
                         void* stream) {
  const int rc = accept_entry(ctx, who, tree, f, round, required | REQ_SPARSE, cost, bound, sparse);
  if (rc) return rc;
  if (bound && bound->cost != cost) return set_err(ctx, DITREE_E_ARG, std::string(who) + ": cost must be bound->cost");
  if (tree->state_dim != 6 || tree->action_dim != 2 || tree->obstacle_ahead || tree->hist)
    return set_err(ctx, DITREE_E_ARG, "sparse: a run_type-0 car tree (no obstacle flags or hist)");
  return accept_impl(ctx, tree, f, round, bound ? AcceptMode::bounded : AcceptMode::best, 0, cost, bound, stream, sparse);
}
int32_t ditree_accept_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, int32_t* cost,
                             const ditree_bound* bound, const ditree_sparse* sparse, void* stream) {
  return accept_sparse(ctx, "accept_sparse", tree, nullptr, 0, round, cost, bound, sparse, stream);
}
int32_t ditree_forest_accept_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                    const ditree_round* round, int32_t* cost, const ditree_bound* bound,
                                    const ditree_sparse* sparse, void* stream) {
  return accept_sparse(ctx, "forest_accept_sparse", tree, forest, REQ_FOREST, round, cost, bound, sparse, stream);
}

int32_t ditree_forest_fallback_goals(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                                     int32_t* out_node, void* stream) {
  return forest_fallback_impl(ctx, "forest_fallback_goals", tree, forest, false, true, goal_xy, out_node, stream);
}

// ---- ant forests (include/ditree.h "ant forests")
// The check of the three ant forest calls: an ant tree with hist, no obstacle flags, an unsharded round, the descriptor and
// the offsets as check_forest validates them.  round == NULL: a call without a round (the fallback; B < 0, offsets not read).
static int check_ant_forest(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* f, const ditree_round* round,
                            const char* what) {
  int rc = round ? check_round(ctx, round) : DITREE_OK;
  if (rc) return rc;
  rc = check_forest(ctx, tree, f, round ? round->B : -1, what, true);
  if (rc) return rc;
  if (round && round->shard > 0)
    return set_err(ctx, DITREE_E_ARG, std::string(what) + ": an ant forest is one rank's run_type-0 tree (no shards)");
  return DITREE_OK;
}

// planners/RRT.py:131-194 for the candidates of every run of an ant forest
int32_t ditree_forest_expand_round_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                       const ditree_round* round, const ditree_ant_round_params* p, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_ant_forest(ctx, tree, forest, round, "forest_expand_round_ant");
  if (rc) return rc;
  return expand_round_ant_impl(ctx, tree, forest, round, p, stream);
}

// planners/RRT.py:195-217 per tree; the commit's `hist` branch writes every new node's history rows
int32_t ditree_forest_accept_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                                 void* stream) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_ant_forest(ctx, tree, forest, round, "forest_accept_ant");
  if (rc) return rc;
  return accept_impl(ctx, tree, forest, round, AcceptMode::first, 0, nullptr, nullptr, stream);
}

// planners/RRT.py:227-254 (run_type 0) for every tree of an ant forest
int32_t ditree_forest_fallback_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                                   int32_t* out_node, void* stream) {
  return forest_fallback_impl(ctx, "forest_fallback_ant", tree, forest, true, false, goal_xy, out_node, stream);
}

// ---- ant scene forests (include/ditree.h "ant scene forests")
int32_t ditree_forest_expand_round_ant_scenes(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                              const ditree_forest_scenes* scenes, const ditree_round* round,
                                              const ditree_ant_round_params* p, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_ant_forest(ctx, tree, forest, round, "forest_expand_round_ant_scenes");
  if (rc) return rc;
  rc = check_scenes(ctx, forest, scenes, "forest_expand_round_ant_scenes");
  if (rc) return rc;
  return expand_round_ant_impl(ctx, tree, forest, round, p, stream, scenes->tree_scene);
}

int32_t ditree_forest_fallback_goals_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                                         int32_t* out_node, void* stream) {
  return forest_fallback_impl(ctx, "forest_fallback_goals_ant", tree, forest, true, true, goal_xy, out_node, stream);
}

// ---- policy roll-outs (include/ditree.h "policy roll-outs"): every check runs on the host before anything is launched
static int check_policy_batch(ditree_ctx* ctx, const ditree_policy_batch* b, const char* what) {
  const std::string w(what);
  if (ctx->n_scenes < 1) return set_err(ctx, DITREE_E_STATE, w + ": no scene table uploaded (ditree_upload_scenes)");
  if (!b || b->N < 1 || !b->scene || !b->scene_host || !b->state || !b->rows || !b->n_steps || !b->success_step || !b->collided ||
      !b->status || !b->best_dist || !b->last_action || !b->has_prev || !b->goal_xy || !b->idx)
    return set_err(ctx, DITREE_E_ARG, w + ": batch descriptor incomplete (N >= 1 and every array)");
  if (b->A < 1 || b->A > 64 || b->max_steps < 1)
    return set_err(ctx, DITREE_E_ARG, w + ": need 1 <= A <= 64, A <= P and 1 <= step_limit <= max_steps (A " + std::to_string(b->A) +
                   ", max_steps " + std::to_string(b->max_steps) + ")");
  for (int i = 0; i < b->N; ++i)
    if (b->scene_host[i] < 0 || b->scene_host[i] >= ctx->n_scenes)
      return set_err(ctx, DITREE_E_ARG, w + ": episode " + std::to_string(i) + " has scene id " + std::to_string(b->scene_host[i]) +
                     ", out of range [0, " + std::to_string(ctx->n_scenes) + ")");
  return DITREE_OK;
}

int32_t ditree_policy_begin(ditree_ctx* ctx, const ditree_policy_batch* batch, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  const int rc = check_policy_batch(ctx, batch, "policy_begin");
  if (rc) return rc;
  ctx->policy_key = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  launch_policy_begin(scene_arg(ctx), *batch, (hipStream_t)stream);
  HIP_TRY(ctx, hipGetLastError());
  ctx->policy_key = batch->idx;
  ctx->policy_n = batch->N;
  return DITREE_OK;
}

int32_t ditree_policy_chunk(ditree_ctx* ctx, const ditree_policy_batch* batch, const ditree_policy_params* p,
                            int32_t* n_active_out, void* stream) {
  if (!ctx) return DITREE_E_ARG;
  int rc = check_policy_batch(ctx, batch, "policy_chunk");
  if (rc) return rc;
  if (!p || !n_active_out) return set_err(ctx, DITREE_E_ARG, "policy_chunk: parameters and n_active_out are required");
  const int N = batch->N, A = batch->A, P = p->P;
  if (A > P || p->step_limit < 1 || p->step_limit > batch->max_steps)
    return set_err(ctx, DITREE_E_ARG, "policy_chunk: need 1 <= A <= 64, A <= P and 1 <= step_limit <= max_steps (A " + std::to_string(A) +
                   ", P " + std::to_string(P) + ", step_limit " + std::to_string(p->step_limit) + ", max_steps " +
                   std::to_string(batch->max_steps) + ")");
  if (!p->noise && !p->tape) return set_err(ctx, DITREE_E_ARG, "policy_chunk: neither noise nor an action tape");
  if (!p->tape) {
    if (!p->norm || !p->axis || !(p->s_global > 0.0))
      return set_err(ctx, DITREE_E_ARG, "policy_chunk: norm, axis and s_global > 0 are required with the network");
    rc = check_sampler(ctx, "policy_chunk", p->t0, p->dt, p->ddpm_coef, p->step_noise, p->K, P, p->lm_n, 2, 7, " (N, K, P, 2)",
                       "; the car's is action_dim 2, cond 7)");
    if (rc) return rc;
  }
  if (ctx->policy_key != batch->idx || ctx->policy_n < 0 || ctx->policy_n > N)
    return set_err(ctx, DITREE_E_STATE, "policy_chunk: call ditree_policy_begin on this batch first");
  const int n = ctx->policy_n;
  *n_active_out = n;
  if (n == 0) return DITREE_OK;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_car_scratch(ctx, N, p->tape ? 1 : p->lm_n, p->tape ? 1 : P);
  if (rc) return rc;
  const SceneArg sc = scene_arg(ctx);
  const double* acts = p->tape;
  int64_t act_stride = (int64_t)P * 2;
  int act_dense = 0;
  if (!p->tape) {
    AxisArg ax;
    rc = fill_axis(ctx, p->axis, p->lm_n, &ax);
    if (rc) return rc;
    NormArg nm;
    fill_norm(p->norm, &nm);
    // the local-map kernel reads a row's scene through the table's row -> scene scratch: rows are episodes here
    rc = ensure_row_scene(ctx, N, s);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->row_scene, batch->scene, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    launch_local_map_scenes(sc, batch->state, batch->status, batch->idx, n, p->lm_n, ax, p->s_global, ctx->car.lmap, s, 6);
    launch_cond_vector(batch->state, batch->last_action, batch->has_prev, batch->goal_xy, batch->idx, n, nm, p->lm_size, ctx->car.cond, s);
    double an[4] = {p->norm[12], p->norm[13], p->norm[14], p->norm[15]};
    rc = round_sampler(ctx, p->noise, (int64_t)P * 2, batch->idx, ctx->car.lmap, ctx->car.cond, n, p->K, p->t0, p->dt, p->ddpm_coef,
                       p->step_noise, (int64_t)p->K * P * 2, (int64_t)P * 2, an, ctx->car.act, s);
    if (rc) { ctx->policy_key = nullptr; return rc; }
    acts = ctx->car.act;
    act_dense = 1;
  }
  ctx->policy_key = nullptr;                         // until the new list and its length are known
  launch_policy_episode(sc, *batch, n, acts, act_stride, act_dense, p->step_limit, ctx->alive_cnt, s);
  launch_compact_alive(batch->status, N, batch->idx, ctx->alive_cnt + 1, s);
  HIP_TRY(ctx, hipGetLastError());
  // [0] the kernel's count of the episodes still running, [1] the length of the rebuilt list: one copy, and they must agree
  HIP_TRY(ctx, hipMemcpyAsync(ctx->alive_cnt_host, ctx->alive_cnt, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  const int left = ctx->alive_cnt_host[0];
  if (left < 0 || left > n || left != ctx->alive_cnt_host[1])
    return set_err(ctx, DITREE_E_STATE, "policy_chunk: the running count (" + std::to_string(left) + ") and the running list (" +
                   std::to_string(ctx->alive_cnt_host[1]) + ") disagree");
  ctx->policy_key = batch->idx;
  ctx->policy_n = left;
  *n_active_out = left;
  return DITREE_OK;
}

}  // extern "C"
