// Ant (BASELINE config 3) kernels of the expansion path: collision glue, the higher-DoF rollout slot, history gather.
// Compiled with -ffp-contract=off (flags bit-exact against the CPU oracle).
//
// Reference sites (paths relative to the reference root):
//   ant_collision   common/map_utils.py:126-219 as called at planners/base_planner.py:154-155
//   ant_rollout     planners/base_planner.py:257-320 (ant branches :278-279,296-298) -- the env step itself is MuJoCo
//                   (third party, no oracle): a next-observation tape or the build's stand-in model takes its place
//   ant_gather      planners/RRT.py:144-147 (prev_actions / prev_states of the first sampler call of an edge)
#include "ant_rollout.h"

// ------------------------------------------------------------------------- collision
__global__ void __launch_bounds__(256)
ant_collision_kernel(const unsigned char* __restrict__ maze, int rows, int cols, const double* __restrict__ state, int stride, int B,
                     double ball_radius, double s_global, uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  stage_maze_ant(lds, maze, rows * cols);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  out[b] = ant_collides(state + (size_t)b * stride, lds, rows, cols, s_global, ball_radius) ? 1 : 0;
}
void launch_ant_collision(const unsigned char* maze, int rows, int cols, const double* state, int stride, int B, double ball_radius,
                          double s_global, uint8_t* out, hipStream_t s) {
  const size_t lds = ((size_t)rows * cols + 15) & ~(size_t)15;
  hipLaunchKernelGGL(ant_collision_kernel, dim3((B + 255) / 256), dim3(256), lds, s, maze, rows, cols, state, stride, B, ball_radius,
                     s_global, out);
}

// ------------------------------------------------------------------------- history gather (round begin)
// hist (B, 3, 29) <- tree.hist[parent], hist_n <- tree.hist_n[parent]; one thread per (candidate, element).
__global__ void ant_gather_hist_kernel(const int32_t* __restrict__ parent, const double* __restrict__ node_hist,
                                       const int32_t* __restrict__ node_hist_n, int B, double* __restrict__ hist,
                                       int32_t* __restrict__ hist_n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = e / (3 * ANT_S), k = e - b * (3 * ANT_S);
  if (b >= B) return;
  const int p = parent[b];
  hist[(size_t)b * 3 * ANT_S + k] = node_hist[(size_t)p * 3 * ANT_S + k];
  if (k == 0) hist_n[b] = node_hist_n[p];
}
void launch_ant_gather_hist(const int32_t* parent, const double* node_hist, const int32_t* node_hist_n, int B, double* hist,
                            int32_t* hist_n, hipStream_t s) {
  const int n = B * 3 * ANT_S;
  hipLaunchKernelGGL(ant_gather_hist_kernel, dim3((n + 255) / 256), dim3(256), 0, s, parent, node_hist, node_hist_n, B, hist, hist_n);
}

// round->actions[b, j, :A, :] <- the first A rows of candidate b's sampled sequence (what a host-side simulator reads before it
// steps; the rollout kernel rewrites the same rows, zeroing those behind a goal step).
__global__ void ant_copy_actions_kernel(const double* __restrict__ act, int64_t act_stride, int act_dense,
                                        const int32_t* __restrict__ idx, const int32_t* __restrict__ status, int n_run, int A,
                                        double* __restrict__ out, int64_t out_stride) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int ob = e / (A * ANT_D), k = e - ob * (A * ANT_D);
  if (ob >= n_run) return;
  const int b = idx ? idx[ob] : ob;
  if (status[b] != DITREE_ST_OK) return;
  out[(size_t)b * out_stride + k] = act[(size_t)(act_dense ? ob : b) * act_stride + k];
}
void launch_ant_copy_actions(const double* act, int64_t act_stride, int act_dense, const int32_t* idx, const int32_t* status,
                             int n_run, int A, double* out, int64_t out_stride, hipStream_t s) {
  const int n = n_run * A * ANT_D;
  hipLaunchKernelGGL(ant_copy_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, s, act, act_stride, act_dense, idx, status, n_run,
                     A, out, out_stride);
}

// ------------------------------------------------------------------------- rollout
// The kernel: ant_rollout.h.  An ant scene forest's launch (scenes != NULL) goes to the scene unit: the whole atlas is staged
// (rows = 1 x cols = its cells).
void launch_ant_rollout_scenes(const SceneArg& scenes, const AntModelArg* model, double* state_io, const double* actions,
                               int64_t act_stride, const double* tape, int64_t tape_stride, int32_t* status_io, int B, int A,
                               double goal_radius, double ball_radius, double s_global, double* states_out, ditree_strides sl,
                               double* actions_out, ditree_strides al, int32_t* steps_out, int64_t steps_stride,
                               int32_t* chunks_run, double* prev_action_io, uint8_t* has_prev_io, double* hist_out, int32_t* hist_n,
                               const int32_t* idx, int act_dense, hipStream_t s, int chunk_from_counter, AntChunkStrides cs);
void launch_ant_rollout(const unsigned char* maze, int rows, int cols, const AntModelArg* model, double* state_io,
                        const double* actions, int64_t act_stride, const double* tape, int64_t tape_stride, int32_t* status_io, int B,
                        int A, double gx, double gy, double goal_radius, double ball_radius, double s_global, double* states_out,
                        ditree_strides sl, double* actions_out, ditree_strides al, int32_t* steps_out, int64_t steps_stride,
                        int32_t* chunks_run, double* prev_action_io, uint8_t* has_prev_io, double* hist_out, int32_t* hist_n,
                        const int32_t* idx, int act_dense, hipStream_t s, int chunk_from_counter, AntChunkStrides cs,
                        const SceneArg* scenes) {
  if (scenes)
    launch_ant_rollout_scenes(*scenes, model, state_io, actions, act_stride, tape, tape_stride, status_io, B, A, goal_radius,
                              ball_radius, s_global, states_out, sl, actions_out, al, steps_out, steps_stride, chunks_run,
                              prev_action_io, has_prev_io, hist_out, hist_n, idx, act_dense, s, chunk_from_counter, cs);
  else
    launch_ant_rollout_t<false>(maze, rows, cols, model, state_io, actions, act_stride, tape, tape_stride, status_io, B, A, gx, gy,
                                goal_radius, ball_radius, s_global, states_out, sl, actions_out, al, steps_out, steps_stride,
                                chunks_run, prev_action_io, has_prev_io, hist_out, hist_n, idx, act_dense, s, chunk_from_counter, cs);
}
