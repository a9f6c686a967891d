// The SCENES instantiations of the ant rollout (ant_rollout.h) -- an ant scene forest's rollout, include/ditree.h "ant scene
// forests" -- in a unit of their own, so that the single-maze instantiations of ant_kernels.hip keep the code they had.
// Compiled with -ffp-contract=off (flags bit-exact against the CPU oracle).
#include "ant_rollout.h"

// `maze` is the scene table and rows x cols = 1 x the atlas's cells: the whole atlas is staged, the action burst sits behind it
// (16 KB of atlas + 64 KB of actions at 256 threads fit the 160 KB the launcher checks).  gx, gy come from each row's scene.
void launch_ant_rollout_scenes(const SceneArg& scenes, const AntModelArg* model, double* state_io, const double* actions,
                               int64_t act_stride, const double* tape, int64_t tape_stride, int32_t* status_io, int B, int A,
                               double goal_radius, double ball_radius, double s_global, double* states_out, ditree_strides sl,
                               double* actions_out, ditree_strides al, int32_t* steps_out, int64_t steps_stride,
                               int32_t* chunks_run, double* prev_action_io, uint8_t* has_prev_io, double* hist_out, int32_t* hist_n,
                               const int32_t* idx, int act_dense, hipStream_t s, int chunk_from_counter, AntChunkStrides cs) {
  launch_ant_rollout_t<true>((const unsigned char*)scenes.table, 1, scenes.atlas_cells, model, state_io, actions, act_stride, tape,
                             tape_stride, status_io, B, A, 0.0, 0.0, goal_radius, ball_radius, s_global, states_out, sl, actions_out,
                             al, steps_out, steps_stride, chunks_run, prev_action_io, has_prev_io, hist_out, hist_n, idx, act_dense, s,
                             chunk_from_counter, cs);
}
