// Internal declarations shared by the HIP translation units of libditree_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ditree.h"

#define DITREE_MAX_AXIS 64
#define DITREE_LIDAR_RAYS 181

struct AxisArg {
  double v[DITREE_MAX_AXIS];
};
struct NormArg {
  double obs_mean[6], obs_std[6], act_mean[2], act_std[2];
};

struct AntNormArg {
  double obs_mean[27], obs_std[27], act_mean[8], act_std[8];
};

struct DenoiserState;   // denoise_state.h

// One scene of a scene table (ditree_upload_scenes): its maze at atlas[offset], rows x cols, and its goal.
struct SceneRec {
  int32_t offset, rows, cols, pad;
  double gx, gy;
};
// The scene table on the device, one block: the scene of every candidate row of the current round (ctx scratch), the records,
// then the atlas bytes.  The scene variants of the round's kernels take it in place of the maze pointer.
struct SceneTable {
  const int32_t* row_scene;
  int32_t n, atlas_cells;
  SceneRec rec[DITREE_MAX_SCENES];
};
static_assert(sizeof(SceneTable) % 16 == 0, "the atlas follows the records 16-byte aligned");
__host__ __device__ inline const unsigned char* scene_atlas(const SceneTable* t) {
  return reinterpret_cast<const unsigned char*>(t + 1);
}
// What the scene launchers need: the table, the atlas size (the rollout stages it whole), the largest maze (the local map
// stages one).
struct SceneArg {
  const SceneTable* table;
  int atlas_cells, max_cells;
};

// The scratch of one robot's rounds (ensure_round_scratch in ditree_api.hip): reserved for B candidates, a local map of lm x lm
// and P predicted actions; S / D / C below are the robot's state, action and conditioning widths.
struct RoundScratch {
  int B = 0, lm = 0, P = 0;
  double* state = nullptr;          // (B, S) live state of a round without history rows (the car; the ant's is round->end_state)
  double* hist = nullptr;           // (B, rows, S) history rows of the live state and (B,) how many are valid (the ant)
  int32_t* hist_n = nullptr;
  double* prev_action = nullptr;    // (B, D)
  uint8_t* has_prev = nullptr;      // (B,)
  float* lmap = nullptr;            // (B, lm, lm)
  float* cond = nullptr;            // (B, C)
  double* act = nullptr;            // (B, P, D) the sampler's actions
  int32_t* idx = nullptr;           // (B,) compacted candidate indices (early-exit rounds)
  int32_t* nrow = nullptr;          // (B,) their rows of the (B * n_chunks, P, D) noise view
};

struct ditree_ctx {
  int device = 0;
  std::string err;
  // known maze (u8 cell codes) on the device
  unsigned char* maze = nullptr;
  int rows = 0, cols = 0;
  size_t maze_cap = 0;
  // round scratch, one per robot so that alternating engines on one context never reallocate: the car's (S 6, D 2, cond 7; also
  // the query rows of the forest fallback and the sampler buffers of the policy roll-outs) and the ant's (29, 8, 97, 3 history rows)
  RoundScratch car, ant;
  int32_t* alive_cnt = nullptr;       // 16-byte device scalar block: list lengths of the early-exit rounds and the policy roll-outs
  int32_t* alive_cnt_host = nullptr;  // pinned host copy
  int ee_calls = 0, ee_waves = 0;     // denoiser calls / tile-waves of the last early-exit round (ditree_round_stats)
  double* path_dev = nullptr;         // reference path xy for the fallback selection
  int path_cap = 0;
  // the stepped ant round (ditree_ant_chunk_sample -> _step): the rows the current chunk runs on and their list (NULL: all)
  int ant_n_run = 0;
  const int32_t* ant_run_idx = nullptr;
  double* mppi_partial = nullptr;   // partial sums of the MPPI update, sized for the ant (256 slices of 3 + 8 * 64 doubles)
  unsigned long long* mppi_minkey = nullptr;   // running minimum of the rollout costs (order-preserving integer image)
  void* polish_partial = nullptr;     // plan polishing: one (tau, k, arriving) record per (plan, K-slice) of the current iteration
  size_t polish_partial_cap = 0;      // bytes
  DenoiserState* dn = nullptr;
  // scene table (ditree_upload_scenes): atlas of u8 cell codes, (n_scenes,) records, and a (row_scene_cap,) row -> scene scratch
  SceneTable* scene_tab = nullptr;                 // device block: header, records, atlas (DITREE_MAX_ATLAS_CELLS bytes)
  int n_scenes = 0, atlas_cells = 0, max_scene_cells = 0;
  int32_t* row_scene = nullptr;
  int row_scene_cap = 0;
  // policy roll-outs (ditree_policy_begin / _chunk): the batch whose running list is current (its idx array) and its length
  const void* policy_key = nullptr;
  int policy_n = 0;
  // optional RCCL communicator (ditree_comm_*): librccl opened at run time
  void* rccl_lib = nullptr;
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
};

int set_err(ditree_ctx* ctx, int code, const std::string& msg);
#define HIP_TRY(ctx, expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return set_err(ctx, DITREE_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// geom_kernels.hip launchers (all asynchronous on `s`)
void launch_maze_convert(const float* src, unsigned char* dst, int n, hipStream_t s);
// The argument block of the nearest-node searches, passed to the kernels by value: B query rows of q_stride doubles (x, y
// first), the node columns, and where the result goes.  state == NULL: only out_idx is written; else the chosen node's state,
// last action and flag are gathered into the three outputs (S <= 64, D <= 32).
struct NnArg {
  const double* queries;
  int q_stride, B;
  const double2* xy;
  const double* state;
  const double* last_action;
  const uint8_t* has_prev;
  int S, D;
  int32_t* out_idx;
  double* out_state;
  double* out_prev_action;
  uint8_t* out_has_prev;
  const int32_t* key;       // != NULL: the mask of the "anytime_pruned" mode, only nodes with key[n] < bcost[incumbent] take part
  const int32_t* bcost;     //          (the incumbent as the segment's counter row names it)
  const uint8_t* active;    // != NULL: only nodes with active[n] != 0 take part (include/ditree.h "sparse tree")
  const int32_t* cost;      // != NULL: the near-parent rule (include/ditree.h ditree_near) with this cost column, radius and reach
  double radius, reach;
};
// Which nodes a search covers: the first N of one tree (counters: its counter row, read under the key's mask only), or for
// every query its own tree of a forest -- T trees of C slots, tree t from slot `skip` up to its counter row's node count; off:
// the candidate offsets (NULL: query t belongs to tree t); norm: the fallback's key instead of the squared distance.
struct NnTree {
  int N;
  const int32_t* counters;
};
struct NnForest {
  const int32_t* off;
  int T;
  const int32_t* counters;
  int C, skip;
  bool norm;
};
void launch_nn(const NnArg& a, const NnTree& seg, hipStream_t s);
void launch_nn(const NnArg& a, const NnForest& seg, hipStream_t s);
void launch_forest_fallback(const double* goals, int T, const double* node_xy, const int32_t* counters, int C, int32_t* out_idx,
                            hipStream_t s);
// the bound of the "anytime_pruned" rounds travels to the kernels as the public descriptor (include/ditree.h ditree_bound)
using BoundArg = ditree_bound;
void launch_bound_keys(const double* xy, int first, int n, int C, const BoundArg& bd, hipStream_t s);
void launch_local_map_scenes(const SceneArg& sc, const double* state, const int32_t* active, const int32_t* idx, int B, int n,
                             const AxisArg& axis, double s_global, float* out, hipStream_t s, int state_stride);
void launch_row_scene(const int32_t* off, int T, const int32_t* tree_scene, int B, int32_t* row_scene, hipStream_t s);
void launch_local_map(const unsigned char* maze, int rows, int cols, const double* state,
                      const int32_t* active, const int32_t* idx, int B, int n, const AxisArg& axis,
                      double s_global, int scaled, float* out, hipStream_t s, int state_stride = 6);
void launch_cond_vector_ant(const double* obs, int n_rows, const int32_t* hist_n, const double* prev_action, const uint8_t* has_prev,
                            const double* cond_goal, const int32_t* idx, int B, const AntNormArg& nm, double lm_size, float* out,
                            hipStream_t s);
void launch_cond_vector(const double* state, const double* prev_action, const uint8_t* has_prev,
                        const double* cond_goal, const int32_t* idx, int B, const NormArg& nm, double lm_size,
                        float* out, hipStream_t s);
void launch_path_after_obstacle(const float* path, int stride, int P, double cx, double cy, int f32_state, const unsigned char* maze,
                                int rows, int cols, int32_t* out, hipStream_t s);
// ant_kernels.hip
struct AntModelArg;
int fill_ant_model(ditree_ctx* ctx, const ditree_ant_model* m, AntModelArg* a);      // ditree_api.hip: checked copy
struct AntChunkStrides { int64_t states, actions_out, actions_in, tape; };
void launch_ant_collision(const unsigned char* maze, int rows, int cols, const double* state, int stride, int B, double ball_radius,
                          double s_global, uint8_t* out, hipStream_t s);
void launch_ant_gather_hist(const int32_t* parent, const double* node_hist, const int32_t* node_hist_n, int B, double* hist,
                            int32_t* hist_n, hipStream_t s);
void launch_ant_copy_actions(const double* act, int64_t act_stride, int act_dense, const int32_t* idx, const int32_t* status,
                             int n_run, int A, double* out, int64_t out_stride, hipStream_t s);
void launch_ant_rollout(const unsigned char* maze, int rows, int cols, const AntModelArg* model, double* state_io,
                        const double* actions, int64_t act_stride, const double* tape, int64_t tape_stride, int32_t* status_io, int B,
                        int A, double gx, double gy, double goal_radius, double ball_radius, double s_global, double* states_out,
                        ditree_strides sl, double* actions_out, ditree_strides al, int32_t* steps_out, int64_t steps_stride,
                        int32_t* chunks_run, double* prev_action_io, uint8_t* has_prev_io, double* hist_out, int32_t* hist_n,
                        const int32_t* idx, int act_dense, hipStream_t s, int chunk_from_counter = 0,
                        AntChunkStrides cs = AntChunkStrides{0, 0, 0, 0}, const SceneArg* scenes = nullptr);
// per-chunk strides (doubles) of the round's row outputs / the injected action tape, for launches whose rows sit at different chunks
struct ChunkStrides { int64_t states, actions_out, actions_in; };
void launch_compact_ready(const int32_t* status, const int32_t* chunks_run, const int32_t* budget, int n_chunks, int B,
                          int32_t* idx_out, int32_t* nrow_out, int32_t* count, hipStream_t s);
int denoise_wave_quantum(ditree_ctx* ctx);
void launch_compact_alive(const int32_t* status, int B, int32_t* idx_out, int32_t* count, hipStream_t s,
                          const int32_t* budget = nullptr, int next_chunk = 0);
void launch_chunk_budget(const int32_t* parent, int B, const int32_t* num_visit, const int32_t* chunks, int n,
                         int32_t* budget, hipStream_t s);
void launch_gather_rows_f32(const float* src, int64_t src_stride, const int32_t* idx, float* dst, int row_floats, int n,
                            hipStream_t s);
void launch_car_rollout(const unsigned char* maze, int rows, int cols, double* state_io,
                        const double* actions, int64_t act_stride, int32_t* status_io, int B, int A,
                        double gx, double gy, double* states_out, int64_t states_stride,
                        double* actions_out, int64_t actout_stride, int32_t* steps_out,
                        double* prev_action_io, uint8_t* has_prev_io, hipStream_t s);
void launch_lidar_scan(const double* poses, int B, const float* maze, int rows, int cols, double* dist,
                       double* endpoints, uint8_t* hit, uint8_t* visited, hipStream_t s);
void launch_round_begin(int32_t* status, int32_t* chunks_run, int32_t* chunk_steps, int B, int n_chunks,
                        hipStream_t s);
void launch_round_chunk_end(const int32_t* chunk_status_in, int32_t* status, int32_t* chunks_run,
                            const double* cur_state, double* end_state, int B, hipStream_t s);
void launch_round_pack(const ditree_tree& t, const ditree_round& r, double* rec, hipStream_t s);
void launch_round_unpack(const ditree_tree& t, const ditree_round& r, const double* rec, hipStream_t s);
int record_doubles(const ditree_tree& t);
// policy_rollout_kernels.hip
void launch_policy_begin(const SceneArg& sc, const ditree_policy_batch& b, hipStream_t s);
void launch_policy_episode(const SceneArg& sc, const ditree_policy_batch& b, int n_run, const double* actions, int64_t act_stride,
                           int act_dense, int step_limit, int32_t* count, hipStream_t s);
struct AheadArg { double t[30]; };
// Which trees an accept works on: a forest is {forest->off, forest->counters, n_trees, tree_capacity}, a single tree the forest
// of one tree {NULL, tree->counters, 1, tree->capacity}.  off == NULL: the one tree takes the whole round.  Tree k owns counter
// row k and node slots [k * C, (k + 1) * C).
struct TreeSet {
  const int32_t* off;
  int32_t* counters;
  int T, C;
};
enum class AcceptMode { first, best, bounded };   // ditree_accept, ditree_accept_best, ditree_accept_bounded
// the sparse tree travels to the kernels as the public descriptor (include/ditree.h ditree_sparse); its table words are unsigned
// long long there, the type the 64-bit atomicMin takes
using SparseArg = ditree_sparse;
static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "sparse table words");
// sp != NULL: ditree_accept_sparse's rule on top of the best or the bounded mode
void launch_accept(const ditree_tree& t, const ditree_round& r, const TreeSet& ts, AcceptMode mode, int emulate_sticky,
                   int32_t* cost, const BoundArg* bd, const unsigned char* maze, int rows, int cols, const AheadArg& ahead,
                   hipStream_t s, const SparseArg* sp = nullptr);
void launch_sparse_rebuild(const ditree_tree& t, const TreeSet& ts, const int32_t* cost, const SparseArg& sp, int first, int n,
                           hipStream_t s);
void launch_obstacle_ahead(const unsigned char* maze, int rows, int cols, const double* state, int stride, int B,
                           const AheadArg& ts, uint8_t* out, hipStream_t s);
// ditree_tree_rebase: the anchor, whether a fresh root (its state by value: the car's 6 doubles) goes in front of it, and the
// rows the anchor's edge loses then
struct RebaseArg {
  int anchor, fresh_root, drop_states, drop_actions;
  double root[8];
};
void launch_tree_rebase(const ditree_tree& src, const ditree_tree& dst, const RebaseArg& a, const int32_t* cost_src,
                        int32_t* cost_dst, int32_t* scratch, const unsigned char* maze, int rows, int cols, const AheadArg& ahead,
                        hipStream_t s);
void launch_fallback_select(const ditree_tree& t, int n_nodes, double gx, double gy, const double* path_dev, int P,
                            int32_t* out_node, hipStream_t s);
void launch_follow_plan(double* state_io, const float* actions, int n_actions, int action_idx, const float* path, int P,
                        float* known, const float* truth, float* scanned, unsigned char* known_codes, int rows, int cols,
                        double gx, double gy, double dt, double scan_time, double* executed, int32_t* result,
                        hipStream_t s);
