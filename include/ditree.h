/*
 * ditree.h -- C-ABI of the MI355X-native DiTree expansion engine (libditree_hip.so).
 *
 * The reference (JJKK1313/DiTreeOnlinePlanner) is pure Python and has no FFI; its
 * "plugin boundary" for the hot path is the Python object surface that
 * run_scenarios*.py uses.  This header is the boundary the
 * build defines underneath that surface: every entry point below replaces the
 * numpy / scipy / PyTorch call site cited next to it (paths relative to the
 * reference root).  The Python facades in ditreeonlineplanner_amd/ bind these
 * symbols with ctypes (INTEGRATION.md shows the stub) and keep the reference's class
 * and argument names.
 *
 * Conventions
 *   - One ditree_ctx per (process, device).  A ctx is not re-entrant.
 *   - Every pointer argument marked [dev] is a caller-owned DEVICE pointer
 *     (e.g. torch.Tensor.data_ptr()); [host] is host memory read before return.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work
 *     is enqueued asynchronously on it; nothing synchronises the device.
 *   - Return value: 0 = ok, negative = DITREE_E_*; ditree_last_error(ctx) gives text
 *     valid until the next call on that ctx.  No exceptions, no exit().
 *   - Layouts are the reference's: car states (.., 6) f64 = x, y, psi, v, D, delta; car actions (.., 2) f64 = dD, ddelta;
 *     ant states (.., 29) f64 = achieved_goal (x, y) | observation (z, qw, qx, qy, qz, 8 joints, 14 velocities)
 *     (planners/base_planner.py:298), ant actions (.., 8); mazes row-major (rows, cols) f32 in {0, 1}.
 */
#ifndef DITREE_H
#define DITREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DITREE_VERSION 400          /* 0.4.0: runtime state / action width of the tree (car 6 / 2, ant 29 / 8), the ant round as a
                                       real expansion round (collision, goal, accept), ant_rollout + stand-in model, row strides.
                                       Added since, without a new number (every addition is new symbols only): forests, scene
                                       forests, branch and bound, near parent, re-planning on a kept tree, policy roll-outs, and
                                       the sparse tree (ditree_sparse: one cheapest node per state cell) */

#define DITREE_OK 0
#define DITREE_E_ARG (-1)           /* bad argument (null pointer, size out of range) */
#define DITREE_E_HIP (-2)           /* a HIP runtime call failed */
#define DITREE_E_STATE (-3)         /* call order (no maze / no weights uploaded) */
#define DITREE_E_NOMEM (-4)
/* Check order.  The car's searches with a descriptor (ditree_[forest_]nn_argmin_{bounded,near,sparse}), its rounds
 * (ditree_[forest_]expand_round[_scenes|_bounded|_near|_sparse]) and its accepts (ditree_[forest_]accept[_best|_bounded|_sparse])
 * test their arguments in one order and report the first fault: ctx, round, tree or forest, scenes, sparse, near, bound, then
 * the call's own rules.  An input with one fault gets that fault's code and text whatever the order. */

/* per-chunk / per-candidate status codes written by the rollout kernels */
#define DITREE_ST_NOT_RUN (-1)
#define DITREE_ST_OK 0              /* chunk finished: neither goal nor collision */
#define DITREE_ST_GOAL 1            /* planners/base_planner.py:300,314-317  (done is True) */
#define DITREE_ST_COLLIDED 2        /* planners/base_planner.py:306-312      (done is None) */
#define DITREE_ST_FLAG_GOAL_AT_COLLISION 0x100  /* the colliding step was inside the goal radius */

typedef struct ditree_ctx ditree_ctx;

int32_t ditree_version(void);
/* 16 hex digits: sha256 over the library's own sources (the csrc directory, this header) and compile flags, embedded at build time by
 * ditreeonlineplanner_amd/build.py; the Python binding refuses a library whose id differs from the sources next to it. */
const char* ditree_build_id(void);
int32_t ditree_ctx_create(int32_t device, ditree_ctx** out);
void ditree_ctx_destroy(ditree_ctx* ctx);
const char* ditree_last_error(ditree_ctx* ctx);

/* The planner's *known* occupancy grid (planners/base_planner.py:118 `self.maze`,
 * planners/RRT.py:57-59 update_maze).  Copies rows*cols floats host->device on
 * `stream`; used by ditree_local_map / ditree_car_rollout / ditree_expand_round. */
int32_t ditree_upload_maze(ditree_ctx* ctx, const float* maze /*[host] rows*cols*/,
                           int32_t rows, int32_t cols, void* stream);

/* planners/RRT.py:49-51 nearest_node (scipy KDTree.query, k = 1, first two dims) plus
 * the gather of the chosen node's fields (RRT.py:139-146).
 *   queries   [dev] (B, q_stride) f64, xy in columns 0..1
 *   node_xy   [dev] (N, 2) f64
 * Outputs (any may be NULL except out_idx):
 *   out_idx   [dev] (B,) i32  argmin_n ||q - node_n||^2, ties -> lowest n
 *   when node_state != NULL: out_state (B,6) = node_state[idx],
 *   out_prev_action (B,2) = node_last_action[idx], out_has_prev (B,) u8. */
int32_t ditree_nn_argmin(ditree_ctx* ctx, const double* queries, int32_t q_stride, int32_t B,
                         const double* node_xy, int32_t N, int32_t* out_idx,
                         const double* node_state, const double* node_last_action,
                         const uint8_t* node_has_prev, double* out_state,
                         double* out_prev_action, uint8_t* out_has_prev, void* stream);

/* common/map_utils.py:391-459 create_local_map on the uploaded maze.
 *   state [dev] (B, state_stride) f64, elements 0, 1, 2 used as x, y, psi (car: stride 6; the reference passes
 *   curr_state[2] for every env, planners/RRT.py:158-166, so the ant -- stride 29 -- rotates by its torso height);
 *   active [dev] (B,) i32 or NULL: rows with
 *   active[b] != DITREE_ST_OK are skipped;  axis [host] n doubles = the reference's
 *   np.linspace(-L/2 + s/2, L/2 - s/2, n) (map_utils.py:422-423), uploaded into ctx.
 *   out [dev] (B, n, n) f32; values m, or 2m-1 when scaled != 0 (policies/fm_policy.py:152). */
int32_t ditree_local_map(ditree_ctx* ctx, const double* state, int32_t state_stride, const int32_t* active,
                         int32_t B, int32_t n, const double* axis, double s_global, int32_t scaled,
                         float* out, void* stream);

/* policies/fm_policy.py:60-143, antmaze branch (obs_history 3, action_history 1, run_scenarios.py:123-132):
 * conditioning vector (B, 97) f32 = 3 x [z, rot6d(normalised quaternion) (6), joints + velocities (22)] | previous action
 * (8, normalised; raw zeros when has_prev == 0) | tanh((goal - position) / local_map_size) (2, yaw = 0).
 *   obs [dev] (B, n_hist, 29) f64, 1 <= n_hist <= 3 (missing steps are zero rows in front, fm_policy.py:96-102);
 *   prev_action [dev] (B, 8) f64; has_prev [dev] (B,) u8; cond_goal [dev] (B, 2) f64;
 *   norm [host] 70 doubles: obs_mean[27], obs_std[27], act_mean[8], act_std[8] (metadata/antmaze.pt). */
int32_t ditree_cond_vector_ant(ditree_ctx* ctx, const double* obs, int32_t n_hist, const double* prev_action,
                               const uint8_t* has_prev, const double* cond_goal, int32_t B, const double* norm,
                               double local_map_size, float* out, void* stream);

/* policies/fm_policy.py:60-143 (car): conditioning vector (B, 7) f32 =
 * [(v-5)/5, (D-.5)/.5, delta/.4 | (a_prev-mu)/sigma or 0,0 | tanh(R(-psi)(g-p)/lm_size)].
 *   norm [host] 16 doubles: obs_mean[6], obs_std[6], act_mean[2], act_std[2]. */
int32_t ditree_cond_vector(ditree_ctx* ctx, const double* state, const double* prev_action,
                           const uint8_t* has_prev, const double* cond_goal, int32_t B,
                           const double* norm, double local_map_size, float* out, void* stream);

/* planners/base_planner.py:257-320 propagate_action_sequence_env for B candidates:
 * A Euler steps of car_env.py:356-396, each followed by the goal test
 * (car_env.py:341-354) and the two-ball collision test (common/map_utils.py:103-115,
 * :221-329) against the uploaded maze.
 *   state_io   [dev] (B,6) f64  in: start state, out: end state (`obs`)
 *   actions    [dev] (B, act_stride) f64, rows of 2; the first A rows are used
 *   status_io  [dev] (B,) i32   in: rows != DITREE_ST_OK are skipped; out: chunk result
 *   states_out [dev] (B, states_stride) f64: (A+1, 6) rows; rows after the last
 *              executed step stay zero (base_planner.py:282)
 *   actions_out[dev] (B, actout_stride) f64: (A, 2) copy with rows after the goal step
 *              zeroed (base_planner.py:314-317)
 *   steps_out  [dev] (B,) i32 env steps executed (the colliding step counts)
 *   prev_action_io / has_prev_io: on DITREE_ST_OK updated to the chunk's last action
 *              (planners/RRT.py:188), may be NULL. */
int32_t ditree_car_rollout(ditree_ctx* ctx, double* state_io, const double* actions,
                           int64_t act_stride, int32_t* status_io, int32_t B, int32_t A,
                           const double* goal_xy /*[host] 2*/, double* states_out,
                           int64_t states_stride, double* actions_out, int64_t actout_stride,
                           int32_t* steps_out, double* prev_action_io, uint8_t* has_prev_io,
                           void* stream);

/* Where element (candidate b, row i, component k) of a per-candidate row block lives: base + b * cand + i * row + k * comp
 * doubles.  Rows packed per candidate (the reference's arrays): {rows * width, width, 1}.  Step-major, component-major,
 * candidate-minor -- {1, width * B, B} -- makes every store of a wavefront (64 consecutive candidates) one contiguous
 * 512-byte run instead of 64 fragments at a stride of rows * width * 8 bytes; what the large standalone rollouts use. */
typedef struct { int64_t cand, row, comp; } ditree_strides;

/* ditree_car_rollout with explicit layouts for the two row outputs (NULL = packed per candidate, i.e. ditree_car_rollout). */
int32_t ditree_car_rollout_ld(ditree_ctx* ctx, double* state_io, const double* actions, int64_t act_stride,
                              int32_t* status_io, int32_t B, int32_t A, const double* goal_xy /*[host] 2*/,
                              double* states_out, const ditree_strides* states_ld, double* actions_out,
                              const ditree_strides* actions_ld, int32_t* steps_out, double* prev_action_io,
                              uint8_t* has_prev_io, void* stream);

/* ------------------------------------------------------------------ ant: collision glue, stand-in dynamics, rollout */

/* common/map_utils.py:126-136 is_colliding_ant(state, maze, ant_radius, map_scale) as planners/base_planner.py:154-155 calls
 * it (1.2, s_global): upside down when R[2][2] = 1 - 2 (qx^2 + qy^2) < 0 with (qw, qx, qy, qz) = state[3:7]
 * (common/se3_utils.py:155-164), else the single-ball is_colliding_maze (common/map_utils.py:139-219: out of the map ->
 * collision; side walls when the ball crosses the cell's edge, beyond the map counting as a wall; corner cells when closer
 * than the radius, cells outside the map skipped) on the uploaded maze.
 *   state [dev] (B, stride >= 7) f64; out [dev] (B,) u8. */
int32_t ditree_ant_collision(ditree_ctx* ctx, const double* state, int32_t stride, int32_t B, double ball_radius,
                             double s_global, uint8_t* out, void* stream);

/* The ant's env step is MuJoCo 3.1.6 behind gymnasium-robotics 1.3.1 AntMaze_Large-v4 (requirements.txt:59,117; call sites
 * planners/base_planner.py:278-279,290): third party, not in the reference repository, no oracle -- NOT implemented.
 * What stands in for it in the higher-DoF rollout slot, PARITY UNPINNED BY CONSTRUCTION and labelled so wherever it runs:
 * this build's own surrogate of a four-legged crawler with the ant's interface (29-d observation, 8-d action clipped to
 * [-1, 1], frame_skip sub-steps of h seconds): per leg a hip and an ankle as damped second-order actuators with soft stops;
 * a loaded foot (load = (1 + tanh(contact_gain (ankle - ank_rest))) / 2) swept by its hip pushes the torso the other way
 * (planar force + yaw torque); uneven foot lift tilts the torso against an uprighting torque; the height follows the mean
 * lift; the quaternion integrates the body angular velocity and is re-normalised.  Defined by DESIGN.md and restated in
 * numpy as oracle/ant.py ant_model_step (tests hold the kernel to it at 1e-9). */
typedef struct {
  double h;                          /* integration step [s] (0.01) */
  double frame_skip;                 /* sub-steps per env step (5) */
  double k_act, k_spr, k_dmp, k_lim; /* actuator gain, joint spring, joint damping, soft-stop stiffness */
  double hip_lim, ank_lo, ank_hi, ank_rest;
  double contact_gain, leg_r, k_push, c_lin;
  double z0, z_gain, k_z, c_z;
  double k_lift, c_ang, k_up, k_yaw;
  double cphi, sphi;                 /* cos / sin of the first leg's mount angle (the others by symmetry) */
} ditree_ant_model;

/* planners/base_planner.py:257-320 for B ant candidates: A env steps, after each the goal test
 * ||obs[:2] - desired_goal|| < goal_radius (:296-297, goal_radius = 0.45 * s_global) and check_collision (:154-155,306;
 * ditree_ant_collision); collision wins, on goal the remaining action rows are zeroed (:315), unexecuted state rows stay 0.
 * The env step itself is `model` (the stand-in above) when model != NULL, else row i of next_obs_tape (test / measurement
 * infrastructure: the observation after every env step given from outside; with the real simulator the caller steps it on
 * the host between ditree_ant_chunk_sample and ditree_ant_chunk_step).
 *   state_io [dev] (B, 29) f64 in: chunk start, out: `obs`; actions [dev] (B, act_stride) f64 rows of 8;
 *   next_obs_tape [dev] (B, tape_stride) f64 rows of 29 or NULL; status_io as ditree_car_rollout;
 *   states_out [dev] A + 1 rows of 29 per candidate, actions_out [dev] A rows of 8, laid out by states_ld / actions_ld
 *   (NULL = packed per candidate); steps_out [dev] (B,) i32. */
int32_t ditree_ant_rollout(ditree_ctx* ctx, const ditree_ant_model* model, double* state_io, const double* actions,
                           int64_t act_stride, const double* next_obs_tape, int64_t tape_stride, int32_t* status_io,
                           int32_t B, int32_t A, const double* desired_goal_xy /*[host] 2*/, double goal_radius,
                           double ball_radius, double s_global, double* states_out, const ditree_strides* states_ld,
                           double* actions_out, const ditree_strides* actions_ld, int32_t* steps_out, void* stream);

/* lidar_sim/lidar_2d_sim.py:18-98 Lidar2DSim.scan for B poses (pose = x_col, y_row, yaw
 * in cell units) against `maze` [dev] (rows, cols) f32 (the *true* world, which may
 * differ from the uploaded known maze).  181 rays, arange(-180, 182, 2) degrees.
 * Extents: x runs along columns (0 .. cols), y along rows (0 .. rows).  On a square map this is the reference bit for bit;
 * on any other map the reference raises (it unpacks the shape as width = rows, :51), so there this is the build's own
 * definition, parity unpinned by construction.  A pose outside the map finds no border: d = 0, no hit, nothing visited
 * (the reference raises TypeError).
 *   dist [dev] (B,181) f64; endpoints [dev] (B,181,2) f64; hit [dev] (B,181) u8;
 *   visited [dev] (B, rows*cols) u8 or NULL: 1 where a ray sample fell before its hit. */
int32_t ditree_lidar_scan(ditree_ctx* ctx, const double* poses, int32_t B, const float* maze,
                          int32_t rows, int32_t cols, double* dist, double* endpoints,
                          uint8_t* hit, uint8_t* visited, void* stream);

/* ------------------------------------------------------------------ tree + rounds */

/* Device-resident tree (planners/base_planner.py:24-34 Node as SoA; all [dev]). */
typedef struct {
  int32_t capacity;          /* node slots */
  int32_t n_chunks, A;       /* edge_length / action_horizon, action_horizon */
  int32_t state_dim, action_dim;   /* S, D: 6 / 2 (car), 29 / 8 (ant); every "(.., 6)" / "(.., 2)" below reads (.., S) / (.., D) */
  double* state;             /* (cap, 6) */
  double* xy;                /* (cap, 2)  copy of state[:, :2] for the NN scan */
  int32_t* parent;           /* (cap,) */
  double* last_action;       /* (cap, 2)  last row of parent_action_seq */
  uint8_t* has_prev;         /* (cap,)    parent_action_seq is not None and not empty */
  int32_t* num_visit;        /* (cap,) */
  double* edge_states;       /* (cap, n_chunks*(A+1), 6)  zero-row-filtered, RRT.py:198-199 */
  double* edge_actions;      /* (cap, n_chunks*A, 2)      zero-row-filtered, RRT.py:196-197 */
  int32_t* edge_nstates;     /* (cap,) rows kept */
  int32_t* edge_nactions;    /* (cap,) */
  uint8_t* obstacle_ahead;   /* (cap,) or NULL: planners/RRT.py:61-81 flag of every appended node (run_type > 0) */
  int32_t* edge_owner;       /* (cap,) or NULL: rank that holds the node's edge rows (sharded rounds keep the trajectories
                                on the producing rank); -1 = every rank (root, frozen-env edges) */
  double* hist;              /* (cap, 3, S) or NULL: the last <= 3 rows of the node's filtered edge states, valid rows at the
                                END -- what the first sampler call of a child sees with obs_history 3 (planners/RRT.py:146-147,
                                policies/fm_policy.py:96-102; the ant).  Replicated on every rank (it travels in the record). */
  int32_t* hist_n;           /* (cap,) valid rows of hist (root: 1 = the start state) */
  int32_t* counters;         /* [0] n_nodes, [1] goal node (-1 none), [2] env.done latched
                                (car_env.py:254,266 "sticky done"), [3] chunk iterations,
                                [4] candidates processed, [5] sticky-done triggered */
} ditree_tree;

/* Per-round candidate records (all [dev]); B rows, written by ditree_expand_round or
 * by the individual ops, consumed by ditree_accept. */
typedef struct {
  int32_t B;
  int32_t* parent;           /* (B,) */
  int32_t* status;           /* (B,) final DITREE_ST_* (| FLAG_GOAL_AT_COLLISION) */
  int32_t* chunks_run;       /* (B,) */
  double* end_state;         /* (B, 6) */
  double* states;            /* (B, n_chunks, A+1, 6) */
  double* actions;           /* (B, n_chunks, A, 2) */
  int32_t* chunk_steps;      /* (B, n_chunks) */
  int32_t* node_id;          /* (B,) out: assigned node index or -1 */
  /* Sharded rounds (one process per GPU): only rows [own_lo, own_lo + own_n) of states / actions / chunk_steps were
   * produced here; the other rows arrive as 96-byte records (ditree_round_pack / _unpack), whose last / first action
   * land in the two arrays below.  Single rank: own_lo = 0, own_n = B, both arrays NULL. */
  double* last_action;       /* (B, 2) or NULL: last kept action row of the candidate's edge */
  double* first_action;      /* (B, 2) or NULL: actions[b, 0, 0, :] (the frozen-env edge of the sticky-done emulation) */
  int32_t own_lo, own_n;
  int32_t shard;             /* candidates per rank: owner of candidate b = b / shard (0 = single rank) */
  double* hist;              /* (B, 3, S) or NULL: trees with `hist`, sharded rounds: the exchanged end-of-edge history */
  int32_t* hist_n;           /* (B,) */
} ditree_round;

/* Candidate record exchanged between ranks once per round: S + 2 D + 2 doubles -- car: 12 = 96 bytes --
 * [end_state S | last_action D | first_action D | (parent, status) as two i32 | (chunks_run, hist_n) as two i32], followed by
 * [hist 3 S] for trees with `hist` (ant: 29 + 16 + 2 + 87 = 134 doubles).  ditree_record_doubles gives the count.
 * Edge trajectories stay on the producing rank.  pack: rows of `round` (this rank's slice) -> records_out (round->B, R);
 * unpack: records (B, R) of ALL candidates -> parent / status / chunks_run / end_state / last_action / first_action [/ hist]. */
#define DITREE_RECORD_DOUBLES 12    /* the car's record */
int32_t ditree_record_doubles(const ditree_tree* tree);
int32_t ditree_round_pack(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, double* records_out,
                          void* stream);
int32_t ditree_round_unpack(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const double* records,
                            void* stream);

/* The per-round exchange for hosts without torch.distributed: an RCCL communicator inside the ctx (librccl is opened at
 * run time; one process per GPU, ranks of ONE node over xGMI).
 *   ditree_comm_unique_id: rank 0 fills a 128-byte id and hands it to the other ranks (file, pipe, MPI ...);
 *   ditree_comm_init:      every rank, collective;
 *   ditree_allgather_nodes: recv (world * count_doubles) <- every rank's send (count_doubles), in rank order, on `stream`
 *                           (in place when send == recv + rank * count_doubles). */
int32_t ditree_comm_unique_id(ditree_ctx* ctx, uint8_t* id128);
int32_t ditree_comm_init(ditree_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id128);
int32_t ditree_allgather_nodes(ditree_ctx* ctx, const double* send, double* recv, int64_t count_doubles, void* stream);
int32_t ditree_comm_destroy(ditree_ctx* ctx);

/* planners/RRT.py:179-217: accept candidates in index order (collided edges dropped,
 * lowest goal-reaching accepted index ends the plan, later candidates dropped),
 * filter all-zero rows, append nodes.  emulate_sticky != 0 reproduces the latched
 * env.done defect described in DESIGN.md. */
int32_t ditree_accept(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                      int32_t emulate_sticky, void* stream);

/* The accept step of the planner's `solution` modes "best_of_round" and "anytime": the round keeps every solution it holds
 * and the goal node is the cheapest one, not the first drawn.
 *   cost [dev] (capacity,) int32, kept by the caller next to the tree: cost[n] = rows of the path from the root to node n
 *   (edge states + node states, as base_planner.py:342-363 strings them) -- cost[root] = 1, set by the caller at reset;
 *   cost[n] = cost[parent[n]] + edge_nstates[n] + 1, written here for every node the round appends.
 * Scan: candidates 0 .. B-1 in index order, nothing is cut at a goal; a candidate is accepted iff
 * (status & 0xff) != DITREE_ST_COLLIDED; node ids run from counters[0], an id at or past the capacity becomes -1 and sets
 * counters[6]; num_visit[parent[b]] += 1 for every candidate; counters[3] += sum of chunks_run, counters[4] += B;
 * counters[2] and [5] are untouched (no sticky-done phantom here) and counters[7] = -1.  Commit: as ditree_accept's.
 * Pick: among the candidates with status DITREE_ST_GOAL and a node id, the smallest (cost[node_id], b) is written to
 * counters[1] when counters[1] < 0 or its cost is strictly below cost[counters[1]] -- the incumbent wins a tie, within a round
 * the lowest index does.  A collided candidate with DITREE_ST_FLAG_GOAL_AT_COLLISION is not a goal, and a goal candidate that
 * lost its slot to the capacity is not eligible.
 * DITREE_E_ARG before anything is launched: "accept_best: cost array missing",
 * "accept_best: one rank (round->shard must be 0)". */
int32_t ditree_accept_best(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, int32_t* cost, void* stream);

/* planners/RRT.py:61-81 check_obstacle_ahead on the uploaded maze: 30 samples over 1.5 cells ahead of the
 * heading in (col, row) space, int-truncated and clipped, any occupied.
 *   state [dev] (B, stride) f64 (x, y, psi used); out [dev] (B,) u8.  The sample offsets are
 *   np.linspace(0, 1.5, 30) = i * (1.5 / 29), last = 1.5, evaluated in f64 as numpy does. */
int32_t ditree_obstacle_ahead(ditree_ctx* ctx, const double* state, int32_t stride, int32_t B,
                              uint8_t* out, void* stream);

/* planners/RRT.py:83-111 extract_path_after_obstacle on the uploaded (known) maze: out2[0] = index c of the path point
 * nearest to cur_xy (first occurrence; np.linalg.norm(env.state[:2] - path[:, :2], axis=1) in the dtype numpy gives the
 * difference: f32_state != 0 when env.state is float32 -- right after env.reset, car_env.py:215 -- else float64 with the f32
 * path promoted), out2[1] = k such that the remaining reference path is path[c:][k:] -- the points behind the first blocked
 * stretch, cells looked up in the path's float32 (k = -1: the path crosses no obstacle, the reference then keeps its last
 * point only; k = P - c: nothing remains).  path [dev] (P, stride >= 2) f32 rows x, y, ...; cur_xy [host] 2 f64
 * (env.state[:2]); out2 [dev] 2 x i32. */
int32_t ditree_path_after_obstacle(ditree_ctx* ctx, const float* path, int32_t stride, int32_t P, const double* cur_xy /*[host] 2*/,
                                   int32_t f32_state, int32_t* out2, void* stream);

/* planners/RRT.py:233-254 fallback node when the budget ends without reaching the goal, over nodes
 * 1..n-1 of the tree: path == NULL: argmin ||xy - goal|| + 1e4 * obstacle_ahead; path != NULL
 * ([host] (P, 2) f64 = init_main_path xy): argmax of the nearest path index (-1 when an obstacle is
 * ahead).  First occurrence wins, as np.argmin / np.argmax.  out_node [dev] i32 (tree index), or -1 when
 * every node has an obstacle ahead or the tree holds only the start (RRT.py:227-232: no plan). */
int32_t ditree_fallback_select(ditree_ctx* ctx, const ditree_tree* tree, int32_t n_nodes,
                               const double* goal_xy /*[host] 2*/, const double* path /*[host] or NULL*/,
                               int32_t P, int32_t* out_node, void* stream);

/* Plan following of the online driver (run_scenarios_with_lidar_DiTree.py:470-506, run_type < 4) fused into
 * one launch: per action one env step with goal test and collision test against the KNOWN maze
 * (planners/base_planner.py:257-320 with a single action); whenever the accumulated step time exceeds
 * scan_time, scan_and_update_maze (:112-127: lidar scan of the TRUE maze from the pose, ray end cells written
 * as occupied into the known and the scanned maze, visited cells = 2) and check_no_obstacles_in_path
 * (:158-181, evaluated in the path's float32).  Stops at the first event.
 *   state_io [dev] (6) f64 in/out; actions [dev] (n_actions, 2) f32 (the plan's dtype); path_xy [dev] (P, 2) f32;
 *   known / scanned [dev] (rows, cols) f32 in/out, true_maze [dev] (rows, cols) f32 (rows, cols = the uploaded
 *   maze's; the ctx's own copy of the known maze is refreshed, so no re-upload is needed before the next
 *   expansion round); goal_xy [host] 2; executed [dev] (n_actions - action_idx, 6) f64: state after every
 *   executed action; result [dev] 4 x i32: event (DITREE_EV_*), next action index, first blocked path index
 *   or -1, number of scans.  Ray end cells outside the map (only possible without border walls, where the
 *   reference raises IndexError) are dropped.  rows * cols <= 13104 (five byte maps of the maze stay in LDS).
 *   The scan is ditree_lidar_scan's: x along columns, y along rows, on non-square maps the build's own definition. */
#define DITREE_EV_ACTIONS_DONE 0
#define DITREE_EV_GOAL 1
#define DITREE_EV_COLLISION 2
#define DITREE_EV_OBSTACLE 3
int32_t ditree_follow_plan(ditree_ctx* ctx, double* state_io, const float* actions, int32_t n_actions,
                           int32_t action_idx, const float* path_xy, int32_t P, float* known_maze,
                           const float* true_maze, float* scanned_maze, const double* goal_xy /*[host] 2*/,
                           double dt, double scan_time, double* executed, int32_t* result, void* stream);

/* ------------------------------------------------------------------ MPPI controller */

/* One step of the MPPI controller `run_scenarios_with_lidar_MPPI.py:10,339-449` drives (`MPPI.mppi.MPPI(maze_data, T, K, nx,
 * nu)`: .reset / .step / .is_done / .set_ref_path / .reference_path / .update_maze / .env).  The reference repository does
 * not ship that module, so the algorithm is this build's own (DESIGN.md "MPPI"; PARITY UNPINNED): information-theoretic MPPI
 * on the reference's car dynamics (car_env.py:356-396), two-ball collision test (common/map_utils.py:103-115) and goal
 * radius (car_env.py:341-354), all against the maze uploaded with ditree_upload_maze.
 *   rollout k, step t:  u = U[t] + eps[k, t] (rollout 0: eps = 0), x <- car_step(x, u);
 *     cost += w_track * d2(x, path) + lambda * sum_d U[t, d] eps[k, t, d] / sigma_d^2;  d2 = squared distance to the nearest
 *     path point with index in [i - window_back, i + window_fwd] around the previous step's nearest index i (the first step
 *     starts from the nearest index of the current state over the whole path);
 *     collision: cost += w_collision, rollout ends;  goal radius: cost -= w_goal, rollout ends;
 *     terminal: cost += w_progress * (P - 1 - i_last).
 *   beta = min_k S_k;  w_k = exp(-(S_k - beta) / lambda);  U[t] += sum_k w_k eps[k, t] / sum_k w_k.
 *   execute: a = clip(U[0]) -> one env step; collision: state unchanged, U <- 0, status 2; else state <- x', U shifted by
 *   one step (last control held), status 1 inside the goal radius, else 0.
 * stages (bit mask, DITREE_MPPI_*): ROLLOUTS (fills costs [, flags]), MIN (beta = min_k S_k -> result[3]), SUMS (w_k from
 * result[3]; sums [dev] (3 + 2T) = {eta = sum w, sum w^2, collided rollouts, sum_k w_k eps[k, t, d]}), APPLY (U += sums[3..] /
 * sums[0], weights normalised, result[4], [6], [7]), EXECUTE (env step + shift).  DITREE_MPPI_ALL = one controller step.
 * SHARDED over ranks (BASELINE config 5: 65 536 rollouts over 8 GPUs; one process per GPU): every rank runs ROLLOUTS | MIN
 * on its K rollouts with k_offset = its first GLOBAL rollout index, the ranks all-reduce result[3] (MIN), run SUMS,
 * all-reduce `sums` (SUM), then APPLY | EXECUTE -- two collectives of 1 and 3 + 2T doubles per controller step; state and
 * controls stay replicated.  noise [dev] (K, T, 2) f64 or NULL = generated on the device, a pure function of (seed,
 * counter, GLOBAL k, t) (splitmix64 -> Box-Muller) that never touches HBM.
 *   state_io [dev] 6 f64; U_io [dev] (T, 2) f64 nominal controls; path_xy [dev] (P, 2) f64, P <= 4096; goal_xy [host] 2;
 *   costs [dev] (K) f64; weights [dev] (K) f64 or NULL (normalised w_k); flags [dev] (K) i32 or NULL (0, 1 goal, 2 collided);
 *   result [dev] 16 f64: executed action (2), status, beta, eta = sum_k w_k, nearest path index of the input state, number of
 *   collided rollouts (needs flags), effective sample size eta^2 / sum w^2, [8..13] the state after EXECUTE (one D2H per step). */
#define DITREE_MPPI_ROLLOUTS 1
#define DITREE_MPPI_MIN 2
#define DITREE_MPPI_SUMS 4
#define DITREE_MPPI_APPLY 8
#define DITREE_MPPI_EXECUTE 16
#define DITREE_MPPI_ALL 31
typedef struct {
  int32_t T, K;                      /* horizon (<= 64), rollouts */
  double lambda;                     /* temperature */
  double sigma[2];                   /* noise standard deviation of (dD, ddelta) */
  double w_track, w_progress, w_collision, w_goal;
  uint64_t seed;
  int32_t window_back, window_fwd;   /* nearest-path-index search window per step */
  int32_t lanes;                     /* lanes of a wavefront that share one rollout: 1, 2 or 4 (one ball and a share of the path
                                        window per lane: that many waves per SIMD at K = 65 536), 0 = the measured default.
                                        Same results whatever the value. */
  int64_t k_offset;                  /* global index of this rank's first rollout (0 for a single rank) */
} ditree_mppi_params;
int32_t ditree_mppi_step(ditree_ctx* ctx, const ditree_mppi_params* p, double* state_io, double* U_io, const double* path_xy,
                         int32_t P, const double* goal_xy, const double* noise, uint64_t counter, int32_t stages,
                         double* costs, double* weights, int32_t* flags, double* sums, double* result, void* stream);

/* MPPI missions: the MPPI driver's control loop (run_scenarios_with_lidar_MPPI.py:417-452: mppi_controller.step, the
 * ALLOWED_TRIALS collision retries, the executed path / actions, and every scan_time a scan_and_update_maze of the controller)
 * for M independent missions (a fleet) in ONE launch -- the controller-side counterpart of ditree_follow_plan.  One work-group
 * of 256 threads owns one mission from its first controller step to its terminating event; work-groups share nothing, so any
 * M runs.  With c counting the controller calls of this launch:
 *   input state inside the goal radius: event GOAL, nothing executed;
 *   for c in [0, max_steps): one controller step (noise counter counter0 + c) = rollouts, beta, weights and sums, U update, one
 *     executed step against the KNOWN maze.  Collided: the state stays, U <- 0, trials += 1, event TRIALS once trials >=
 *     allowed_trials.  Else trials = 0, the new state and the executed action are appended to the mission's trace, t_acc += dt;
 *     t_acc > scan_time: lidar scan of the TRUE maze from the pose, ray end cells -> 1 in known and scanned, visited cells -> 2
 *     in scanned (ditree_follow_plan's scan: x along columns, y along rows, on non-square maps the build's own definition),
 *     t_acc = 0; then inside the goal radius: event GOAL (after the scan, as the
 *     driver's loop body ends before is_done is tested again);
 *   event STEPS_DONE when the loop runs out.
 * BIT-EXACT against the stepwise form: a mission leaves exactly what the same sequence of ditree_mppi_step(DITREE_MPPI_ALL),
 * ditree_lidar_scan and ditree_upload_maze calls leaves (K <= 256 is that path's one-slice case; every sum takes its order).
 *   p: shared by the fleet (T <= 64, K <= 256, lambda, sigma, weights, windows; p->seed and p->lanes are not read, k_offset = 0).
 *   Per mission, [dev] arrays of M rows: seed, counter0 u64; state_io (M, 6), U_io (M, T, 2) f64 in/out; path_xy packed
 *   (sum P, 2) f64 with path_off / path_len (M) i32, every length <= P_max <= 4096; goal_xy (M, 2) f64; known_maze / scanned_maze
 *   (M, rows, cols) f32 in/out, true_maze (M, rows, cols) f32, rows * cols <= 13104; max_steps (M) i32, each <= trace_steps <=
 *   DITREE_MPPI_MISSION_MAX_STEPS (longer missions take further launches); allowed_trials (M) i32; dt, scan_time (M) f64;
 *   t_acc_io (M) f64 and trials_io (M) i32 in/out carry the scan cadence and the trial count across launches.
 *   Out: executed_states (M, trace_steps, 6), executed_actions (M, trace_steps, 2) f64, rows [0, steps executed) written;
 *   result (M, DITREE_MPPI_MISSION_RESULT) f64: event (DITREE_MEV_*), controller calls made, steps executed, scans, then the
 *   last controller call's beta, eta, nearest path index, collided rollouts and effective sample size (zero without a call).
 *   A mission whose path_len or max_steps breaks its bound runs nothing and reports DITREE_MEV_REFUSED.
 *   refresh_mission >= 0: that mission's final known-maze codes also replace the ctx's own maze copy (which must have the same
 *   shape), as ditree_follow_plan does; -1: the ctx's maze is not touched.
 * DITREE_E_ARG, each naming its limit, for K > 256, T > 64, P_max > 4096, rows * cols > 13104, k_offset != 0, a null pointer,
 * M < 1, trace_steps above the launch bound. */
#define DITREE_MEV_REFUSED (-1)
#define DITREE_MEV_STEPS_DONE 0
#define DITREE_MEV_GOAL 1
#define DITREE_MEV_TRIALS 2
#define DITREE_MPPI_MISSION_RESULT 16
#define DITREE_MPPI_MISSION_MAX_STEPS 2048
int32_t ditree_mppi_missions(ditree_ctx* ctx, const ditree_mppi_params* p, int32_t M, const uint64_t* seed,
                             const uint64_t* counter0, double* state_io, double* U_io, const double* path_xy,
                             const int32_t* path_off, const int32_t* path_len, int32_t P_max, const double* goal_xy,
                             float* known_maze, const float* true_maze, float* scanned_maze, int32_t rows, int32_t cols,
                             const int32_t* max_steps, int32_t trace_steps, const int32_t* allowed_trials, const double* dt,
                             const double* scan_time, double* t_acc_io, int32_t* trials_io, double* executed_states,
                             double* executed_actions, double* result, int32_t refresh_mission, void* stream);

/* The same controller on the higher-DoF rollout slot -- BASELINE config 5 as written ("MPPI antmaze, 65 536 rollouts"): 29-d
 * state, 8-d controls U (T, 8) with noise eps ~ N(0, diag(sigma^2)), every rollout step one env step of the build's STAND-IN
 * model (ditree_ant_model; NOT MuJoCo), the reference's ant collision test (ditree_ant_collision) and goal radius, the same
 * cost, soft-min update, executed step and stages as ditree_mppi_step.  The reference ships neither an MPPI module nor the
 * ant's physics: PARITY UNPINNED BY CONSTRUCTION (the build's numpy restatement: oracle/mppi.py).
 *   state_io [dev] 29 f64; U_io [dev] (T, 8); path_xy [dev] (P, 2); noise [dev] (K, T, 8) or NULL (counter hash, four
 *   Box-Muller pairs per (GLOBAL rollout, step)); costs / weights / flags as ditree_mppi_step; sums [dev] 3 + 8 T;
 *   result [dev] 64 f64: [2] status, [3] beta, [4] eta, [5] nearest path index of the input state, [6] collided rollouts,
 *   [7] effective sample size, [16..24) the executed action, [24..53) the state after EXECUTE. */
typedef struct {
  int32_t T, K;
  double lambda;
  double sigma[8];
  double w_track, w_progress, w_collision, w_goal;
  uint64_t seed;
  int32_t window_back, window_fwd;
  int64_t k_offset;
  double goal_radius, ball_radius, s_global;     /* 0.45 * s_global, 1.2, 4 (planners/base_planner.py:155,297) */
  ditree_ant_model model;
} ditree_mppi_ant_params;
int32_t ditree_mppi_step_ant(ditree_ctx* ctx, const ditree_mppi_ant_params* p, double* state_io, double* U_io,
                             const double* path_xy, int32_t P, const double* desired_goal_xy /*[host] 2*/, const double* noise,
                             uint64_t counter, int32_t stages, double* costs, double* weights, int32_t* flags, double* sums,
                             double* result, void* stream);

/* ------------------------------------------------------------------ denoiser */

/* Upload the denoiser weights (reference: run_scenarios.py:157-185, state-dict keys
 * `encoder.*`, `unet.*`).  `blob` [host] is the flat fp32 parameter blob and
 * `manifest` [host] a NUL-terminated text table "name offset n_elems dims...\n" built by
 * ditreeonlineplanner_amd/weights.py; the library repacks into MFMA-friendly bf16
 * (and, for the f32 parity instantiation, fp32) tiles on the device.
 *
 * Meta lines of the manifest (what the tensor shapes do not tell):
 *   #config pred_horizon <P> local_map_size <N>
 *   #encoder <name> <E>      the local-map encoder (local_map_encoder.py:78-97) and its embedding width; without the
 *                            line the net is a 'resnet' one (every blob stored before the line existed keeps loading)
 *   #checksum <s1> <s2>      Fletcher-style sums over the blob's 32-bit words (optional)
 * Encoders and the parameters they read:
 *   resnet    encoder.resnet18.*                      E = rows of encoder.resnet18.fc.weight
 *   identity  none                                    E = N * N
 *   mlp       encoder.fc{1,2,3}.{weight,bias}         E = N * N   (Linear(N*N, 128), ReLU, Linear(128, 256), ReLU, Linear(256, E))
 *   max       none                                    E = k * k   (AdaptiveMaxPool2d(k); E must be a perfect square)
 *   grid      encoder.conv{1,2,3}.{weight,bias}       E = 144     (3x3 convs 1 -> 3 -> 6 -> 4, ReLU, AdaptiveMaxPool2d(6))
 *   cnn       encoder.conv{1..4}.{weight,bias}        E = 4 (N - 8)^2   (3x3 convs 1 -> 2 -> 4 -> 4 -> 4, Mish after each)
 * The five small encoders run in f32 in every DITREE_PREC_* (encoder_kernels.hip); E must equal the width the kind
 * produces at N and cond_dim - 256 - E (the observation-conditioning width) must not be negative: DITREE_E_ARG otherwise. */
int32_t ditree_load_weights(ditree_ctx* ctx, const float* blob, int64_t n_floats,
                            const char* manifest, void* stream);

/* Allocate the activation workspace for up to max_batch candidates. */
int32_t ditree_denoise_reserve(ditree_ctx* ctx, int32_t max_batch, int32_t precision);
#define DITREE_PREC_BF16 0          /* bf16 MFMA inputs, fp32 accumulate (throughput path; 8 significand bits) */
#define DITREE_PREC_F32 1           /* fp32 MFMA (v_mfma_f32_32x32x2_f32): the reference's arithmetic, 1/16 of the bf16 rate */
#define DITREE_PREC_F16X3 2         /* f32-class: every operand as f16 hi + lo planes, 3 f16 MFMAs per product (22 bits),
                                       f32 accumulate, the encoder split the same way; 1/3 of the 16-bit rate.  f16 range:
                                       activations beyond +-65504 are clamped AND reported (ditree_denoise_status) */
#define DITREE_PREC_BF16X3 3        /* the same split on bf16 (16 significand bits, f32 range) */
#define DITREE_PREC_F16 4           /* plain f16 MFMA inputs (11 significand bits) at the bf16 rate */

/* Range guard of the f16 instantiations (DITREE_PREC_F16X3 / _F16).  The reference computes in fp32
 * (model/diffusion/conditional_unet1d.py:110-117: `scale * out + bias` of a FiLM layer has no bound); f16 activations
 * saturate at +-65504.  Every layer that stores f16 activations raises a sticky device flag when it is handed a value
 * beyond that range.  This call WAITS for `stream` (the one exception to "nothing synchronises"), reads the flags and
 * returns the number of layers that saturated since the last clear; their state-dict names (e.g.
 * "unet.mid_modules.0.blocks.0.block.0"), newline-separated and NUL-terminated, go to names [host] (names_cap bytes, may
 * be 0).  clear != 0 resets the flags.  A result > 0 means the actions of those calls are NOT the network's: re-reserve
 * with DITREE_PREC_BF16X3 (f32 exponent range) or DITREE_PREC_F32.  Always 0 for the bf16 / f32 instantiations. */
int32_t ditree_denoise_status(ditree_ctx* ctx, int32_t* n_saturated /*[host]*/, char* names /*[host]*/, int64_t names_cap,
                              int32_t clear, void* stream);

/* Dimensions of the loaded denoiser: dims5 = {pred_horizon, action_dim, local_map_size, obs-cond width, map embedding}. */
int32_t ditree_denoise_dims(ditree_ctx* ctx, int32_t* dims5);

/* policies/fm_policy.py:155-203 + local_map_encoder.py:101-109 +
 * model/diffusion/conditional_unet1d.py:268-347: K flow steps of
 * x <- x + net(x, map, 20*t0[k], cond) * dt[k], then a = x*sigma + mu.
 *   noise     [dev] (B, P, 2) f32   x0 ~ N(0, I)
 *   local_map [dev] (B, 20, 20) f32 already scaled to {-1, +1}
 *   cond      [dev] (B, 7) f32
 *   t0, dt    [host] K floats (common/fm_utils.py:4-17)
 *   act_norm  [host] 2*D doubles mu[D], sigma[D] (D = action_dim of the loaded net)
 *   actions   [dev] (B, P, 2) f64   un-normalised actions
 *   x_out     [dev] (B, P, 2) f32 or NULL: the normalised sample after the last step */
int32_t ditree_denoise(ditree_ctx* ctx, const float* noise, const float* local_map,
                       const float* cond, int32_t B, int32_t K, const float* t0, const float* dt,
                       const double* act_norm, double* actions, float* x_out, void* stream);

/* The sampler's policy = 'diffusion' branch (policies/fm_policy.py:164-182) with a DDPM scheduler as the reference configures it
 * (run_scenarios.py:157-158: beta_schedule 'squaredcos_cap_v2', clip_sample True, prediction_type 'epsilon'; variance
 * 'fixed_small'), K reverse steps inside the library:
 *   eps = net(x, map, timesteps[k], cond)            (the embedding sees the scheduler's integer timestep, unscaled)
 *   x0  = clip((x - sb_k eps) / sa_k, -1, 1);   x <- c0_k x0 + c1_k x + sigma_k z_k
 * with, for timestep t and its predecessor (abar = cumulative product of 1 - beta, abar_prev = 1 behind the last step):
 *   sb = sqrt(1 - abar_t), sa = sqrt(abar_t), c0 = sqrt(abar_prev) (1 - abar_t / abar_prev) / (1 - abar_t),
 *   c1 = sqrt(abar_t / abar_prev) (1 - abar_prev) / (1 - abar_t), sigma = sqrt(max((1 - abar_prev) / (1 - abar_t) (1 - abar_t /
 *   abar_prev), 1e-20)) for t > 0 and 0 at t = 0 -- all formed by the caller in float32 as the scheduler's tensors are.
 * `diffusers` is not part of the reference repository: the arithmetic follows the published algorithm (Ho et al. 2020 as
 * diffusers 0.x implements it) and is held to the build's numpy restatement -- PARITY UNPINNED.
 *   noise [dev] (B, P, D) f32 x_K ~ N(0, I); step_noise [dev] (B, K, P, D) f32 z_k ~ N(0, I) (row k unused where sigma_k = 0);
 *   timesteps [host] K floats; coef [host] (K, 5) floats sb, sa, c0, c1, sigma; other arguments as ditree_denoise. */
int32_t ditree_denoise_ddpm(ditree_ctx* ctx, const float* noise, const float* step_noise, const float* local_map,
                            const float* cond, int32_t B, int32_t K, const float* timesteps, const float* coef,
                            const double* act_norm, double* actions, float* x_out, void* stream);

/* One raw evaluation of the noise-prediction network, out = net(sample, map, timestep, cond)
 * (model/diffusion/conditional_unet1d.py:268-347 behind local_map_encoder.py:101-109): the building block of the
 * sampler's policy = 'diffusion' branch (policies/fm_policy.py:164-182), whose scheduler step stays with the caller.
 *   sample [dev] (B, P, 2) f32; timestep: the value the sinusoidal embedding sees (the scheduler's k);
 *   reuse_encoder != 0 keeps the map embedding of the previous call (same local maps, later steps of one loop);
 *   out [dev] (B, P, 2) f32. */
int32_t ditree_denoise_eval(ditree_ctx* ctx, const float* sample, const float* local_map, const float* cond,
                            int32_t B, float timestep, int32_t reuse_encoder, float* out, void* stream);

/* Measurement support.  enable = 1: every launch of the MFMA kernels is bracketed by hipEvents on its launch
 * stream (back-to-back launches share an event; ~120 marker packets per denoiser call, which costs a timed
 * region ~6 %); enable = 2: only the dominant kernel, one event pair around each run of back-to-back halo
 * launches (~20 packets per call); 0: off.  ditree_profile_read waits for the events and returns, per kernel
 * kind k = 0 conv3_halo16_kernel, 1 gemm16_kernel / conv_gemm_kernel, 2 conv2d_small_kernel: summed kernel time ms3[k],
 * launches3[k] and executed FLOPs flops3[k] (2*M*N*K of every launch) since the last enable. */
int32_t ditree_profile(ditree_ctx* ctx, int32_t enable);
int32_t ditree_profile_read(ditree_ctx* ctx, double* ms3, int64_t* launches3, double* flops3);

/* Test / debug support: copy a named internal activation of the last ditree_denoise call
 * (e.g. "d0b1.out", "skip2", "mid2.out", "final.h", "film", "map_emb") as f32
 * (B, L, C) into out [dev]; dims3 [host] receives (B, L, C). */
int32_t ditree_denoise_debug_read(ditree_ctx* ctx, const char* name, int32_t B, float* out,
                                  int64_t capacity, int32_t* dims3, void* stream);

/* One expansion round for B candidates (planners/RRT.py:131-194 batched):
 * nearest node -> n_chunks x [local map -> cond -> denoise (or injected actions)
 * -> rollout].  Fills `round`; does not modify the tree (call ditree_accept, after
 * the cross-rank all-gather when sharded). */
typedef struct {
  int32_t n_nodes;               /* tree size to search */
  const double* samples;         /* [dev] (B, 6) */
  const double* cond_goal;       /* [dev] (B, 2) */
  const float* noise;            /* [dev] (B, n_chunks, P, 2) f32, or NULL with inject_actions */
  const double* inject_actions;  /* [dev] (B, n_chunks, P, 2) f64 or NULL: bypass the denoiser */
  int32_t P;                     /* pred_horizon */
  int32_t K;                     /* flow steps */
  const float* t0;               /* [host] K */
  const float* dt;               /* [host] K */
  const double* norm;            /* [host] 16 doubles, see ditree_cond_vector */
  const double* goal_xy;         /* [host] 2: env.goal = centre of the goal cell */
  const double* axis;            /* [host] local-map axis, n doubles */
  int32_t lm_n;                  /* local_map_size */
  double lm_size;                /* the divisor of the goal conditioning (local_map_size) */
  double s_global;
  int32_t early_exit;            /* != 0: chunks run for the candidates that are still alive only (RRT.py:179-184), the denoiser calls
                                    packed to whole tile-waves from the pool of ready (candidate, chunk) items; same results */
  const float* ddpm_coef;        /* [host] (K, 5) or NULL.  != NULL: the sampler's DDPM branch (ditree_denoise_ddpm) instead of the
                                    flow steps; t0 then holds the K scheduler timesteps and dt is unused */
  const float* step_noise;       /* [dev] (B, n_chunks, K, P, 2) f32 with ddpm_coef */
  const int32_t* chunk_budget;   /* [dev] (B,) chunks each candidate may run (ditree_chunk_budget), or NULL = all n_chunks */
} ditree_round_params;

/* planners/RRT.py:26,149-152: `edge_length = prop_duration[clip(curr_node.num_visit)]; curr_node.num_visit += 1`.
 * For a round expanded against one tree snapshot the candidates of a parent are its visits in candidate order:
 * budget[b] = schedule[clip(num_visit[parent(b)] + #{b' < b : parent(b') == parent(b)})], in chunks of action_horizon steps.
 *   samples [dev] (B, 6): ALL candidates of the round (every rank computes the whole round's budgets: the rank inside a
 *   parent's visit order is a global property); schedule_chunks [host] n_schedule ints, each <= tree->n_chunks;
 *   parent_scratch [dev] (B,) i32 workspace (the nearest nodes); budget_out [dev] (B,) i32. */
int32_t ditree_chunk_budget(ditree_ctx* ctx, const ditree_tree* tree, const double* samples, int32_t B, int32_t n_nodes,
                            const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch,
                            int32_t* budget_out, void* stream);

int32_t ditree_expand_round(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                            const ditree_round_params* p, void* stream);

/* Scheduling figures of the last ditree_expand_round with early_exit on this ctx: stats4 [host] = {denoiser calls, tile-waves
 * they cost (sum over calls of ceil(rows / quantum)), the quantum = candidates per full wave of tiles on the 256 CUs for the
 * loaded denoiser (512 for the car network), 0}.  An early-exit round packs its calls to whole waves from a pool of ready
 * (candidate, next chunk) items (DESIGN.md "Early exit"); without early exit a round of B candidates and n chunks costs
 * n * ceil(B / quantum) waves. */
int32_t ditree_round_stats(ditree_ctx* ctx, int32_t* stats4);

/* ------------------------------------------------------------------ forests: many independent runs in one round
 * A forest of T trees with C node slots each is one ordinary ditree_tree with capacity >= T * C (car: state_dim 6,
 * action_dim 2).  Tree t owns node slots [t * C, (t + 1) * C) and its root sits at t * C; parent indices stay global, so edge
 * storage, num_visit and every per-candidate kernel work unchanged.  Each tree has its own row of a (T, 8) counter block in the
 * layout of ditree_tree.counters, with the goal node in the global numbering and [7] the phantom candidate as a row of the round.
 * The candidates of one round are grouped by tree: tree t's are rows [off[t], off[t + 1]) (empty: no candidate this round),
 * in that run's own order.  All trees share the maze, the start and the goal (the goal test lives in the rollout).
 * The tree argument's own `counters` is not read by the forest calls.  The calls of this section take a car tree only; an
 * ant tree (state_dim 29, action_dim 8, hist) has its own three calls, "ant forests" at the end of this header. */
typedef struct {
  int32_t n_trees;               /* T >= 1 */
  int32_t tree_capacity;         /* C >= 1 node slots per tree; T * C <= tree->capacity */
  int32_t* counters;             /* [dev] (T, 8) */
  const int32_t* off;            /* [dev] (T + 1) candidate offsets */
  const int32_t* off_host;       /* [host] (T + 1) the same offsets: validated before anything is launched */
} ditree_forest;

/* ditree_expand_round on a forest: each candidate's nearest node is searched in its own tree only (nodes
 * [t * C, t * C + n_t), n_t from the tree's counter row on the device -- no host round trip; p->n_nodes is not read).  Every
 * other step treats rows independently and is the single-tree round's.  round->B must equal off[T]. */
int32_t ditree_forest_expand_round(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                   const ditree_round* round, const ditree_round_params* p, void* stream);
/* ditree_accept per tree: one work-group per tree applies the single-tree rules (first goal, sticky-done phantom, accepted prefix,
 * iteration / candidate counts, overflow at the tree's own C) to its counter row and writes global node ids from t * C + n_t.
 * The accept calls of a single tree and of a forest (this one, _accept_best, _accept_bounded, _accept_ant) run the same kernels:
 * a single tree is accepted as the forest of one tree {its own counters, C = tree->capacity} whose range is the whole round. */
int32_t ditree_forest_accept(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                             int32_t emulate_sticky, void* stream);
/* ditree_accept_best per tree: one work-group per tree scans its candidate range (ids from t * C + n_t, overflow at the tree's
 * own C), and after the commit one work-group per tree picks its goal node into its counter row.  cost [dev] (tree->capacity,)
 * is indexed by the global node id; the caller sets cost[t * C] = 1 when it resets tree t.  An empty range leaves the tree
 * untouched.  The same two DITREE_E_ARG messages, before anything is launched. */
int32_t ditree_forest_accept_best(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                                  int32_t* cost, void* stream);
/* ditree_chunk_budget on a forest: samples [dev] (off[T], 6), nearest nodes searched per tree; B = off[T]. */
int32_t ditree_forest_chunk_budget(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* samples,
                                   int32_t B, const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch,
                                   int32_t* budget_out, void* stream);
/* Segmented nearest node: queries [dev] (B, q_stride >= 2) grouped by forest->off (B = off[T]) -> out_idx [dev] (B,) global node
 * ids; minimum squared distance, ties to the lowest index, an all-NaN scan -> the tree's root. */
int32_t ditree_forest_nn_argmin(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* queries,
                                int32_t q_stride, int32_t B, int32_t* out_idx, void* stream);
/* The run_type-0 fallback of every tree (planners/RRT.py:227-254): among nodes t * C + 1 .. t * C + n_t - 1 the one nearest to
 * goal_xy [host 2] -> out_node [dev] (T,) global ids, -1 for a tree that holds only its root.  forest->off is not read.
 * The key is the reference's, np.linalg.norm(state[:2] - goal) = sqrt(fma(dy, dy, dx*dx)) as ditree_fallback_select computes it,
 * first occurrence on ties -- not the squared distance of ditree_forest_nn_argmin: two nodes whose squares differ in the last
 * place can have equal norms, and the reference then returns the lower index. */
int32_t ditree_forest_fallback(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                               int32_t* out_node, void* stream);

/* ------------------------------------------------------------------ scene forests: trees of different scenarios in one round
 * A scene table holds n scenes (maze, goal) of a scenario set (run_scenarios.py:203-250: one maze, start and goal per row of
 * the scenario file).  The mazes are stored once each, as u8 cell codes (ditree_upload_maze's rule) in one atlas that the
 * rollout stages into LDS whole; identical maps (same dims, same codes) share their atlas bytes.  The table lives next to the
 * single maze of ditree_upload_maze and does not replace it.  A scene forest is a ditree_forest plus a scene id per tree; every
 * row of a round uses its tree's maze (local map, collision tests) and goal (goal test). */
#define DITREE_MAX_SCENES 64
#define DITREE_MAX_ATLAS_CELLS 16384
/* mazes [host] f32: the n row-major maps concatenated (scene i: rows[i] x cols[i]); rows, cols [host] (n,); goal_xy [host] (n, 2):
 * each scene's env.goal.  1 <= n <= DITREE_MAX_SCENES, every rows / cols >= 1, sum of rows * cols <= DITREE_MAX_ATLAS_CELLS. */
int32_t ditree_upload_scenes(ditree_ctx* ctx, int32_t n, const float* mazes, const int32_t* rows, const int32_t* cols,
                             const double* goal_xy, void* stream);
typedef struct {
  const int32_t* tree_scene;        /* [dev] (T,) the scene of every tree */
  const int32_t* tree_scene_host;   /* [host] (T,) the same ids: each in [0, n uploaded), validated before anything is launched */
} ditree_forest_scenes;
/* ditree_forest_expand_round with each tree's own scene: p->goal_xy is not read, and no single maze is needed.  DITREE_E_STATE
 * without an uploaded scene table.  Each candidate's arithmetic is the single-maze round's on its scene's bytes, dims and goal. */
int32_t ditree_forest_expand_round_scenes(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                          const ditree_forest_scenes* scenes, const ditree_round* round,
                                          const ditree_round_params* p, void* stream);
/* ditree_forest_fallback with one goal per tree: goal_xy [host] (T, 2). */
int32_t ditree_forest_fallback_goals(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                                     int32_t* out_node, void* stream);

/* ------------------------------------------------------------------ branch and bound: the planner's "anytime_pruned" mode
 * Extends ditree_accept_best (the cost column and the incumbent in counters[1]) by a bound: once a tree holds an incumbent,
 * only nodes that can still lead to a shorter path are selected as parents, and only candidates that can still beat it get a
 * node.  All quantities are int32 path rows, like cost.
 *   h(x, y) = 0 unless q = (sqrt(fma(dy, dy, dx*dx)) - goal_radius) / reach > 0 (a NaN distance gives 0), else
 *             min(ceil(q), 2^30); (dx, dy) = (x, y) - the tree's goal.  reach = the metres one path row is ASSUMED to cover at
 *             most: the dynamics have no hard speed limit, so the bound is a setting, not a theorem.
 *   key[n]  = cost[n] + h(xy[n]); a node is open while key[n] < U, else closed.  Closed nodes stay in the tree.
 *   U       = cost[counters[1]], or INT32_MAX while counters[1] < 0 -- read on the device; counters[1] is written by the accept's
 *             pick alone, so the nearest-node search and the accept of one round use the incumbent the round before left.
 * Single tree: goal_xy (1, 2), stats (4,), and the tree's own counters.  Forest: goal_xy (T, 2) -- each tree's own goal, which
 * covers scene forests --, stats (T, 4), key / cost indexed by the global slot, the forest's counter block. */
typedef struct {
  int32_t* cost;                 /* [dev] (capacity,) as ditree_accept_best's; the caller sets cost[root] = 1 at reset */
  int32_t* key;                  /* [dev] (capacity,) written by the accept for every node it appends; roots: ditree_bound_keys */
  const double* goal_xy;         /* [dev] (T, 2) the goal the rollout tests against (the car: env.goal) */
  double goal_radius;            /* the goal test's radius (the car: 0.5) */
  double reach;                  /* > 0 */
  int32_t* stats;                /* [dev] (T, 4): [0] U after the last accept, [1] candidates pruned since the reset, [2] 1 when
                                    key[root] >= U -- no node of the tree can be open: the plan is exhausted --, [3] candidates
                                    pruned by the last accept.  The caller sets (INT32_MAX, 0, 0, 0) at reset. */
} ditree_bound;
/* Every call of this section refuses by name (DITREE_E_ARG) before anything is launched: "bound: descriptor missing",
 * "bound: cost array missing", "bound: key column missing", "bound: goal_xy missing", "bound: stats rows missing",
 * "bound: reach must be > 0", "bound: goal_radius must be >= 0 and finite", and -- the calls that take a round --
 * "bound: one rank (round->shard must be 0)". */

/* key[n] = cost[n] + h(xy[n]) for nodes [first, first + n) -- the roots after a reset, or any range (tests).  tree_capacity:
 * 0 for a single tree, else the forest's C (node n belongs to tree n / C and uses goal_xy row n / C). */
int32_t ditree_bound_keys(ditree_ctx* ctx, const ditree_tree* tree, const ditree_bound* bound, int32_t first, int32_t n,
                          int32_t tree_capacity, void* stream);
/* ditree_nn_argmin among the open nodes of tree->xy[0 .. n_nodes): squared distance, ties to the lowest open index, the scan
 * order and reduction of ditree_nn_argmin -- with U = INT32_MAX its result bit for bit.  No open node: what an all-NaN scan
 * returns (node 0); a planner never launches such a round (stats[2]).  out_state / out_prev_action / out_has_prev [dev]
 * (B, S) / (B, D) / (B,): the gathered node rows, or all three NULL.  bound->goal_xy, reach and stats are not read. */
int32_t ditree_nn_argmin_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_bound* bound, const double* queries,
                                 int32_t q_stride, int32_t B, int32_t n_nodes, int32_t* out_idx, double* out_state,
                                 double* out_prev_action, uint8_t* out_has_prev, void* stream);
/* ditree_forest_nn_argmin among each tree's open nodes, under that tree's own U (no open node: the tree's root). */
int32_t ditree_forest_nn_argmin_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                        const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B,
                                        int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev,
                                        void* stream);
/* ditree_expand_round with the masked nearest-node search; every other step is ditree_expand_round's.  Also refused:
 * "expand_round_bounded: chunk budgets are not built (p->chunk_budget must be NULL)" -- ditree_chunk_budget runs its own
 * unmasked search. */
int32_t ditree_expand_round_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                    const ditree_round_params* p, const ditree_bound* bound, void* stream);
/* ditree_forest_expand_round (scenes == NULL) or ditree_forest_expand_round_scenes with the masked search per tree. */
int32_t ditree_forest_expand_round_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                           const ditree_forest_scenes* scenes, const ditree_round* round,
                                           const ditree_round_params* p, const ditree_bound* bound, void* stream);
/* ditree_accept_best under the bound.  In candidate order every candidate counts (counters[4]), adds its chunks (counters[3])
 * and visits its parent; a collided candidate gets no node; a candidate that did not collide has c = cost[parent] + kept edge
 * states + 1 (kept: after the zero-row filter, so a pre-pass counts the rows before ids are assigned) and f = c + h(end xy),
 * and gets a node slot only if f < U -- else it is pruned: node id -1, stats[1] and [3].  A goal candidate has h = 0: it gets a
 * node only when strictly cheaper than the incumbent.  counters[6] is raised only by a candidate that was neither collided nor
 * pruned.  Commit: ditree_accept_best's, with key[id] beside cost[id].  Pick: ditree_accept_best's, then stats[0] and [2].
 * While counters[1] < 0 nothing is pruned and every array equals ditree_accept_best's.  round->node_id is scratch during the
 * call (it carries f between the pre-pass and the scan). */
int32_t ditree_accept_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_bound* bound,
                              void* stream);
/* ditree_forest_accept_best under each tree's own bound; an empty range leaves the tree and its stats row untouched. */
int32_t ditree_forest_accept_bounded(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                     const ditree_round* round, const ditree_bound* bound, void* stream);

/* ------------------------------------------------------------------ near parent: the planner's `near_radius`
 * The "choose parent" step of RRT*, without steering or rewiring: a sample's parent is not its nearest node but, among the nodes
 * NEAR the sample, the one through which the sample is reached in the fewest path rows.  It needs the cost column of
 * ditree_accept_best and two settings: `radius` in metres, and `reach`, the metres one path row is ASSUMED to cover (a setting,
 * not a theorem, like ditree_bound's).
 * For a query q the candidates C are the nodes the plain search looks at -- nodes 0 .. n_nodes-1, a forest: the query's tree's
 * slots; with a bound only the open ones, key[n] < U, U read on the device as in the section above.
 *   1. d2(n) = dx*dx + dy*dy, and n* = the nearest node of C as ditree_nn_argmin[_bounded] / ditree_forest_nn_argmin[_bounded]
 *      return it: strict '<', lowest index on a tie, a NaN distance never wins.
 *   2. t = sqrt(d2(n*)) + radius, tau2 = t * t, once per query in f64.  Near set N = {n*} + {n in C : d2(n) <= tau2}; n* is a
 *      member by index, so a rounding of t * t below d2(n*) cannot drop it.
 *   3. g(n) = (double)cost[n] + sqrt(d2(n)) / reach.  The parent is the member of N with the smallest g; ties go to the smaller
 *      d2, then to the lower index.  Without the distance term an ancestor inside the radius would always beat its descendant.
 *   4. No node of C with a distance that can win a '<': what the plain scans give -- node 0, a forest: the tree's root.
 * If all of C has equal cost the parent is n*, bit for bit (sqrt, / and + are monotone; ties go to the smaller d2).  Nothing is
 * read that the plain rounds do not have, and no random stream moves. */
typedef struct {
  const int32_t* cost;           /* [dev] (capacity,) as ditree_accept_best's (a forest: indexed by the global slot) */
  double radius;                 /* > 0, metres */
  double reach;                  /* > 0, metres per path row */
} ditree_near;
/* Every call of this section refuses by name (DITREE_E_ARG) before anything is launched: "near: descriptor missing",
 * "near: cost array missing", "near: radius must be > 0 and finite", "near: reach must be > 0 and finite", and -- the calls that
 * take a round -- "near: one rank (round->shard must be 0)"; with a bound, the bound's own refusals too. */

/* ditree_nn_argmin_bounded's arguments and outputs with the rule above; bound == NULL: every node 0 .. n_nodes-1 is a candidate. */
int32_t ditree_nn_argmin_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_near* near, const ditree_bound* bound,
                              const double* queries, int32_t q_stride, int32_t B, int32_t n_nodes, int32_t* out_idx,
                              double* out_state, double* out_prev_action, uint8_t* out_has_prev, void* stream);
/* ditree_forest_nn_argmin_bounded's with the rule above per tree; a tree without a node gives -1 and gathers nothing. */
int32_t ditree_forest_nn_argmin_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_near* near,
                                     const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B,
                                     int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev,
                                     void* stream);
/* ditree_expand_round (bound == NULL) or ditree_expand_round_bounded with this search; every other step is unchanged.  Also
 * refused: "expand_round_near: chunk budgets are not built (p->chunk_budget must be NULL)" -- ditree_chunk_budget runs its own
 * nearest-node search. */
int32_t ditree_expand_round_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_round_params* p,
                                 const ditree_bound* bound, const ditree_near* near, void* stream);
/* ditree_forest_expand_round[_scenes] (bound == NULL) or ditree_forest_expand_round_bounded with this search per tree;
 * scenes == NULL: a plain forest. */
int32_t ditree_forest_expand_round_near(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                        const ditree_forest_scenes* scenes, const ditree_round* round,
                                        const ditree_round_params* p, const ditree_bound* bound, const ditree_near* near,
                                        void* stream);

/* ------------------------------------------------------------------ sparse tree: the planner's `sparse_cell`
 * The witness pruning of SST (Li, Littlefield, Bekris 2016) on a grid: two nodes that end in the same small cell of (x, y, psi)
 * are interchangeable, only the cheaper one -- the cell's REPRESENTATIVE -- goes on being expanded, and a candidate that lands
 * where a cheaper node already stands takes no node at all.  It needs the cost column of ditree_accept_best.
 * The cell of a state (x, y, psi, ..) in tree t, whose map spans W x L metres (extent row t) in nx x ny cells (dims row t):
 *   ix = clamp(floor((x + W / 2) / cell), 0, nx - 1), iy the same with y, L and ny;
 *   a  = psi - 2pi * floor(psi / 2pi), ih = clamp(floor(a / w), 0, nh - 1), 2pi = the double 2.0 * M_PI, w = 2pi / nh as the
 *   caller computed it; the cell is (iy * nx + ix) * nh + ih < stride.  Every operation is a separately rounded IEEE f64 one (no
 *   contraction); the clamps are taken on the floored doubles.  A state whose x, y or psi is not finite has no cell.
 * ACTIVE nodes: node n is active iff it has a cell and (cost[n], n) is the lexicographic minimum over the nodes of its tree in
 * that cell -- a pure function of the tree.  table[t * stride + cell] = ((uint64_t)cost[n] << 32) | n for the cell's active node
 * n (the global slot), all ones for a cell without a node.  The root costs 1 and is always active.
 * The accept (ditree_accept_sparse), per tree, behind what the mode does already (collided candidates get no node; with a bound,
 * candidates with f >= U get none and are counted as pruned):
 *   1. c(b) = cost[parent] + kept edge rows + 1, the cell of b = the cell of its end state.
 *   2. Among the remaining candidates of one cell, goal-reaching ones included, the contender is the one with the smallest (c, b).
 *   3. The contender WINS its cell iff the cell holds no node or c < the representative's cost (strict: an equal cost keeps the
 *      older node).  A winner gets a node.
 *   4. A goal-reaching candidate gets a node in any case; one that did not win its cell is appended inactive.
 *   5. A candidate without a cell gets its node as without the descriptor and is never active.
 *   6. Every other candidate gets node id -1 and counts as dominated.
 *   7. Ids go out in candidate order, as in ditree_accept_best; a winner ranked past the tree's capacity gets no node and does
 *      not become the representative (counters[6] is raised as ever).
 *   8. After the call a winner that got a node is active and is its cell's table entry; the node it displaced is inactive
 *      ("retired": it stays in the tree with its subtree, its paths and its place in the fallback).
 * The searches of this section look at active nodes only (with a bound: active and open); scan order, strict '<' and the tie
 * rules are those of the searches they mask.  A scan without a candidate ends as theirs does. */
typedef struct {
  double cell;                   /* > 0 and finite, metres */
  double w;                      /* 2pi / nh */
  int32_t nh;                    /* heading bins, 1 .. 64 */
  int32_t stride;                /* table entries per tree: >= nx * ny * nh of every tree, <= 2^22 */
  const double* extent;          /* [dev] (T, 2): W, L of each tree's map (a single tree: T = 1) */
  const int32_t* dims;           /* [dev] (T, 2): nx, ny of each tree */
  const int32_t* dims_host;      /* [host] (T, 2) the same numbers: validated before anything is launched */
  uint64_t* table;               /* [dev] (T, stride): written by ditree_sparse_rebuild and the accept */
  uint64_t* scratch;             /* [dev] (T, stride): the contenders of a round; all ones between calls (the rebuild sets it) */
  uint8_t* active;               /* [dev] (capacity,) indexed by the global slot */
  int32_t* stats;                /* [dev] (T, 4): [0] candidates dominated since the rebuild, [1] nodes retired since the rebuild,
                                    [2] active nodes, [3] candidates dominated by the last accept */
  int32_t* cand;                 /* [dev] (2 * B) scratch of the accept: c and the cell of every candidate of the round */
} ditree_sparse;
/* Every call of this section refuses by name (DITREE_E_ARG) before anything is launched: "sparse: descriptor missing",
 * "sparse: cell must be > 0 and finite", "sparse: nh must be 1..64 and w > 0", "sparse: extent / dims missing", "sparse: table,
 * scratch, active or stats missing", "sparse: stride must be 1..2^22", "sparse: nx * ny * nh of tree <t> exceeds the stride",
 * "sparse: cost array missing", -- the accepts -- "sparse: cand scratch missing", "sparse: one rank (round->shard must be 0)", "sparse:
 * a run_type-0 car tree (no obstacle flags or hist)"; with a bound or a near descriptor, their own refusals too. */

/* table, active and stats of trees [first, first + n) from scratch, from the trees as they are (node counts read on the device;
 * forest == NULL: the single tree, first = 0, n = 1): after a reset of a root, and after ditree_tree_rebase -- purity makes that
 * exact; a retired node whose representative was dropped is active again.  stats rows become (0, 0, active nodes, 0). */
int32_t ditree_sparse_rebuild(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_sparse* sparse,
                              const int32_t* cost, int32_t first, int32_t n, void* stream);
/* ditree_accept_best (bound == NULL) or ditree_accept_bounded (cost == bound->cost) with the rule above.  round->node_id is
 * scratch during the call, as in ditree_accept_bounded. */
int32_t ditree_accept_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, int32_t* cost,
                             const ditree_bound* bound, const ditree_sparse* sparse, void* stream);
/* The same per tree of a forest; an empty range leaves the tree, its table rows and its stats row untouched. */
int32_t ditree_forest_accept_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                    const ditree_round* round, int32_t* cost, const ditree_bound* bound,
                                    const ditree_sparse* sparse, void* stream);
/* ditree_nn_argmin_bounded's arguments and outputs over the ACTIVE nodes: near == NULL the nearest node, else the near-parent
 * rule; bound == NULL every active node, else the active and open ones. */
int32_t ditree_nn_argmin_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_sparse* sparse, const ditree_near* near,
                                const ditree_bound* bound, const double* queries, int32_t q_stride, int32_t B, int32_t n_nodes,
                                int32_t* out_idx, double* out_state, double* out_prev_action, uint8_t* out_has_prev, void* stream);
int32_t ditree_forest_nn_argmin_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                       const ditree_sparse* sparse, const ditree_near* near, const ditree_bound* bound,
                                       const double* queries, int32_t q_stride, int32_t B, int32_t* out_idx, double* out_state,
                                       double* out_prev_action, uint8_t* out_has_prev, void* stream);
/* ditree_chunk_budget (forest == NULL) or ditree_forest_chunk_budget (n_nodes not read) with the nearest ACTIVE node (bound !=
 * NULL: active and open) as the parent whose visits are counted. */
int32_t ditree_chunk_budget_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                   const ditree_sparse* sparse, const ditree_bound* bound, const double* samples, int32_t B,
                                   int32_t n_nodes, const int32_t* schedule_chunks, int32_t n_schedule, int32_t* parent_scratch,
                                   int32_t* budget_out, void* stream);
/* ditree_expand_round_near's round (bound and near each NULL or set) with the search over the active nodes; every other step is
 * unchanged.  p->chunk_budget must be NULL, as there. */
int32_t ditree_expand_round_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round, const ditree_round_params* p,
                                   const ditree_bound* bound, const ditree_near* near, const ditree_sparse* sparse, void* stream);
/* ditree_forest_expand_round_near's (scenes == NULL: a plain forest) with the search over each tree's active nodes. */
int32_t ditree_forest_expand_round_sparse(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                          const ditree_forest_scenes* scenes, const ditree_round* round,
                                          const ditree_round_params* p, const ditree_bound* bound, const ditree_near* near,
                                          const ditree_sparse* sparse, void* stream);

/* ------------------------------------------------------------------ re-planning on a kept tree
 * The online driver re-plans from wherever the car stands on its plan (run_scenarios_with_lidar_DiTree.py:397-516).  Instead of
 * starting from an empty tree, ditree_tree_rebase re-roots the tree at the car, keeps the branches that grow from there and
 * still clear the maze uploaded to the ctx, and compacts them to the front of a SECOND tree `dst` of the same shape (src is only
 * read; src and dst share no buffer).  n = src->counters[0] is read on the device.
 *   root_state == NULL: the car stands on node `anchor`, which becomes node 0 (drop_states = drop_actions = 0).
 *   root_state != NULL ([host] S doubles, read during the call): the car is inside anchor's edge.  Node 0 is a fresh node with
 *     that state; anchor becomes node 1 with parent 0 and its edge without the first drop_states state rows and the first
 *     drop_actions action rows, 0 < drop_states < edge_nstates[anchor], 0 <= drop_actions < edge_nactions[anchor].
 *   Node 0 is a root as after a reset: parent -1, no edge rows, has_prev 0, last_action 0, obstacle_ahead 0, cost 1; its
 *   num_visit is anchor's when anchor became it, 0 when it is fresh.
 * Node m is kept iff it is anchor or a descendant of it and no node on the chain anchor .. m is blocked.  A node is blocked when
 * car_collides(x, y, psi) holds for its state or for a kept row of its edge states (a NaN row collides); of anchor's edge only
 * the rows behind the dropped ones count, and none when it becomes the root -- that root is kept even if the car's own pose
 * collides, its subtree then is not.  A blocked anchor leaves node 0 alone: a fresh reset.
 * New ids: the exclusive scan of the keep flags (+ 1 behind a fresh root), so parent < child still holds; parents are remapped.
 * Moved per kept node: state, xy, last_action, has_prev, num_visit, edge_owner, both edge arrays and row counts; obstacle_ahead
 * (where the trees have it) is evaluated again on the current maze.  cost_src / cost_dst [dev] (capacity,) int32, both or
 * neither: the cost column of ditree_accept_best, re-based to the rows of the new paths -- cost'[m] = cost[m] - cost[anchor] +
 * cost'[anchor], cost'[anchor] = 1 as the root, else 1 + its kept edge rows + 1.
 * dst->counters: [0] nodes of dst, [1] the new id of src's goal node / incumbent or -1 when it was not kept, [2..6] 0, [7] -1.
 * scratch [dev]: 3 * src->capacity int32; when the call returns, scratch[2 * capacity + m] is the new id of node m < n, -1 for
 * a node that was dropped.
 * Checked on the device, because n and the row counts live there: a refused call writes DITREE_REBASE_E_DROP (drop counts out
 * of range) or DITREE_REBASE_E_ANCHOR (anchor >= n) to dst->counters[0] -- a tree holds at least its root, so a count <= 0 is the
 * status word -- and touches nothing else of dst.
 * Refused before anything is launched, DITREE_E_ARG: "tree_rebase: the car (a tree with state_dim 6, action_dim 2 and no
 * hist)", "tree_rebase: src and dst share a buffer", "tree_rebase: src and dst differ in shape", "tree_rebase: dst->capacity
 * below src->capacity", "tree_rebase: anchor out of range", "tree_rebase: drop counts belong to a root_state", "tree_rebase:
 * cost_src and cost_dst come together", "tree_rebase: scratch missing", "tree_rebase: obstacle_ahead in one tree only";
 * DITREE_E_STATE: "tree_rebase: no maze uploaded". */
#define DITREE_REBASE_E_DROP (-1)
#define DITREE_REBASE_E_ANCHOR (-2)
int32_t ditree_tree_rebase(ditree_ctx* ctx, const ditree_tree* src, const ditree_tree* dst, int32_t anchor,
                           const double* root_state /*[host] S or NULL*/, int32_t drop_states, int32_t drop_actions,
                           const int32_t* cost_src, int32_t* cost_dst, int32_t* scratch, void* stream);

/* One expansion round of the ANT (BASELINE config 3; cfgs/antmaze.yaml + run_scenarios.py:123-132: action_horizon 2, edge
 * length 48 = 24 chunks, pred_horizon 16, obs_history 3, local map 16 x 16 @ 0.8, s_global 4) against a tree with state_dim
 * 29, action_dim 8 and `hist`: planners/RRT.py:131-194 batched --
 *   nearest node (RRT.py:49-51) -> its state, last action and the last <= 3 rows of its edge (RRT.py:144-147) ->
 *   n_chunks x [create_local_map at (state[0], state[1], state[2]) (RRT.py:158-166: element 2 -- the torso height -- is what
 *   the reference passes as the rotation) -> ant conditioning vector (policies/fm_policy.py:77-143: normalise, quaternion ->
 *   rot6d of the normalised values, 3-step history, previous action, tanh of the goal offset with yaw 0) -> denoiser (input_dim 8)
 *   -> the first A un-normalised actions -> A env steps with goal + collision test (ditree_ant_rollout) ->
 *   prev_states = curr_states_seq, prev_actions = curr_action_seq (RRT.py:186-190)].
 * Fills `round` (status / chunks_run / chunk_steps / states (B, n_chunks, A + 1, 29) / actions (B, n_chunks, A, 8) /
 * end_state); ditree_accept then appends the nodes (emulate_sticky = 0: the ant env has no latched `done`).
 * THE ENV STEP (MuJoCo, not in the reference repository, no oracle) is one of:
 *   DITREE_ANT_DYN_TAPE   next_obs_tape (B, n_chunks, A, 29): observations given from outside (tests, measurement);
 *   DITREE_ANT_DYN_MODEL  the build's stand-in model (ditree_ant_model; parity unpinned, not MuJoCo);
 *   the caller's own simulator, one chunk at a time: ditree_ant_round_begin, then per chunk ditree_ant_chunk_sample (actions of
 *   the chunk -> round->actions[:, j], start states in round->end_state), the host steps its env, ditree_ant_chunk_step with
 *   the observations.  ditree_expand_round_ant is exactly that sequence with the tape / model in the middle. */
#define DITREE_ANT_DYN_TAPE 0
#define DITREE_ANT_DYN_MODEL 1
typedef struct {
  int32_t n_nodes;               /* tree size to search */
  const double* samples;         /* [dev] (B, 29): columns 0, 1 used (the KD-tree is over x, y, RRT.py:23,50) */
  const double* cond_goal;       /* [dev] (B, 2) */
  const float* noise;            /* [dev] (B, n_chunks, P, 8) f32, or NULL with inject_actions */
  const double* inject_actions;  /* [dev] (B, n_chunks, P, 8) f64 or NULL: bypass the denoiser (tests: action tapes) */
  int32_t P;                     /* pred_horizon (16) */
  int32_t K;                     /* flow steps */
  const float* t0;               /* [host] K */
  const float* dt;               /* [host] K */
  const double* norm;            /* [host] 70: obs_mean[27], obs_std[27], act_mean[8], act_std[8] (metadata/antmaze.pt) */
  const double* desired_goal;    /* [host] 2: obs['desired_goal'] of the env (base_planner.py:296) */
  double goal_radius;            /* 0.45 * s_global */
  double ball_radius;            /* 1.2 (base_planner.py:155) */
  const double* axis;            /* [host] local-map axis, lm_n doubles */
  int32_t lm_n;                  /* local_map_size (16) */
  double lm_size;                /* divisor of the goal conditioning */
  double s_global;               /* 4 */
  int32_t dynamics;              /* DITREE_ANT_DYN_* (ditree_expand_round_ant only) */
  const double* next_obs_tape;   /* [dev] (B, n_chunks, A, 29) f64 for DITREE_ANT_DYN_TAPE */
  const ditree_ant_model* model; /* [host] for DITREE_ANT_DYN_MODEL */
  int32_t early_exit;            /* != 0: later chunks run on the still-alive candidates only (RRT.py:179-184) */
  const float* ddpm_coef;        /* [host] (K, 5) or NULL: the DDPM branch, as ditree_round_params */
  const float* step_noise;       /* [dev] (B, n_chunks, K, P, 8) f32 with ddpm_coef */
  float* cond_out;               /* [dev] (B, n_chunks, 97) f32 or NULL: the conditioning vector of every sampler call (tests) */
} ditree_ant_round_params;
int32_t ditree_expand_round_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                const ditree_ant_round_params* p, void* stream);
/* The same round with the caller's simulator between the two halves of a chunk (j = 0 .. n_chunks - 1, in order):
 *   begin:  status / counters reset, nearest node, parent state -> round->end_state, history + previous action -> ctx;
 *   sample: local map, conditioning, denoiser for the candidates that are still alive; round->actions[:, j] <- the A actions;
 *   step:   next_obs [dev] (B, A, 29) f64 = the observation after each of the A env steps from round->end_state[b] with
 *           round->actions[b, j] (rows of candidates that are not alive are ignored; a candidate that collides or reaches the
 *           goal at step i ignores the rows after i) -> tests, round->states[:, j], status, history for the next chunk. */
int32_t ditree_ant_round_begin(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                               const ditree_ant_round_params* p, void* stream);
int32_t ditree_ant_chunk_sample(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                                const ditree_ant_round_params* p, int32_t j, void* stream);
int32_t ditree_ant_chunk_step(ditree_ctx* ctx, const ditree_tree* tree, const ditree_round* round,
                              const ditree_ant_round_params* p, int32_t j, const double* next_obs, void* stream);

/* ------------------------------------------------------------------ ant forests: many seeded antmaze runs in one round
 * The benchmark loop (run_scenarios.py:336-343) for BASELINE config 3: a ditree_forest whose tree is an ANT tree (state_dim 29,
 * action_dim 8, `hist` / `hist_n` present: 20.8 KB per node slot at edge length 48), run_type 0, one rank (no shards, no
 * obstacle flags).  Layout, counter block and candidate offsets are ditree_forest's.  Each of the three calls validates the
 * tree and the forest before anything is launched (DITREE_E_ARG with a message); the car's forest calls keep refusing an ant
 * tree.  The host-stepped triple (ditree_ant_round_begin / _chunk_sample / _chunk_step) has no forest form. */
/* ditree_expand_round_ant on a forest (planners/RRT.py:131-194 for the candidates of every run): each candidate's nearest node
 * is searched in its own tree only (nodes [t * C, t * C + n_t), n_t from the tree's counter row on the device; p->n_nodes is
 * not read), its state, last action, has_prev and -- from the global parent id -- its history rows are gathered; everything
 * behind that is the single-tree ant round.  p->dynamics: DITREE_ANT_DYN_TAPE or DITREE_ANT_DYN_MODEL.  round->B = off[T]. */
int32_t ditree_forest_expand_round_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                       const ditree_round* round, const ditree_ant_round_params* p, void* stream);
/* ditree_accept (planners/RRT.py:195-217) per tree of an ant forest, without the sticky-done emulation (the ant env has no
 * latched `done`): first goal, accepted prefix, iteration / candidate counts and overflow at the tree's own C in its counter
 * row; global node ids from t * C + n_t; every appended node's hist / hist_n rows as the single-tree commit writes them (valid
 * rows at the end of the three slots). */
int32_t ditree_forest_accept_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const ditree_round* round,
                                 void* stream);
/* ditree_forest_fallback (planners/RRT.py:227-254, run_type 0) on an ant forest's xy: goal_xy [host 2] -> out_node [dev] (T,)
 * global ids; the norm as the key, first occurrence on ties, -1 for a tree that holds only its root. */
int32_t ditree_forest_fallback_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest, const double* goal_xy,
                                   int32_t* out_node, void* stream);

/* ------------------------------------------------------------------ ant scene forests: an antmaze scenario set in one round
 * The ant benchmark is a scenario set too (run_scenarios.py:202-233: one maze, start and goal cell per row of
 * experiments/test_scenarios_ant.csv).  An ant scene forest is an ant forest plus a scene id per tree (ditree_forest_scenes) on
 * the scene table of ditree_upload_scenes, whose goal column holds each scene's obs['desired_goal'] (base_planner.py:296).  The
 * accept step is ditree_forest_accept_ant.  Both calls validate everything on the host before anything is launched. */
/* ditree_forest_expand_round_ant with each tree's own scene: every row's local map, collision tests and goal test use its
 * tree's maze and desired goal.  p->desired_goal is not read and no single maze is needed; p->goal_radius, p->ball_radius and
 * p->s_global hold for all scenes.  DITREE_E_STATE without an uploaded scene table; DITREE_E_ARG for a car tree, a sharded
 * round, an incomplete forest or scene descriptor, a scene id outside [0, n uploaded), or p->dynamics that is neither
 * DITREE_ANT_DYN_TAPE nor DITREE_ANT_DYN_MODEL.  Each candidate's arithmetic is the single-maze ant round's on its scene's bytes,
 * dims and goal. */
int32_t ditree_forest_expand_round_ant_scenes(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                              const ditree_forest_scenes* scenes, const ditree_round* round,
                                              const ditree_ant_round_params* p, void* stream);
/* ditree_forest_fallback_ant with one goal per tree: goal_xy [host] (T, 2) (ditree_forest_fallback_goals refuses an ant tree). */
int32_t ditree_forest_fallback_goals_ant(ditree_ctx* ctx, const ditree_tree* tree, const ditree_forest* forest,
                                         const double* goal_xy, int32_t* out_node, void* stream);

/* ------------------------------------------------------------------ policy roll-outs: validation episodes as one batch
 * The closed-loop roll-out of rollout_manager.py:545-838 (what train_diffusion_policy.py:354,481,604 runs on every row of
 * experiments/validation_scenarios_car.csv) for the car: N = S scenes x E episodes, each car driven by the sampler alone --
 * local map at its pose -> conditioning vector (previous action = the last executed one, none before the first step; the
 * goal = its scene's goal) -> sampler -> up to A env steps (car_env.py:371-390) each followed by success = ||xy - goal|| < 0.5
 * (car_env.py:341-350) and is_colliding_car (car_env.py:267-268) -- until it succeeds, collides or has run `step_limit` steps.
 * Mazes and goals come from the scene table of ditree_upload_scenes; episode i lives in scene batch->scene[i].
 * Departures from the reference loop, PARITY UNPINNED: (a) stable-baselines3's DummyVecEnv (not in the
 * reference tree) re-resets a terminated env and hands observations back in its buffer dtype -- here a terminated episode is
 * frozen, `collided` is 0 or 1 and every quantity comes from the float64 env state; (b) terminated episodes are left out of
 * later sampler calls (the denoiser is batch-invariant: nobody else's result changes); (c) best_dist takes the success test's
 * norm, sqrt(fma(dy, dy, dx * dx)), where rollout_manager.py:800 adds the two squares unfused.
 * All arrays [dev], caller-owned, N rows. */
#define DITREE_EP_RUNNING 0         /* = DITREE_ST_OK */
#define DITREE_EP_SUCCESS 1         /* = DITREE_ST_GOAL */
#define DITREE_EP_COLLIDED 2        /* = DITREE_ST_COLLIDED; | DITREE_ST_FLAG_GOAL_AT_COLLISION when the same step also succeeded */
#define DITREE_EP_OUT_OF_STEPS 3    /* n_steps reached step_limit */
typedef struct {
  int32_t N;                     /* episodes */
  int32_t A;                     /* action_horizon: env steps per chunk, 1 .. 64 */
  int32_t max_steps;             /* rows per episode in `rows` */
  const int32_t* scene;          /* (N,) the scene of every episode */
  const int32_t* scene_host;     /* [host] (N,) the same ids: each in [0, n uploaded), validated before anything is launched */
  double* state;                 /* (N, 6) in: start states (ditree_policy_begin does not touch them); live env state */
  double* rows;                  /* (N, max_steps, 8): row t = [state before step t (6) | the action as sampled (2)] */
  int32_t* n_steps;              /* (N,) env steps executed */
  int32_t* success_step;         /* (N,) index of the first successful step, -1 = never */
  int32_t* collided;             /* (N,) 0 / 1 */
  int32_t* status;               /* (N,) DITREE_EP_* */
  double* best_dist;             /* (N,) min over executed steps of the distance to the goal after the step; +inf before */
  double* last_action;           /* (N, 2) the last executed action (as sampled) */
  uint8_t* has_prev;             /* (N,) a step has been executed */
  double* goal_xy;               /* (N, 2) out of ditree_policy_begin: each episode's goal = its scene's (the sampler's goal input) */
  int32_t* idx;                  /* (N,) scratch: the running episodes, in episode order */
} ditree_policy_batch;
typedef struct {
  int32_t step_limit;            /* max_episode_steps: an episode stops in the middle of a chunk when it is reached; <= max_steps */
  const float* noise;            /* (N, P, 2) f32: the chunk's start noise for the WHOLE batch (fm_policy.py:158), or NULL with tape */
  const double* tape;            /* (N, P, 2) f64 or NULL: the chunk's actions given from outside -- no map, conditioning, sampler */
  int32_t P;                     /* pred_horizon >= A */
  int32_t K;                     /* flow / DDPM steps */
  const float* t0;               /* [host] K */
  const float* dt;               /* [host] K */
  const double* norm;            /* [host] 16 doubles, see ditree_cond_vector */
  const double* axis;            /* [host] local-map axis, lm_n doubles */
  int32_t lm_n;                  /* local_map_size */
  double lm_size;                /* the divisor of the goal conditioning */
  double s_global;
  const float* ddpm_coef;        /* [host] (K, 5) or NULL, as ditree_round_params */
  const float* step_noise;       /* (N, K, P, 2) f32 with ddpm_coef */
} ditree_policy_params;
/* Start a batch of episodes: n_steps = 0, success_step = -1, collided = 0, status = RUNNING, best_dist = +inf, has_prev = 0,
 * last_action = 0, goal_xy = the scene's goal, idx = 0 .. N - 1.  The ctx remembers the batch (by its idx array) and its running
 * count.  Validated like ditree_policy_chunk ("policy_begin: ..."); needs the scene table. */
int32_t ditree_policy_begin(ditree_ctx* ctx, const ditree_policy_batch* batch, void* stream);
/* One chunk of the loop (rollout_manager.py:706-807) for the running episodes: [local maps -> conditioning -> sampler (flow
 * steps, or the DDPM loop with p->ddpm_coef) ->] up to A env steps with the bookkeeping above, then the list of the episodes
 * still running is rebuilt; its length and the kernel's own count of running episodes are read back (one 8-byte D2H per chunk;
 * they must agree) -> *n_active_out [host].  With p->tape the bracketed steps are skipped.  A ctx follows ONE batch at a time:
 * a chunk on another batch than the one last begun (or chunked) is DITREE_E_STATE.  A chunk on a batch with no running episode
 * launches nothing and returns 0.
 * Everything is validated before anything is launched: DITREE_E_STATE "policy_chunk: no scene table uploaded" / "policy_chunk:
 * call ditree_policy_begin on this batch first"; DITREE_E_ARG "policy_chunk: batch descriptor incomplete", "policy_chunk: need
 * 1 <= A <= 64, A <= P and 1 <= step_limit <= max_steps", "policy_chunk: episode i has scene id k, out of range [0, n)",
 * "policy_chunk: neither noise nor an action tape", "policy_chunk: flow schedule missing", "policy_chunk: the DDPM branch needs
 * step_noise", "policy_chunk: ... do not match the loaded denoiser (...; the car's is action_dim 2, cond 7)". */
int32_t ditree_policy_chunk(ditree_ctx* ctx, const ditree_policy_batch* batch, const ditree_policy_params* p,
                            int32_t* n_active_out /*[host]*/, void* stream);

/* ------------------------------------------------------------------ plan polishing: shorten a found plan's action tape
 * A post-processing step of the build's own (no counterpart in the reference: PARITY UNPINNED, like MPPI; DESIGN.md section 3
 * "Plan polishing"; the numpy restatement is tests/polish_ref.py) on the pinned pieces: the car step (car_env.py:356-396), the
 * two-ball collision test (common/map_utils.py:103-115), the goal radius (car_env.py:341-354), and ditree_mppi_step's normal
 * generator.  A plan is a start state x0, a goal, a maze and an action tape U (T rows of 2).
 *   Rolling a tape: X[0] = x0; row t = 0 .. T - 1: X[t + 1] = car_step(X[t], clip(U[t])), then the collision test and the goal
 *     test of the expansion rounds on X[t + 1], collision first (a colliding row is a collision even inside the radius).
 *     d_t = sqrt(fma(dy, dy, dx * dx)) of X[t] against the goal, the rounds' goal norm.
 *   A tape ARRIVES at s rows when X[s] is the first state inside the radius (d_s < 0.5) and no X[1 .. s] collides; its arrival
 *     time is tau = (s - 1) + (d_{s-1} - 0.5) / (d_{s-1} - d_s)  [rows, continuous].
 *   Replay: the input tape is rolled.  It is refused -- its status set, every other output of the plan untouched, no iteration
 *     run on it -- when it collides, does not arrive within its rows, starts inside the radius (d_0 < 0.5), or holds a row up to
 *     its arrival that is not f32-exact (u != (double)(float)u: the planner's actions are float32, and so is every tape this
 *     call writes).  Else the incumbent is the tape cut to its s rows: T* = s, tau*, states X*[0 .. T*].
 *   Iteration n = 0 .. N - 1, candidate k = 0 .. K - 1:
 *     first perturbed row a = H(seed, n, k) mod T*, with splitmix64 as ditree_mppi_step's generator uses it
 *       (x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *       z ^ z >> 31):   h = splitmix64(seed ^ splitmix64(n));  h = splitmix64(h ^ k * 0xD1B54A32D192ED03);
 *       H = splitmix64(h ^ 0xA24BAED4963EE407);
 *     noise eps[k, b] for the block b = t div hold of the ABSOLUTE row index t = ditree_mppi_step's generator at (seed,
 *       counter = n, k, t = b, sigma);
 *     candidate action u_k[t] = (double)(float) clip(U*[t] + (t >= a ? eps[k, t div hold] : 0)), the clip the env's (the
 *       replay keeps the input's rows as given, so a row outside the env's range is stored clipped once a candidate wins);
 *     the candidate is rolled for at most T* rows.  It is integrated from X*[a] on (rows < a are the incumbent's own), which
 *       gives what rolling its whole tape from x0 gives.
 *   Select: the winner is the arriving candidate with the smallest tau, ties to the lowest k; if tau_k < tau* STRICTLY its
 *     tape cut to its s rows and its states become the incumbent, else nothing changes.
 *   Hence: the result is a rolled, collision-free, arriving tape; rows never grow; tau never grows; sigma = 0 returns the
 *   replayed plan.
 * Two launches per iteration (roll-outs: a grid of K-slices x plans, one candidate per lane, each work-group's (tau, k) minimum
 * and arriving count; commit: one work-group per plan reduces the slices in index order, applies the strict test and re-rolls
 * the winner once into tape / states / trace), all N iterations enqueued without a host read: T* and tau* live in rows and
 * arrival.  Results are a pure function of the arguments (a second identical call leaves the same bits), and a plan's results
 * do not depend on the other plans of the call.
 *   n_plans plans; scene == NULL: all against the maze of ditree_upload_maze; else plan i against the maze of scene scene[i] of
 *     ditree_upload_scenes (the table's goal column is not read: goals are per plan).  Every maze used holds at most
 *     DITREE_POLISH_MAX_CELLS cells (it is staged in LDS).
 *   x0 [dev] (n_plans, 6), goal_xy [dev] (n_plans, 2) f64; tape [dev] (n_plans, capacity, 2) f64 in / out, rows [0, T*) count;
 *     rows [dev] (n_plans,) i32 in: the rows of each input tape, 1 .. capacity, out: T*; rows_host [host] the input values again,
 *     validated before anything is launched; states [dev] (n_plans, capacity + 1, 6) f64, rows 0 .. T* written; arrival [dev] (n_plans, 2) f64 = tau of the replay, tau*; status [dev] (n_plans,) i32
 *     DITREE_POLISH_*; trace [dev] (n_plans, N, DITREE_POLISH_TRACE) f64 per iteration: winner k (-1: nothing arrived), its tau
 *     (+inf then), accepted 0 / 1, T* and tau* after the iteration, arriving candidates.
 *   noise [dev] (N, K, noise_blocks, 2) f64 or NULL, first_row [dev] (N, K) i32 or NULL replace the generator and the hash for
 *     every plan alike (tests): a = r mod T* for r = first_row[n, k] >= 0, max(T* + r, 0) for r < 0 (-1: the last row).
 * DITREE_E_ARG by name: a null pointer, n_plans < 1, state_dim / action_dim other than the car's 6 / 2 (the ant is not built),
 * K not a positive multiple of 64, N < 0, hold < 1, sigma not finite or negative, capacity < 1, a tape longer than the
 * capacity, noise_blocks * hold < capacity with noise, a scene id out of range, a maze past DITREE_POLISH_MAX_CELLS;
 * DITREE_E_STATE without the maze / scene table asked for. */
#define DITREE_POLISH_OK 0
#define DITREE_POLISH_NO_ARRIVAL 1      /* the tape's rows end outside the goal radius */
#define DITREE_POLISH_COLLIDES 2
#define DITREE_POLISH_START_IN_GOAL 3   /* d_0 < 0.5 */
#define DITREE_POLISH_NOT_F32 4         /* a row up to the arrival is not f32-exact */
#define DITREE_POLISH_TRACE 6
#define DITREE_POLISH_MAX_CELLS 16384
typedef struct {
  int32_t n_plans;
  int32_t state_dim, action_dim;     /* 6, 2 */
  int32_t capacity;                  /* rows per plan in `tape`; `states` holds capacity + 1 */
  int32_t K, N, hold;                /* candidates per iteration, iterations, rows per noise block */
  double sigma[2];
  uint64_t seed;
  const int32_t* scene;              /* [dev] (n_plans,) or NULL */
  const int32_t* scene_host;         /* [host] the same ids */
  const double* x0;
  const double* goal_xy;
  double* tape;
  int32_t* rows;
  const int32_t* rows_host;          /* [host] the rows of every input tape */
  double* states;
  double* arrival;
  int32_t* status;
  double* trace;
  const double* noise;
  int32_t noise_blocks;
  const int32_t* first_row;
} ditree_polish;
int32_t ditree_polish_plans(ditree_ctx* ctx, const ditree_polish* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DITREE_H */
