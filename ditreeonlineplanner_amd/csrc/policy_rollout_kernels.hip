// Policy roll-outs (include/ditree.h "policy roll-outs"): the env-step half of one chunk of rollout_manager.py:706-807 for a
// batch of car episodes spread over the scenes of a scene table.  Compiled with -ffp-contract=off like every unit that
// includes car_device.h: the flags must be bit-exact against the CPU oracle.
#include "car_device.h"
#include "ditree_internal.h"

// ditree_policy_begin: the bookkeeping of a fresh batch (rollout_manager.py:693-703) and the list of running episodes = all.
__global__ void policy_begin_kernel(const SceneTable* __restrict__ tab, ditree_policy_batch bt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= bt.N) return;
  bt.n_steps[b] = 0;
  bt.success_step[b] = -1;
  bt.collided[b] = 0;
  bt.status[b] = DITREE_EP_RUNNING;
  bt.best_dist[b] = __longlong_as_double(0x7ff0000000000000LL);       // np.inf
  bt.last_action[(size_t)b * 2] = 0.0;
  bt.last_action[(size_t)b * 2 + 1] = 0.0;
  bt.has_prev[b] = 0;
  const SceneRec sc = tab->rec[bt.scene[b]];
  bt.goal_xy[(size_t)b * 2] = sc.gx;
  bt.goal_xy[(size_t)b * 2 + 1] = sc.gy;
  bt.idx[b] = b;
}
void launch_policy_begin(const SceneArg& sc, const ditree_policy_batch& b, hipStream_t s) {
  hipLaunchKernelGGL(policy_begin_kernel, dim3((b.N + 255) / 256), dim3(256), 0, s, sc.table, b);
}

// Up to A env steps of every running episode: one lane per episode, rows idx[0 .. n_run).
//   The design is car_rollout_kernel<1, false, true, true>'s (geom_kernels.hip, DESIGN.md section 5 "The rollout kernels against
//   their roofline"): what a step costs is ONE sequential FP64 chain per lane -- Euler step -> norm -> two-ball test, each
//   instruction waiting for its predecessor -- so the loop must hold nothing else that waits.  The whole atlas (<= 16 KB) is
//   staged into LDS once per work-group, before the early returns; a lane reads its scene record, state and bookkeeping next to
//   each other; its A action rows (A <= 64) go into lane-private LDS slots by bursts of sixteen loads issued back to back (slot q
//   of lane t at (q * blockDim + t) * 16 bytes: no bank conflicts, no barrier -- a lane reads only what it wrote); an explicit
//   vmcnt(0) stands in front of the step loop, so that no wait for a load sits inside it (vmcnt retires in order and counts
//   stores: a wait for a load inside the loop would also wait for the previous step's row store).  The loop then holds the chain,
//   six LDS cell reads per ball behind one wait (car_device.h) and one 64-byte row store per step, which nothing waits for.
//   Work-groups of 64 threads: a validation batch (96 .. 3 072 episodes) fills a fraction of the SIMDs, one wave per group spreads
//   it over the most CUs.  The launch is a few microseconds next to the sampler call of the same chunk (tens of milliseconds).
// Per step t = n_steps (rollout_manager.py:767-804): row t = [state, action as sampled]; car_step with the clipped action;
// success = ||xy - goal|| < 0.5 (np.linalg.norm of a 2-vector: one fma) and collision = is_colliding_car, both may be set by the
// same step; best_dist = min(best_dist, that norm) (np.minimum: NaN wins); the step ends the episode on either flag; the loop
// stops in the middle of the chunk when step_limit is reached.
__global__ void __launch_bounds__(64)
policy_episode_kernel(const SceneTable* __restrict__ tab, int atlas_cells, ditree_policy_batch bt, int n_run,
                      const double* __restrict__ actions, int64_t act_stride, int act_dense, int step_limit,
                      int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  {
    const unsigned char* g = scene_atlas(tab);
    for (int i = threadIdx.x; i < atlas_cells; i += blockDim.x) lds[i] = g[i];
    __syncthreads();
  }
  const int ob = blockIdx.x * blockDim.x + threadIdx.x;
  if (ob >= n_run) return;
  const int b = bt.idx[ob];                          // actions of the sampler are dense (row ob), everything else per episode
  if (bt.status[b] != DITREE_EP_RUNNING) return;
  const SceneRec sc = tab->rec[bt.scene[b]];
  const unsigned char* mz = lds + sc.offset;
  const int H = sc.rows, W = sc.cols;
  const double gx = sc.gx, gy = sc.gy;
  const int n0 = bt.n_steps[b];
  const int A = min(bt.A, step_limit - n0);          // steps this chunk may take (<= 0: the episode was out of steps already)
  double s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = bt.state[(size_t)b * 6 + k];
  double best = bt.best_dist[b];
  int succ = bt.success_step[b];
  const double* act = actions + (size_t)(act_dense ? ob : b) * act_stride;
  double2* abuf = reinterpret_cast<double2*>(lds + (((size_t)atlas_cells + 15) & ~(size_t)15)) + threadIdx.x;
  const int bd = blockDim.x;
  for (int i0 = 0; i0 < A; i0 += 16) {
    double2 t[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = min(i0 + q, A - 1);
      t[q] = double2{act[2 * r], act[2 * r + 1]};
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) abuf[(i0 + q) * bd] = t[q];
  }
  double* row = bt.rows + ((size_t)b * bt.max_steps + n0) * 8;
  int status = DITREE_EP_RUNNING, steps = 0, coll_any = 0;
  double la0 = 0.0, la1 = 0.0;
  __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): every load above has arrived before the step loop
  for (int i = 0; i < A; ++i) {
    const double2 a = abuf[i * bd];
#pragma unroll
    for (int k = 0; k < 6; ++k) row[k] = s[k];       // traj[~done, curr_step] = [obs, action]
    row[6] = a.x;
    row[7] = a.y;
    row += 8;
    car_euler_step(s, a.x, a.y);                     // car_env.py:371-390 (clips the action itself)
    steps = i + 1;
    la0 = a.x; la1 = a.y;
    const double ex = s[0] - gx, ey = s[1] - gy;
    const double dist = sqrt(fma(ey, ey, ex * ex));
    const bool done = dist < 0.5;                    // car_env.py:341-350
    const bool coll = car_collides(s[0], s[1], s[2], mz, H, W);                   // car_env.py:267-268
    best = (dist < best || dist != dist) ? dist : best;                           // np.minimum(best_dist, dist)
    if (done && succ < 0) succ = n0 + i;
    if (coll) {
      coll_any = 1;
      status = DITREE_EP_COLLIDED | (done ? DITREE_ST_FLAG_GOAL_AT_COLLISION : 0);
      break;
    }
    if (done) {
      status = DITREE_EP_SUCCESS;
      break;
    }
  }
  const int n1 = n0 + steps;
  if (status == DITREE_EP_RUNNING && n1 >= step_limit) status = DITREE_EP_OUT_OF_STEPS;
#pragma unroll
  for (int k = 0; k < 6; ++k) bt.state[(size_t)b * 6 + k] = s[k];
  bt.n_steps[b] = n1;
  bt.success_step[b] = succ;
  if (coll_any) bt.collided[b] = 1;
  bt.status[b] = status;
  bt.best_dist[b] = best;
  if (steps > 0) {
    bt.last_action[(size_t)b * 2] = la0;
    bt.last_action[(size_t)b * 2 + 1] = la1;
    bt.has_prev[b] = 1;
  }
  if (status == DITREE_EP_RUNNING) atomicAdd(count, 1);
}

void launch_policy_episode(const SceneArg& sc, const ditree_policy_batch& b, int n_run, const double* actions, int64_t act_stride,
                           int act_dense, int step_limit, int32_t* count, hipStream_t s) {
  const int blk = 64;
  // atlas (<= 16 KB) + 64 lanes x 64 action rows x 16 B = at most 80 KB: above the 64 KB default
  const size_t lds = (((size_t)sc.atlas_cells + 15) & ~(size_t)15) + (size_t)blk * 64 * sizeof(double2);
  static bool attr_done_dev[64] = {};                        // the attribute is per kernel AND per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!(dev >= 0 && dev < 64 && attr_done_dev[dev])) {
    (void)hipFuncSetAttribute((const void*)policy_episode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (dev >= 0 && dev < 64) attr_done_dev[dev] = true;
  }
  (void)hipMemsetAsync(count, 0, sizeof(int32_t), s);
  hipLaunchKernelGGL(policy_episode_kernel, dim3((n_run + blk - 1) / blk), dim3(blk), lds, s, sc.table, sc.atlas_cells, b, n_run,
                     actions, act_stride, act_dense, step_limit, count);
}
