// Per-candidate kinodynamic kernels of the DiTree expansion path (gfx950, FP64).
//
// This translation unit is compiled with -ffp-contract=off: the reference computes
// every expression with separately rounded numpy operations, and flags / parent
// indices must be bit-exact against the CPU oracle, so no a*b+c may be fused here
// except where the reference's LAPACK does (lidar border solve, explicit fma()).
//
// Reference sites (paths relative to the reference root):
//   nn_argmin      planners/RRT.py:49-51 (KDTree.query k=1 on state[:2])
//   local_map      common/map_utils.py:391-459
//   cond_vector    policies/fm_policy.py:60-143 (car branch)
//   car_rollout    planners/base_planner.py:257-320, car_env.py:341-396,
//                  common/map_utils.py:103-115,221-329
//   lidar_scan     lidar_sim/lidar_2d_sim.py:18-98
//   accept/commit  planners/RRT.py:179-217
#include "car_device.h"
#include "ditree_internal.h"
#include "lidar_device.h"

#define WAVE 64

// ------------------------------------------------------------------------- maze
__global__ void maze_convert_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float v = src[i];
    int c = (int)v;
    dst[i] = (v == (float)c && c >= 0 && c < 256) ? (unsigned char)c : (unsigned char)255;
  }
}
void launch_maze_convert(const float* src, unsigned char* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(maze_convert_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
}

// Stage the maze into LDS (cells are single bytes; every shipped maze is <= 31x31).
__device__ __forceinline__ void stage_maze(unsigned char* lds, const unsigned char* __restrict__ g, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) lds[i] = g[i];
  __syncthreads();
}

// ------------------------------------------------------------------------- nearest node, near parent
// One scan trip (scan_nodes), one nearest pass (nearest), one near-parent search on top of it (near_parent), one tree lookup
// (tree_of_query) and one gather epilogue (write_parent) behind the four kernels: nn_argmin_kernel / nn_near_kernel serve a single
// tree with NN_QPW queries per wave, nn_forest_kernel / nn_forest_near_kernel a forest with one query per wave.
#define NN_QPW 4
// The bound of a branch-and-bound round (include/ditree.h ditree_bound): U = cost[incumbent] as the tree's counter row names
// it, INT32_MAX without one.  The counter row is not written between a round's nearest-node search and its accept's pick, so
// every kernel of the round reads the same value.
__device__ __forceinline__ int bound_of(const int32_t* __restrict__ counters, const int32_t* __restrict__ cost) {
  const int inc = counters[1];
  return inc < 0 ? 0x7fffffff : cost[inc];
}
// The rows a path from (x, y) still needs at best to reach the goal disc, at `reach` metres per row: the norm is
// fallback_select_kernel's, sqrt(fma(dy, dy, dx*dx)); 0 inside the disc and for a NaN distance, at most 2^30.  The one place
// where the mode's heuristic is computed (keys of new nodes, keys of roots, the accept's pre-pass).
__device__ __forceinline__ int bound_h(double x, double y, double gx, double gy, double goal_radius, double reach) {
  const double dx = x - gx, dy = y - gy;
  const double d = sqrt(fma(dy, dy, dx * dx));
  const double q = (d - goal_radius) / reach;
  if (!(q > 0.0)) return 0;
  const double c = ceil(q);
  return c < 1073741824.0 ? (int)c : 1073741824;
}
// MASK (the planner's "anytime_pruned" mode, ditree_nn_argmin_bounded): only open nodes, key[n] < U, take part in the compare
// -- eight more independent coalesced i32 loads per trip beside the eight double2 loads; a closed node is masked exactly as an
// index past N is.  Scan order, strict '<' and the reduction are unchanged, so with U = INT32_MAX the result is the unmasked
// kernel's, and a scan without an open node ends as an all-NaN scan does (node 0).
// MASK is a bit set: MASK_KEY the mask above, MASK_ACTIVE (include/ditree.h "sparse tree") only nodes with active[n] != 0 take part
// -- eight byte loads per trip --, both: nodes that are active and open.
#define MASK_KEY 1
#define MASK_ACTIVE 2
// The one scan trip of the nearest pass: lane `lane` of a wave strides the n nodes of the segment that starts at slot `base`
// of xy / key / active, eight nodes per trip.  Their loads are independent (one load - wait - compare round per node exposes
// a memory round trip n / 64 times: 1.1 ms of a round at 10^5 nodes), only the visitor's running minima chain: eight double2
// loads, eight key loads under MASK_KEY, eight byte loads under MASK_ACTIVE.  Indices past n are clamped for the load and
// masked for the compare; visit(index, xy) sees the nodes that take part in increasing index.  `base` is a 32-bit term of the
// index, not an offset of the pointers: that costs nn_forest_kernel<false, 3> 15 VGPRs and a step (profiles/NOTES.md).
template <int MASK, class Visit>
__device__ __forceinline__ void scan_nodes(const double2* __restrict__ xy, const int32_t* __restrict__ key,
                                           const uint8_t* __restrict__ active, int base, int n, int U, int lane, Visit visit) {
  for (int i = lane; i < n; i += 8 * WAVE) {
    double2 p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = xy[base + min(i + u * WAVE, n - 1)];
    int kk[8];
    if constexpr (MASK & MASK_KEY) {
#pragma unroll
      for (int u = 0; u < 8; ++u) kk[u] = key[base + min(i + u * WAVE, n - 1)];
    }
    uint8_t aa[8];
    if constexpr (MASK & MASK_ACTIVE) {
#pragma unroll
      for (int u = 0; u < 8; ++u) aa[u] = active[base + min(i + u * WAVE, n - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int iu = i + u * WAVE;
      bool in = iu < n;
      if constexpr (MASK & MASK_KEY) in = in && kk[u] < U;
      if constexpr (MASK & MASK_ACTIVE) in = in && aa[u] != 0;
      if (in) visit(iu, p[u]);
    }
  }
}
// The nearest of the n nodes to each of a wave's Q queries: the scan with strict '<' per lane (a lane keeps its lowest index),
// then the 64-lane arg-min reduction carrying (distance, index), ties -> lowest index.  best[k] / bidx[k] hold the result in
// every lane; NaN distances never win a '<', so a scan without a winner (all NaN, all closed, all inactive, n = 0) leaves
// 0x7fffffff, which the callers clamp to the segment's first node.
// NORM: the key of the fallback choice (planners/RRT.py:233-237, np.argmin of np.linalg.norm(state[:2] - goal)) instead of the
// squared distance: sqrt(fma(dy, dy, dx*dx)) as fallback_select_kernel and oracle/rrt.py::fallback_node compute it.  sqrt merges
// neighbouring doubles, so two nodes whose squares differ in the last place can have equal norms; the reference then returns
// the lower index, which the square's strict '<' would not.  The expansion search (NORM = false) keeps the squared distance:
// it is pinned bit for bit to the KDTree goldens.
template <int MASK, int Q, bool NORM, class Found>
__device__ __forceinline__ void nearest(const double2* __restrict__ xy, const int32_t* __restrict__ key,
                                        const uint8_t* __restrict__ active, int base, int n, int U, const double (&qx)[Q],
                                        const double (&qy)[Q], int lane, Found found) {
  double best[Q];
  int bidx[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    best[k] = __builtin_huge_val();
    bidx[k] = 0x7fffffff;
  }
  scan_nodes<MASK>(xy, key, active, base, n, U, lane, [&](int iu, const double2& p) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      double dx = qx[k] - p.x, dy = qy[k] - p.y;
      double d;
      if constexpr (NORM) d = sqrt(fma(dy, dy, dx * dx));
      else d = dx * dx + dy * dy;
      if (d < best[k]) { best[k] = d; bidx[k] = iu; }     // strict: keeps the lowest index per lane
    }
  });
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    double d = best[k];
    int ix = bidx[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      double od = __shfl_xor(d, m);
      int oi = __shfl_xor(ix, m);
      if (od < d || (od == d && oi < ix)) { d = od; ix = oi; }
    }
    found(k, d, ix);
  }
}
// The "choose parent" search (include/ditree.h "near parent"): among the nodes NEAR the query, the one through which the query
// is reached in the fewest path rows, in two passes over the same nodes.
//   pass 1: nearest() -> n*, the nearest node, in every lane; then tau2 = (sqrt(d2(n*)) + radius)^2, once per query.
//   pass 2: the same nodes again, with the cost loads.  A node takes part when d2 <= tau2, or when it is n* itself (by index:
//           a rounding of t * t below d2(n*) cannot drop it).  Of these only a node that can still win pays the FP64 sqrt and
//           the divide of g = cost + sqrt(d2) / reach: every candidate has d2 >= d2(n*), and sqrt, / and + round monotonically,
//           so g >= cost + sqrt(d2(n*)) / reach, one add per node; above the lane's running minimum the node is out (equal: it
//           may still tie, and is evaluated).  Near nodes are scattered over the lanes, so without this bound the branch is
//           taken by a third of the wave-steps at a radius of one cell (one near lane is enough); with it, by the few nodes
//           whose cost is within radius / reach rows of the lane's best.  The running minimum is (g, d2) with strict '<', so a
//           lane keeps its lowest index; the reduction carries (g, d2, index): ties in g go to the smaller d2, then to the lower
//           index.
// res[k]: the parent's index in the segment, 0x7fffffff when no node had a distance that wins a '<' (all NaN, all closed, n = 0),
// which the callers clamp as nearest()'s.  With equal costs g is monotone in d2 and the result is n*.
template <int MASK, int Q>
__device__ __forceinline__ void near_parent(const double2* __restrict__ xy, const int32_t* __restrict__ key,
                                            const uint8_t* __restrict__ active, const int32_t* __restrict__ cost, int base, int n, int U,
                                            const double (&qx)[Q], const double (&qy)[Q], double radius, double reach, int lane,
                                            int (&res)[Q]) {
  int bidx[Q];
  double tau2[Q], gfloor[Q];
  bool any = false;
  nearest<MASK, Q, false>(xy, key, active, base, n, U, qx, qy, lane, [&](int k, double d, int ix) __attribute__((always_inline)) {
    bidx[k] = ix;                                       // n* in every lane
    const double sd = sqrt(d);
    const double t = sd + radius;
    tau2[k] = t * t;
    gfloor[k] = sd / reach;                             // g(n) >= cost[n] + gfloor for every candidate n
    any = any || ix != 0x7fffffff;
    res[k] = 0x7fffffff;
  });
  if (!any) return;                                     // wave-uniform: no query of the wave has a nearest node
  double bg[Q], bd[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    bg[k] = __builtin_huge_val();
    bd[k] = __builtin_huge_val();
  }
  // Pass 2 keeps its own copy of scan_nodes' trip (plus the eight cost loads).  Run through the shared trip, the compiler folds
  // the bound test into the near test and every node pays the FP64 add: nn_near_kernel then takes 6 % longer at a radius of
  // 0.5 m (10^5 and 10^6 nodes) and 8 % less at 2 m; with the near test marked unlikely it is the other way round.  Neither
  // is the time it had, so this loop stays as it was (profiles/NOTES.md, "Nearest-node search: one scan body").  For one query
  // per wave (nn_forest_near_kernel) both forms compile to the same instructions, so that kernel loses nothing by sharing it.
  for (int i = lane; i < n; i += 8 * WAVE) {
    double2 p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = xy[base + min(i + u * WAVE, n - 1)];
    int cc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) cc[u] = cost[base + min(i + u * WAVE, n - 1)];
    int kk[8];
    if constexpr (MASK & MASK_KEY) {
#pragma unroll
      for (int u = 0; u < 8; ++u) kk[u] = key[base + min(i + u * WAVE, n - 1)];
    }
    uint8_t aa[8];
    if constexpr (MASK & MASK_ACTIVE) {
#pragma unroll
      for (int u = 0; u < 8; ++u) aa[u] = active[base + min(i + u * WAVE, n - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int iu = i + u * WAVE;
      bool in = iu < n;
      if constexpr (MASK & MASK_KEY) in = in && kk[u] < U;
      if constexpr (MASK & MASK_ACTIVE) in = in && aa[u] != 0;
      if (in) {
        const double c = (double)cc[u];
#pragma unroll
        for (int k = 0; k < Q; ++k) {
          double dx = qx[k] - p[u].x, dy = qy[k] - p[u].y;
          double d = dx * dx + dy * dy;
          if ((d <= tau2[k] || iu == bidx[k]) && !(c + gfloor[k] > bg[k])) {      // near, and not yet out by the bound on g
            const double g = c + sqrt(d) / reach;
            if (g < bg[k] || (g == bg[k] && d < bd[k])) { bg[k] = g; bd[k] = d; res[k] = iu; }
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    double g = bg[k], d = bd[k];
    int ix = res[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      double og = __shfl_xor(g, m), od = __shfl_xor(d, m);
      int oi = __shfl_xor(ix, m);
      if (og < g || (og == g && (od < d || (od == d && oi < ix)))) { g = og; d = od; ix = oi; }
    }
    res[k] = ix;
  }
}
// The tree of candidate row q of a forest: the last tree whose range [off[t], off[t+1]) starts at or before q (empty ranges are
// skipped); without offsets, one row per tree.
__device__ __forceinline__ int tree_of_query(const int32_t* __restrict__ off, int T, int q) {
  if (off == nullptr) return q;
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= q) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// What a search leaves for query q, by the whole wave: the chosen node's index and, where the caller gathers (a.state != NULL),
// its state (lanes < S; S <= 64), last action (lanes 32 .. 32 + D) and flag (lane 63).
__device__ __forceinline__ void write_parent(const NnArg& a, int q, int ix, int lane) {
  if (lane == 0) a.out_idx[q] = ix;
  if (a.state != nullptr) {
    if (lane < a.S) a.out_state[(size_t)q * a.S + lane] = a.state[(size_t)ix * a.S + lane];
    if (lane >= 32 && lane < 32 + a.D) a.out_prev_action[(size_t)q * a.D + (lane - 32)] = a.last_action[(size_t)ix * a.D + (lane - 32)];
    if (lane == 63) a.out_has_prev[q] = a.has_prev[ix];
  }
}
// The search of one tree: one wave per group of NN_QPW queries over nodes 0 .. N-1.  NEAR: the near-parent rule instead of the
// nearest node.  No candidate -> node 0.
template <int MASK, bool NEAR>
__device__ __forceinline__ void tree_search(const NnArg& a, const NnTree& seg) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int q0 = wave * NN_QPW;
  if (q0 >= a.B) return;
  int U = 0x7fffffff;
  if constexpr (MASK & MASK_KEY) U = bound_of(seg.counters, a.bcost);
  double qx[NN_QPW], qy[NN_QPW];
#pragma unroll
  for (int k = 0; k < NN_QPW; ++k) {
    int q = min(q0 + k, a.B - 1);
    qx[k] = a.queries[(size_t)q * a.q_stride + 0];
    qy[k] = a.queries[(size_t)q * a.q_stride + 1];
  }
  auto chosen = [&](int k, int ix) __attribute__((always_inline)) {
    if (q0 + k < a.B) write_parent(a, q0 + k, ix == 0x7fffffff ? 0 : ix, lane);
  };
  if constexpr (NEAR) {
    int res[NN_QPW];
    near_parent<MASK, NN_QPW>(a.xy, a.key, a.active, a.cost, 0, seg.N, U, qx, qy, a.radius, a.reach, lane, res);
#pragma unroll
    for (int k = 0; k < NN_QPW; ++k) chosen(k, res[k]);
  } else {
    nearest<MASK, NN_QPW, false>(a.xy, a.key, a.active, 0, seg.N, U, qx, qy, lane,
                                 [&](int k, double, int ix) __attribute__((always_inline)) { chosen(k, ix); });
  }
}
// The segmented search of a forest (include/ditree.h ditree_forest): query q belongs to tree t = tree_of_query and searches only
// that tree's node slots [t*C + skip, t*C + n_t), n_t read from the tree's counter row (never past the tree's own slots), under
// the tree's own bound U; key, cost and active are indexed by the global slot.  Queries of one wave may belong to different trees
// (at one candidate per run they always do), so every wave takes one query; the scan is tree_search's, so the result is
// tree_search's on the segment alone (no candidate -> the segment's first slot).  A segment with no node gives -1 and gathers nothing.
template <bool NORM, int MASK, bool NEAR>
__device__ __forceinline__ void forest_search(const NnArg& a, const NnForest& seg) {
  const int lane = threadIdx.x & 63;
  const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (q >= a.B) return;
  const int t = tree_of_query(seg.off, seg.T, q);
  const int base = t * seg.C + seg.skip;
  int n = seg.counters[t * 8] - seg.skip;
  n = n > seg.C - seg.skip ? seg.C - seg.skip : n;
  if (n <= 0) {
    if (lane == 0) a.out_idx[q] = -1;
    return;
  }
  int U = 0x7fffffff;
  if constexpr (MASK & MASK_KEY) U = bound_of(seg.counters + (size_t)t * 8, a.bcost);
  const double qx[1] = {a.queries[(size_t)q * a.q_stride + 0]}, qy[1] = {a.queries[(size_t)q * a.q_stride + 1]};
  int res[1];
  if constexpr (NEAR) near_parent<MASK, 1>(a.xy, a.key, a.active, a.cost, base, n, U, qx, qy, a.radius, a.reach, lane, res);
  else nearest<MASK, 1, NORM>(a.xy, a.key, a.active, base, n, U, qx, qy, lane, [&](int, double, int ix) { res[0] = ix; });
  write_parent(a, q, base + (res[0] == 0x7fffffff ? 0 : res[0]), lane);
}
// The four kernels: MASK = 0 reads none of key / bcost / active, and only the near kernels read cost / radius / reach.
// nn_argmin_kernel names the waves per SIMD it has always had (4 with both masks, 5 otherwise): left to itself the MASK_ACTIVE
// instantiation takes 98 VGPRs, two over the step.
template <int MASK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MASK == (MASK_KEY | MASK_ACTIVE) ? 4 : 5)))
nn_argmin_kernel(NnArg a, NnTree seg) { tree_search<MASK, false>(a, seg); }
template <int MASK>
__global__ void __launch_bounds__(256) nn_near_kernel(NnArg a, NnTree seg) { tree_search<MASK, true>(a, seg); }
template <bool NORM, int MASK = 0>
__global__ void __launch_bounds__(256) nn_forest_kernel(NnArg a, NnForest seg) { forest_search<NORM, MASK, false>(a, seg); }
template <int MASK>
__global__ void __launch_bounds__(256) nn_forest_near_kernel(NnArg a, NnForest seg) { forest_search<false, MASK, true>(a, seg); }

// f(the MASK of a search with these columns, as a compile-time constant)
template <class F>
static void with_mask(const void* key, const void* active, F f) {
  if (active) {
    if (key) f(std::integral_constant<int, MASK_KEY | MASK_ACTIVE>{}); else f(std::integral_constant<int, MASK_ACTIVE>{});
  } else {
    if (key) f(std::integral_constant<int, MASK_KEY>{}); else f(std::integral_constant<int, 0>{});
  }
}
void launch_nn(const NnArg& a, const NnTree& seg, hipStream_t s) {
  const int waves = (a.B + NN_QPW - 1) / NN_QPW;
  with_mask(a.key, a.active, [&](auto m) {
    constexpr int M = decltype(m)::value;
    hipLaunchKernelGGL(a.cost ? nn_near_kernel<M> : nn_argmin_kernel<M>, dim3((waves + 3) / 4), dim3(256), 0, s, a, seg);
  });
}
void launch_nn(const NnArg& a, const NnForest& seg, hipStream_t s) {
  if (seg.norm) {
    hipLaunchKernelGGL(nn_forest_kernel<true>, dim3((a.B + 3) / 4), dim3(256), 0, s, a, seg);
    return;
  }
  with_mask(a.key, a.active, [&](auto m) {
    constexpr int M = decltype(m)::value;
    hipLaunchKernelGGL((a.cost ? nn_forest_near_kernel<M> : nn_forest_kernel<false, M>), dim3((a.B + 3) / 4), dim3(256), 0, s, a, seg);
  });
}
// The fallback choice of every tree (planners/RRT.py:233-237): query t is tree t's goal, the scan covers its nodes 1.. with the
// norm as the key.
void launch_forest_fallback(const double* goals, int T, const double* node_xy, const int32_t* counters, int C, int32_t* out_idx,
                            hipStream_t s) {
  const NnArg a{goals, 2, T, (const double2*)node_xy, nullptr, nullptr, nullptr, 6, 2, out_idx,
                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0};
  launch_nn(a, NnForest{nullptr, T, counters, C, 1, true}, s);
}

// ------------------------------------------------------------------------- local map
// One workgroup per candidate; maze staged in LDS; one thread per output cell.
// SCENES (a scene forest, include/ditree.h "scene forests"): `maze` is the scene table (SceneTable); the work-group stages only
// its candidate's maze from the atlas and uses that scene's dims for the centre and the clipping.
template <bool SCENES>
__global__ void __launch_bounds__(256)
local_map_kernel(const unsigned char* __restrict__ maze, int rows, int cols, const double* __restrict__ state,
                 int state_stride, const int32_t* __restrict__ active, const int32_t* __restrict__ idx, int n, AxisArg axis,
                 double s_global, int scaled, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int ob = blockIdx.x;                                        // dense output row
  const int b = idx ? idx[ob] : ob;                                 // candidate (compacted rounds pass an index list)
  if (active != nullptr && active[b] != DITREE_ST_OK) return;      // block-uniform
  if constexpr (SCENES) {
    const SceneTable* tab = reinterpret_cast<const SceneTable*>(maze);
    const SceneRec sc = tab->rec[tab->row_scene[b]];
    rows = sc.rows;
    cols = sc.cols;
    stage_maze(lds, scene_atlas(tab) + sc.offset, rows * cols);
  } else {
    stage_maze(lds, maze, rows * cols);
  }
  // RRT.py:158-166 passes curr_state[0], curr_state[1], curr_state[2] for every env (for the ant, element 2 is the torso
  // height, not a heading -- the reference's own behaviour, kept)
  const double x = state[(size_t)b * state_stride + 0], y = state[(size_t)b * state_stride + 1], th = state[(size_t)b * state_stride + 2];
  double c, sn;
  sincos(th, &sn, &c);          // one range reduction; ocml's sin / cos evaluate the same kernels (identical values)
  // base_planner.py:88-89,100-101,113-114: centre = (W/2, H/2) * maze_size_scaling (car: 1, ant: s_global = 4); RRT.py:166
  const double cx = (double)cols / 2.0 * s_global, cy = (double)rows / 2.0 * s_global;
  for (int cell = threadIdx.x; cell < n * n; cell += blockDim.x) {
    int i = cell / n, j = cell - i * n;                             // meshgrid: x_local[i][j] = xs[j], y_local = ys[i]
    double xl = axis.v[j], yl = axis.v[i];
    double xg = c * xl - sn * yl + x;                               // map_utils.py:443
    double yg = sn * xl + c * yl + y;                               // :444
    double fy = floor((cy - yg) / s_global);                        // :447
    double fx = floor((xg + cx) / s_global);                        // :448
    // np.clip after astype(int): NaN / huge values become INT64_MIN in numpy -> clip to 0
    int yi = (fy >= 0.0) ? ((fy < (double)rows) ? (int)fy : rows - 1) : 0;
    int xi = (fx >= 0.0) ? ((fx < (double)cols) ? (int)fx : cols - 1) : 0;
    float m = (float)lds[yi * cols + xi];
    out[(size_t)ob * n * n + cell] = scaled ? (m * 2.0f - 1.0f) : m;
  }
}
void launch_local_map(const unsigned char* maze, int rows, int cols, const double* state, const int32_t* active,
                      const int32_t* idx, int B, int n, const AxisArg& axis, double s_global, int scaled, float* out,
                      hipStream_t s, int state_stride) {
  size_t lds = ((size_t)rows * cols + 15) & ~(size_t)15;
  hipLaunchKernelGGL(local_map_kernel<false>, dim3(B), dim3(256), lds, s, maze, rows, cols, state, state_stride, active, idx, n, axis,
                     s_global, scaled, out);
}
void launch_local_map_scenes(const SceneArg& sc, const double* state, const int32_t* active, const int32_t* idx, int B, int n,
                             const AxisArg& axis, double s_global, float* out, hipStream_t s, int state_stride) {
  const size_t lds = ((size_t)sc.max_cells + 15) & ~(size_t)15;
  hipLaunchKernelGGL(local_map_kernel<true>, dim3(B), dim3(256), lds, s, (const unsigned char*)sc.table, 0, 0, state, state_stride, active,
                     idx, n, axis, s_global, 1, out);
}
// The scene of every candidate row: tree_scene[t] for the tree whose range [off[t], off[t+1]) holds the row (tree_of_query).
__global__ void row_scene_kernel(const int32_t* __restrict__ off, int T, const int32_t* __restrict__ tree_scene, int B,
                                 int32_t* __restrict__ row_scene) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  row_scene[q] = tree_scene[tree_of_query(off, T, q)];
}
void launch_row_scene(const int32_t* off, int T, const int32_t* tree_scene, int B, int32_t* row_scene, hipStream_t s) {
  hipLaunchKernelGGL(row_scene_kernel, dim3((B + 255) / 256), dim3(256), 0, s, off, T, tree_scene, B, row_scene);
}

// ------------------------------------------------------------------------- conditioning vector
__global__ void cond_vector_kernel(const double* __restrict__ state, const double* __restrict__ prev_action,
                                   const uint8_t* __restrict__ has_prev, const double* __restrict__ cond_goal,
                                   const int32_t* __restrict__ idx, int B, NormArg nm, double lm_size,
                                   float* __restrict__ out) {
  const int ob = blockIdx.x * blockDim.x + threadIdx.x;
  if (ob >= B) return;
  const int b = idx ? idx[ob] : ob;
  const double* st = state + (size_t)b * 6;
  float* o = out + (size_t)ob * 7;
  // fm_policy.py:76,108,110,112: normalise in f64, drop x,y,psi, cast to f32
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = (float)((st[3 + k] - nm.obs_mean[3 + k]) / nm.obs_std[3 + k]);
  // :113-123: zeros stay un-normalised when prev_actions is None
  if (has_prev[b]) {
    o[3] = (float)((prev_action[(size_t)b * 2 + 0] - nm.act_mean[0]) / nm.act_std[0]);
    o[4] = (float)((prev_action[(size_t)b * 2 + 1] - nm.act_mean[1]) / nm.act_std[1]);
  } else {
    o[3] = 0.0f;
    o[4] = 0.0f;
  }
  // :125-143 in f32: g = float(goal - pos); R(-yaw) g; tanh(g / lm_size)
  float gx = (float)(cond_goal[(size_t)b * 2 + 0] - st[0]);
  float gy = (float)(cond_goal[(size_t)b * 2 + 1] - st[1]);
  float yaw = (float)st[2];
  float c = cosf(yaw), sn = sinf(yaw);
  float rx = c * gx + sn * gy;
  float ry = (-sn) * gx + c * gy;
  float sc = (float)lm_size;
  o[5] = tanhf(rx / sc);
  o[6] = tanhf(ry / sc);
}
void launch_cond_vector(const double* state, const double* prev_action, const uint8_t* has_prev,
                        const double* cond_goal, const int32_t* idx, int B, const NormArg& nm, double lm_size,
                        float* out, hipStream_t s) {
  hipLaunchKernelGGL(cond_vector_kernel, dim3((B + 255) / 256), dim3(256), 0, s, state, prev_action, has_prev,
                     cond_goal, idx, B, nm, lm_size, out);
}

// policies/fm_policy.py:60-143, antmaze branch.  obs (B, n_hist, 29) f64: [x, y | 27 observations]; the 27 are normalised
// (:77), the quaternion is taken FROM THE NORMALISED values (:78, elements 3..6 = x, y, z, w) and replaced by the first two
// columns of its rotation matrix (common/se3_utils.py:177-189), the last `obs_history` = 3 steps are kept (zero rows in
// front when fewer are given, :96-102), x, y dropped (:107): 3 x 29 = 87 values; then the previous action (8, normalised;
// raw zeros when there is none, :113-123) and tanh((goal - position) / local_map_size) with yaw = 0 (:82,125-143).
// Two input forms: obs (B, n_rows, 29) with n_rows = n_hist given steps each (hist_n == NULL), or -- the round's buffers --
// obs (B, 3, 29) with the hist_n[b] valid steps at the END of the three rows (n_rows = 3).  idx: compacted rounds (dense output
// row ob <- candidate idx[ob]).
__global__ void cond_vector_ant_kernel(const double* __restrict__ obs, int n_rows, const int32_t* __restrict__ hist_n,
                                       const double* __restrict__ prev_action,
                                       const uint8_t* __restrict__ has_prev, const double* __restrict__ cond_goal,
                                       const int32_t* __restrict__ idx, int B,
                                       AntNormArg nm, double lm_size, float* __restrict__ out) {
  const int ob = blockIdx.x * blockDim.x + threadIdx.x;
  if (ob >= B) return;
  const int b = idx ? idx[ob] : ob;
  const int n_hist = hist_n ? hist_n[b] : n_rows;
  float* o = out + (size_t)ob * 97;
  for (int hs = 0; hs < 3; ++hs) {                        // slot hs of the 3-step history <- given step hs - (3 - n_hist)
    const int src = hs - (3 - n_hist) + (n_rows - n_hist);          // the valid steps are the LAST n_hist of the n_rows rows
    float* oh = o + hs * 29;
    if (hs < 3 - n_hist) {
      for (int k = 0; k < 29; ++k) oh[k] = 0.0f;
      continue;
    }
    const double* st = obs + ((size_t)b * n_rows + src) * 29;
    double v[27];
    for (int k = 0; k < 27; ++k) v[k] = (st[2 + k] - nm.obs_mean[k]) / nm.obs_std[k];
    // obs_seq[..., 3:7] = v[1..4] = (qx, qy, qz, qw)
    const double qx = v[1], qy = v[2], qz = v[3], qw = v[4];
    const double r00 = 1.0 - 2.0 * (qy * qy + qz * qz);
    const double r10 = 2.0 * (qx * qy + qw * qz);
    const double r20 = 2.0 * (qx * qz - qw * qy);
    const double r01 = 2.0 * (qx * qy - qw * qz);
    const double r11 = 1.0 - 2.0 * (qx * qx + qz * qz);
    const double r21 = 2.0 * (qy * qz + qw * qx);
    oh[0] = (float)v[0];                                  // torso height
    oh[1] = (float)r00; oh[2] = (float)r10; oh[3] = (float)r20; oh[4] = (float)r01; oh[5] = (float)r11; oh[6] = (float)r21;
    for (int k = 5; k < 27; ++k) oh[2 + k] = (float)v[k];  // obs_seq[..., 7:] -> 22 values
  }
  float* oa = o + 87;
  if (has_prev[b]) {
    for (int k = 0; k < 8; ++k) oa[k] = (float)((prev_action[(size_t)b * 8 + k] - nm.act_mean[k]) / nm.act_std[k]);
  } else {
    for (int k = 0; k < 8; ++k) oa[k] = 0.0f;
  }
  const double* last = obs + ((size_t)b * n_rows + (n_rows - 1)) * 29;        // position = obs_seq[:, -1, :2] (:74)
  const float gx = (float)(cond_goal[(size_t)b * 2 + 0] - last[0]);
  const float gy = (float)(cond_goal[(size_t)b * 2 + 1] - last[1]);
  const float sc = (float)lm_size;
  // yaw = 0: the rotation matrix [[1, 0], [-0, 1]] leaves g unchanged
  o[95] = tanhf(gx / sc);
  o[96] = tanhf(gy / sc);
}
void launch_cond_vector_ant(const double* obs, int n_rows, const int32_t* hist_n, const double* prev_action, const uint8_t* has_prev,
                            const double* cond_goal, const int32_t* idx, int B, const AntNormArg& nm, double lm_size, float* out,
                            hipStream_t s) {
  hipLaunchKernelGGL(cond_vector_ant_kernel, dim3((B + 127) / 128), dim3(128), 0, s, obs, n_rows, hist_n, prev_action, has_prev,
                     cond_goal, idx, B, nm, lm_size, out);
}

// ------------------------------------------------------------------------- reference path behind the obstacle
// planners/RRT.py:83-111 extract_path_after_obstacle: c = argmin_i ||cur - path_i|| (first occurrence, np.linalg.norm along
// axis 1 = sqrt(dx*dx + dy*dy)) in the dtype numpy gives `env.state[:2] - path[:, :2]` -- float64 when the env state is float64
// (after any env step; the f32 path is promoted), float32 right after env.reset (car_env.py:215 builds a float32 state) --;
// over rest = path[c:], cells by cell_xy_to_rowcol (the path's f32, floor); i_b = first rest index in an occupied cell (none: -1, the reference then indexes the LAST point); then the
// reference's while loop walks to the first free point j >= i_b and returns rest[j + 1:] (k = j + 1; the blocked run reaching
// the end gives k = len(rest); no crossing gives k = -1, i.e. the last point alone when that one is free).
// out[0] = c, out[1] = k.  One work-group; the path is a few hundred to a few thousand points.
__global__ void __launch_bounds__(256)
path_after_obstacle_kernel(const float* __restrict__ path, int stride, int P, double cx, double cy, int f32_state,
                           const unsigned char* __restrict__ maze, int rows, int cols, int32_t* __restrict__ out) {
  __shared__ double s_d[256];
  __shared__ int s_i[256];
  __shared__ int s_c, s_ib, s_j;
  const int tid = threadIdx.x;
  double best = __builtin_huge_val();
  int bi = 0x7fffffff;
  for (int i = tid; i < P; i += 256) {
    double d;
    if (f32_state) {
      const float dx = (float)cx - path[(size_t)i * stride], dy = (float)cy - path[(size_t)i * stride + 1];
      d = (double)sqrtf(dx * dx + dy * dy);
    } else {
      const double dx = cx - (double)path[(size_t)i * stride], dy = cy - (double)path[(size_t)i * stride + 1];
      d = sqrt(dx * dx + dy * dy);
    }
    if (d < best) { best = d; bi = i; }
  }
  s_d[tid] = best; s_i[tid] = bi;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
      const double od = s_d[tid + o];
      const int oi = s_i[tid + o];
      if (od < s_d[tid] || (od == s_d[tid] && oi < s_i[tid])) { s_d[tid] = od; s_i[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) { s_c = s_i[0]; s_ib = 0x7fffffff; s_j = 0x7fffffff; }
  __syncthreads();
  const int c = s_c, n = P - c;
  const float yc = (float)rows / 2.0f, xc = (float)cols / 2.0f;
  auto blocked = [&](int r) {                               // rest index r -> occupied cell?
    const float x = path[(size_t)(c + r) * stride], y = path[(size_t)(c + r) * stride + 1];
    const int i = (int)floorf((yc - y) / 1.0f), j = (int)floorf((x + xc) / 1.0f);
    // numpy would wrap a negative index and raise beyond the map: paths of a planner stay inside; clamp instead of faulting
    const int ii = min(max(i, 0), rows - 1), jj = min(max(j, 0), cols - 1);
    return maze[ii * cols + jj] == 1;
  };
  int mine = 0x7fffffff;
  for (int r = tid; r < n; r += 256)
    if (blocked(r)) { mine = r; break; }
  if (mine != 0x7fffffff) atomicMin(&s_ib, mine);
  __syncthreads();
  const int ib = s_ib;
  if (ib == 0x7fffffff) {                                   // no crossing: the reference looks at the last point
    if (tid == 0) { out[0] = c; out[1] = blocked(n - 1) ? n : -1; }
    return;
  }
  mine = 0x7fffffff;
  for (int r = ib + tid; r < n; r += 256)
    if (!blocked(r)) { mine = r; break; }
  if (mine != 0x7fffffff) atomicMin(&s_j, mine);
  __syncthreads();
  if (tid == 0) { out[0] = c; out[1] = s_j == 0x7fffffff ? n : s_j + 1; }
}
void launch_path_after_obstacle(const float* path, int stride, int P, double cx, double cy, int f32_state, const unsigned char* maze,
                                int rows, int cols, int32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(path_after_obstacle_kernel, dim3(1), dim3(256), 0, s, path, stride, P, cx, cy, f32_state, maze, rows, cols, out);
}

// ------------------------------------------------------------------------- rollout
// planners/base_planner.py:257-320 + car_env.py:240-282,341-396 + common/map_utils.py:103-115 for a batch of candidates.
// One lane per candidate: the A Euler steps with their goal + two-ball collision tests are a sequential FP64 chain of
// ~ 800 instructions per step (2 sincos, cos, tanh, 2 hypot, sqrt; round 3: 1 200).  Work-group size by batch (launcher): one wave
// per group spreads a small batch over many CUs (the round's 1 024 candidates: 16 CUs instead of 4), 256 threads once every
// SIMD has a wave anyway.
//   The kernel is bound by that FP64 chain with one wave per SIMD (dependent FP64 instructions, ~ 8 cycles each), not by HBM:
//   65 536 x 16 steps take 41.6 us with candidate-minor rows, 35.6 us without any row stores (round 3: 66.6 us); HBM-side
//   traffic 94.3 MB for 93.8 MB of algorithmic bytes (round 3: 214 MB).  What it took, each step measured on its own
//   (profiles/NOTES.md): lockstep stores of candidate-minor rows; the action rows staged per lane in LDS by
//   one burst of loads per 16 steps and an explicit vmcnt(0) in front of the step loop (vmcnt counts stores: any wait for a load
//   inside the loop also waited for the previous step's row stores); one sincos per sin / cos pair, the nearest-corner test,
//   branch-free cell tests, tanh through expm1 (car_device.h, fp64_device.h).  Measured and dropped: wave-cooperative LDS staging
//   with barriers (100 us), register prefetch of the next steps' actions, software-pipelined steps, a wave-specialised two-wave
//   form, work-groups of 128 threads (+ 27 %).
// G lanes per candidate (1 or 2).  G = 2: both lanes of a pair integrate the (identical) dynamics, lane g tests ball g and the
// pair ORs by one lane exchange, lane 0 stores the state rows and lane 1 the action rows -- twice the waves for the same batch
// (two per SIMD at 65 536 candidates), each with a shorter chain per step.  Same arithmetic, same results.
// SCENES (a scene forest, include/ditree.h "scene forests"): `maze` is the scene table (SceneTable) and rows x cols its atlas
// size; the whole atlas is staged, and each lane reads its candidate's scene record -- atlas offset, dims, goal -- next to its
// state, before the vmcnt(0) below.  From there on every test is the single-maze kernel's on that scene's bytes, dims and goal.
template <int G, bool LOCKSTEP, bool STAGE, bool SCENES>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2)))   // the action burst holds 64 registers: no spills
car_rollout_kernel(const unsigned char* __restrict__ maze, int rows, int cols, double* __restrict__ state_io,
                   const double* __restrict__ actions, int64_t act_stride, int32_t* __restrict__ status_io, int B,
                   int A, double gx, double gy, double* __restrict__ states_out, ditree_strides sl,
                   double* __restrict__ actions_out, ditree_strides al, int32_t* __restrict__ steps_out,
                   int64_t steps_stride, int32_t* __restrict__ chunks_run, double* __restrict__ prev_action_io,
                   uint8_t* __restrict__ has_prev_io, const int32_t* __restrict__ idx, int act_dense,
                   const int32_t* __restrict__ budget, int chunk_j, ChunkStrides cs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  if constexpr (SCENES)
    stage_maze(lds, scene_atlas(reinterpret_cast<const SceneTable*>(maze)), rows * cols);
  else
    stage_maze(lds, maze, rows * cols);
  const int ob = (blockIdx.x * blockDim.x + threadIdx.x) / G, g = threadIdx.x & (G - 1);
  if (ob >= B) return;
  const int b = idx ? idx[ob] : ob;                 // compacted rounds: actions are dense (row ob), the rest per candidate
  if (status_io[b] != DITREE_ST_OK) return;
  const unsigned char* mz = lds;                    // this candidate's maze in LDS and its dims
  int H = rows, W = cols;
  if constexpr (SCENES) {
    const SceneTable* tab = reinterpret_cast<const SceneTable*>(maze);
    const SceneRec sc = tab->rec[tab->row_scene[b]];
    mz = lds + sc.offset;
    H = sc.rows;
    W = sc.cols;
    gx = sc.gx;
    gy = sc.gy;
  }
  // chunk_j < 0 (pool-scheduled early-exit rounds: one launch holds candidates at DIFFERENT chunks of their edges): the chunk
  // is the number of chunks this candidate has finished; the chunk-0 bases are offset by it
  if (chunk_j < 0) {
    chunk_j = chunks_run[b];
    if (states_out) states_out += (size_t)chunk_j * cs.states;
    if (actions_out) actions_out += (size_t)chunk_j * cs.actions_out;
    if (steps_out) steps_out += chunk_j;
    if (!act_dense) actions += (size_t)chunk_j * cs.actions_in;
  }
  if (budget != nullptr && chunk_j >= budget[b]) return;      // this visit's edge is shorter (prop_duration schedule)
  double s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = state_io[(size_t)b * 6 + k];
  const double* act = actions + (size_t)(act_dense ? ob : b) * act_stride;
  // STAGE: a lane copies sixteen steps of ITS actions into its LDS slots in ONE burst of loads (issued back to back, one wait) and
  // reads them back step by step -- no barrier (a lane only reads what it wrote); slot q of lane t at (q * blockDim + t) * 16: no
  // bank conflicts.  Two things are wrong with a 16-byte global load per step: the same 128-byte line is touched eight times up to
  // 4 us apart (re-fetched when the store stream has evicted it: 29 ... 114 MB per launch for 20 MB), and -- worse -- vmcnt retires
  // in order and counts stores, so waiting for step i's load also waits for the row stores of step i - 1: 45 % of the wave
  // cycles were s_waitcnt (profiles/r04_rollout_pmc_sq.json).  With the burst the step loop holds no global load at all.
  double2* abuf = STAGE ? reinterpret_cast<double2*>(lds + (((size_t)rows * cols + 15) & ~(size_t)15)) + threadIdx.x : nullptr;
  const int bd = blockDim.x;
  auto action_at = [&](int i, double& a0, double& a1) {
    if constexpr (STAGE) {
      if ((i & 15) == 0) {
        // sixteen named values, not an array: the scheduling barrier below is opaque to the optimiser, an array on its two sides
        // would stay in scratch memory
#define ACT_LD(q) const double2 t##q = *reinterpret_cast<const double2*>(act + 2 * min(i + q, A - 1))
        ACT_LD(0); ACT_LD(1); ACT_LD(2); ACT_LD(3); ACT_LD(4); ACT_LD(5); ACT_LD(6); ACT_LD(7);
        ACT_LD(8); ACT_LD(9); ACT_LD(10); ACT_LD(11); ACT_LD(12); ACT_LD(13); ACT_LD(14); ACT_LD(15);
#undef ACT_LD
        __builtin_amdgcn_sched_barrier(0);                        // all sixteen loads in flight before the first LDS write waits
#define ACT_ST(q) abuf[q * bd] = t##q
        ACT_ST(0); ACT_ST(1); ACT_ST(2); ACT_ST(3); ACT_ST(4); ACT_ST(5); ACT_ST(6); ACT_ST(7);
        ACT_ST(8); ACT_ST(9); ACT_ST(10); ACT_ST(11); ACT_ST(12); ACT_ST(13); ACT_ST(14); ACT_ST(15);
#undef ACT_ST
      }
      const double2 v = abuf[(i & 15) * bd];
      a0 = v.x; a1 = v.y;
    } else {
      a0 = act[2 * i]; a1 = act[2 * i + 1];
    }
  };
  // G = 2: lane 0 owns the state rows, lane 1 the action rows
  // row i, component k of a candidate's block: base + i * row + k * comp (packed rows: {6, 1}; step-major SoA: {6 B, B} --
  // then the 64 lanes of a wave store 512 contiguous bytes)
  double* so = (states_out && (G == 1 || g == 0)) ? states_out + (size_t)b * sl.cand : nullptr;
  double* ao = (actions_out && (G == 1 || g == 1)) ? actions_out + (size_t)b * al.cand : nullptr;
  if (so) {
#pragma unroll
    for (int k = 0; k < 6; ++k) so[k * sl.comp] = s[k];                         // states_sequence[0] = state
  }
  int status = DITREE_ST_OK;
  int steps = 0;
  double la0 = 0.0, la1 = 0.0;
  int i = 0;
  // Everything loaded so far (state, status, indices) has arrived BEFORE the step loop.  Left to the compiler, the wait for these
  // loads sits at their first use inside the loop, as vmcnt(0) -- and vmcnt counts the row stores of the previous step too: every
  // step then waited for its predecessor's stores to reach memory.
  __builtin_amdgcn_s_waitcnt(0x0F70);                                            // vmcnt(0)
  if constexpr (LOCKSTEP) {
    // Candidate-minor rows (sl.cand == 1) are stored in LOCKSTEP: every lane of the wave stores row i + 1 in the same
    // instruction -- its state while its edge is running, the zero row (base_planner.py:282) once it has ended -- so every store
    // is a whole 512-byte run.  (A lane that zero-filled its tail later, on its own, wrote partial sectors that the memory
    // system first had to fetch: 162 MB per launch for 94 MB of algorithmic bytes at 65 536 x 16, 111 MB in lockstep --
    // profiles/r04_rollout_*pmc_traffic.json.)
    bool alive = true;
    for (i = 0; i < A; ++i) {
      double c0r, c1r;
      action_at(i, c0r, c1r);
      if (alive) {
        car_euler_step(s, c0r, c1r);
        steps = i + 1;
        la0 = c0r; la1 = c1r;
      } else if (status == DITREE_ST_GOAL) {
        c0r = 0.0; c1r = 0.0;                                                     // :314-317; a collided edge's tail is copied through
      }
      if (so) {
#pragma unroll
        for (int k = 0; k < 6; ++k) so[(size_t)(i + 1) * sl.row + k * sl.comp] = alive ? s[k] : 0.0;
      }
      if (ao) { ao[(size_t)i * al.row] = c0r; ao[(size_t)i * al.row + al.comp] = c1r; }
      bool coll = false, done = false;
      if (alive) {
        const double ex = s[0] - gx, ey = s[1] - gy;
        done = sqrt(fma(ey, ey, ex * ex)) < 0.5;    // np.linalg.norm (ddot rounds as one fma), car_env.py:346-351
      }
      if constexpr (G == 2) {                       // both lanes of a pair stay in step (the exchange below is pair-wide)
        int mine = 0;
        if (alive) {
          const double off = 0.15 * 0.5, sgn = g ? -1.0 : 1.0;                   // common/map_utils.py:103-115: lane g, ball g
          double sps, cps;
          sincos(s[2], &sps, &cps);
          const double ox = off * cps, oy = off * sps;
          mine = ball_collides(s[0] + sgn * ox, s[1] + sgn * oy, mz, H, W) ? 1 : 0;
        }
        coll = (mine | __shfl_xor(mine, 1)) != 0;
      } else if (alive) {
        coll = car_collides(s[0], s[1], s[2], mz, H, W);                           // base_planner.py:306
      }
      if (alive && coll) {
        status = DITREE_ST_COLLIDED | (done ? DITREE_ST_FLAG_GOAL_AT_COLLISION : 0);
        alive = false;
      } else if (alive && done) {                                                 // :314-317
        status = DITREE_ST_GOAL;
        alive = false;
      }
    }
  } else {
    for (; i < A; ++i) {
      double a0r, a1r;
      action_at(i, a0r, a1r);
      car_euler_step(s, a0r, a1r);
      steps = i + 1;
      if (so) {
#pragma unroll
        for (int k = 0; k < 6; ++k) so[(size_t)(i + 1) * sl.row + k * sl.comp] = s[k];
      }
      if (ao) { ao[(size_t)i * al.row] = a0r; ao[(size_t)i * al.row + al.comp] = a1r; }
      la0 = a0r; la1 = a1r;
      double ex = s[0] - gx, ey = s[1] - gy;
      bool done = sqrt(fma(ey, ey, ex * ex)) < 0.5;   // np.linalg.norm (ddot rounds as one fma), car_env.py:346-351
      bool coll;                                                                   // base_planner.py:306
      if constexpr (G == 2) {
        const double off = 0.15 * 0.5, sgn = g ? -1.0 : 1.0;                       // common/map_utils.py:103-115: lane g, ball g
        double sps, cps;
        sincos(s[2], &sps, &cps);
        const double ox = off * cps, oy = off * sps;
        const int mine = ball_collides(s[0] + sgn * ox, s[1] + sgn * oy, mz, H, W) ? 1 : 0;
        coll = (mine | __shfl_xor(mine, 1)) != 0;
      } else {
        coll = car_collides(s[0], s[1], s[2], mz, H, W);
      }
      if (coll) {
        status = DITREE_ST_COLLIDED | (done ? DITREE_ST_FLAG_GOAL_AT_COLLISION : 0);
        ++i;
        break;
      }
      if (done) {                                                                   // :314-317
        status = DITREE_ST_GOAL;
        ++i;
        break;
      }
    }
    // rows after the last executed step stay zero (states :282; actions zeroed :315)
    for (int r = i; r < A; ++r) {
      if (so) {
#pragma unroll
        for (int k = 0; k < 6; ++k) so[(size_t)(r + 1) * sl.row + k * sl.comp] = 0.0;
      }
      if (ao) {
        // only the goal branch zeroes the remaining actions (:314-317); a collided edge is discarded
        // by the caller, its untouched tail is copied through like the reference's array
        const bool z = (status == DITREE_ST_GOAL);
        ao[(size_t)r * al.row] = z ? 0.0 : act[2 * r];
        ao[(size_t)r * al.row + al.comp] = z ? 0.0 : act[2 * r + 1];
      }
    }
  }
  if (G == 2 && g != 0) return;                       // per-candidate results: lane 0
#pragma unroll
  for (int k = 0; k < 6; ++k) state_io[(size_t)b * 6 + k] = s[k];
  status_io[b] = status;
  if (steps_out) steps_out[(size_t)b * steps_stride] = steps;
  if (chunks_run) chunks_run[b] += 1;
  if (status == DITREE_ST_OK && prev_action_io) {                                 // RRT.py:188
    prev_action_io[(size_t)b * 2 + 0] = la0;
    prev_action_io[(size_t)b * 2 + 1] = la1;
    if (has_prev_io) has_prev_io[b] = 1;
  }
}
void launch_car_rollout_ex(const unsigned char* maze, int rows, int cols, double* state_io, const double* actions,
                           int64_t act_stride, int32_t* status_io, int B, int A, double gx, double gy,
                           double* states_out, ditree_strides states_stride, double* actions_out, ditree_strides actout_stride,
                           int32_t* steps_out, int64_t steps_stride, int32_t* chunks_run, double* prev_action_io,
                           uint8_t* has_prev_io, const int32_t* idx, int act_dense, hipStream_t s, const int32_t* budget,
                           int chunk_j, ChunkStrides cs, const SceneArg* scenes) {
  if (scenes) {                                              // the whole atlas is staged (rows = 1 x cols = its cells)
    maze = (const unsigned char*)scenes->table;
    rows = 1;
    cols = scenes->atlas_cells;
  }
  size_t lds = ((size_t)rows * cols + 15) & ~(size_t)15;
  // lane-private LDS staging of the action rows (DITREE_ROLLOUT_STAGE=0 turns it off; needs 16-byte aligned rows): 65 536 x 16,
  // candidate-minor rows: 114 -> 20.4 MB fetched per launch (total 188 -> 94.3 MB = 1.005 x the algorithmic 93.8 MB), and no
  // global load or vmcnt wait left inside the step loop (profiles/r04_rollout_stage_* vs r04_rollout_nostage_*, NOTES.md)
  static int stage_env = -1;
  if (stage_env < 0) { const char* e = getenv("DITREE_ROLLOUT_STAGE"); stage_env = e ? atoi(e) : 1; }
  int stage = stage_env && (act_stride % 2 == 0) && (cs.actions_in % 2 == 0) && ((uintptr_t)actions % 16 == 0) ? 1 : 0;
  // work-group size: one wave per group spreads a small batch over many CUs (1 024 candidates: 16 CUs instead of 4); once
  // every SIMD has a wave anyway, four waves per group share one staged maze.  NOT two: 65 536 x 16 steps take 64.0 us in groups
  // of 128 threads against 50.5 (256) and 51.2 (64) -- profiles/r04_rollout_blocksize_probe.json; two-wave groups do not spread
  // evenly over the four SIMDs of a CU.  DITREE_ROLLOUT_BLK = 64 | 128 | 256 overrides.
  static int blk_env = -1;
  if (blk_env < 0) { const char* e = getenv("DITREE_ROLLOUT_BLK"); blk_env = e ? atoi(e) : 0; }
  const int blk = (blk_env == 64 || blk_env == 128 || blk_env == 256) ? blk_env : (B >= 16384 ? 256 : 64);
  static bool attr_done_dev[64] = {};                        // the attribute is per kernel AND per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool attr_done = dev >= 0 && dev < 64 && attr_done_dev[dev];
  if (!attr_done) {                                          // 256 threads x 256 B of staged actions + the maze exceed 64 KB
    const hipFuncAttribute at = hipFuncAttributeMaxDynamicSharedMemorySize;
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<1, true, true, false>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<1, true, true, true>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<1, false, true, false>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<1, false, true, true>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<2, true, true, false>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<2, true, true, true>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<2, false, true, false>, at, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)car_rollout_kernel<2, false, true, true>, at, 160 * 1024);
    if (dev >= 0 && dev < 64) attr_done_dev[dev] = true;
  }
  if (lds + (size_t)blk * 256 > 160 * 1024) stage = 0;        // a maze that leaves no room for the staged actions: per-step loads
  // lanes per candidate, measured on MI355X (profiles/r03_rollout_lanes.json): 8 192 candidates x 8 steps 31.6 -> 26.2 us with
  // two lanes (the batch fills a quarter of the SIMDs: the second lane's wave is free), 65 536 x 16 steps 73.2 -> 80.0 us
  // (every SIMD already has a wave; the duplicated dynamics cost more than the shorter chain saves).  DITREE_ROLLOUT_LANES
  // = 1 | 2 overrides.  (A wave-specialised form -- two waves per candidate set, one per half of the step's chain, two barriers
  // per step -- gave the same results and the same 56 us: profiles/NOTES.md.)
  static int lanes_env = -1;
  if (lanes_env < 0) { const char* e = getenv("DITREE_ROLLOUT_LANES"); lanes_env = e ? atoi(e) : 0; }
  // lockstep row stores pay with candidate-minor rows (whole 512-byte runs); with rows packed per candidate they cost 27 %
  // (dead lanes keep storing zero rows step by step: profiles/r04_rollout_layout_probe.json) -- chosen by the layout
  const bool lock = (states_out && states_stride.cand == 1) || (!states_out && actions_out && actout_stride.cand == 1);
  const int G = lanes_env == 1 ? 1 : (lanes_env == 2 ? 2 : (B <= 32768 ? 2 : 1));
#define CAR_ROLLOUT_LAUNCH(GG, PP, SS, SC)                                                                                      \
  hipLaunchKernelGGL((car_rollout_kernel<GG, PP, SS, SC>), dim3((GG * B + blk - 1) / blk), dim3(blk), lds + (SS ? (size_t)blk * 256 : 0), s, maze, \
                     rows, cols, state_io, actions, act_stride, status_io, B, A, gx, gy, states_out, states_stride, actions_out,  \
                     actout_stride, steps_out, steps_stride, chunks_run, prev_action_io, has_prev_io, idx, act_dense, budget, chunk_j, cs)
#define CAR_ROLLOUT_PICK(GG, SC)                                                                    \
  do {                                                                                              \
    if (lock) { if (stage) CAR_ROLLOUT_LAUNCH(GG, true, true, SC); else CAR_ROLLOUT_LAUNCH(GG, true, false, SC); }   \
    else { if (stage) CAR_ROLLOUT_LAUNCH(GG, false, true, SC); else CAR_ROLLOUT_LAUNCH(GG, false, false, SC); }      \
  } while (0)
  if (scenes) {
    if (G == 2) CAR_ROLLOUT_PICK(2, true); else CAR_ROLLOUT_PICK(1, true);
  } else {
    if (G == 2) CAR_ROLLOUT_PICK(2, false); else CAR_ROLLOUT_PICK(1, false);
  }
#undef CAR_ROLLOUT_PICK
#undef CAR_ROLLOUT_LAUNCH
}
void launch_car_rollout(const unsigned char* maze, int rows, int cols, double* state_io, const double* actions,
                        int64_t act_stride, int32_t* status_io, int B, int A, double gx, double gy,
                        double* states_out, int64_t states_stride, double* actions_out, int64_t actout_stride,
                        int32_t* steps_out, double* prev_action_io, uint8_t* has_prev_io, hipStream_t s) {
  launch_car_rollout_ex(maze, rows, cols, state_io, actions, act_stride, status_io, B, A, gx, gy, states_out,
                        ditree_strides{states_stride, 6, 1}, actions_out, ditree_strides{actout_stride, 2, 1}, steps_out, 1,
                        nullptr, prev_action_io, has_prev_io, nullptr, 1, s, nullptr, 0, ChunkStrides{0, 0, 0}, nullptr);
}

// ------------------------------------------------------------------------- lidar
// One workgroup per pose, one thread per ray (181 rays -> 192 threads).  The maze (f32
// {0,1}) is staged into LDS as bytes; visited cells are OR-ed into an LDS bitmap.
__global__ void __launch_bounds__(192)
lidar_scan_kernel(const double* __restrict__ poses, const float* __restrict__ maze, int rows, int cols,
                  double* __restrict__ dist, double* __restrict__ endpoints, uint8_t* __restrict__ hit,
                  uint8_t* __restrict__ visited) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int ncell = rows * cols;
  unsigned char* mz = lds;
  unsigned char* vis = lds + ((ncell + 15) & ~15);
  for (int i = threadIdx.x; i < ncell; i += blockDim.x) {
    mz[i] = (maze[i] == 1.0f) ? 1 : 0;
    vis[i] = 0;
  }
  __syncthreads();
  const int b = blockIdx.x;
  const int ray = threadIdx.x;
  const double x0 = poses[(size_t)b * 3 + 0], y0 = poses[(size_t)b * 3 + 1], yaw = poses[(size_t)b * 3 + 2];
  if (ray < DITREE_LIDAR_RAYS) {
    double d, ex, ey;
    bool h;
    lidar_ray(x0, y0, yaw, ray, mz, rows, cols, vis, &d, &ex, &ey, &h);
    dist[(size_t)b * DITREE_LIDAR_RAYS + ray] = d;
    endpoints[((size_t)b * DITREE_LIDAR_RAYS + ray) * 2 + 0] = ex;
    endpoints[((size_t)b * DITREE_LIDAR_RAYS + ray) * 2 + 1] = ey;
    hit[(size_t)b * DITREE_LIDAR_RAYS + ray] = h ? 1 : 0;
  }
  if (visited != nullptr) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) visited[(size_t)b * ncell + i] = vis[i];
  }
}
void launch_lidar_scan(const double* poses, int B, const float* maze, int rows, int cols, double* dist,
                       double* endpoints, uint8_t* hit, uint8_t* visited, hipStream_t s) {
  size_t n = ((size_t)rows * cols + 15) & ~(size_t)15;
  hipLaunchKernelGGL(lidar_scan_kernel, dim3(B), dim3(192), 2 * n, s, poses, maze, rows, cols, dist, endpoints,
                     hit, visited);
}

// ------------------------------------------------------------------------- plan following (online loop)
// run_scenarios_with_lidar_DiTree.py:470-506 (run_type < 4) as ONE launch: execute the plan's actions one env step
// at a time (propagate_action_sequence_env: step, goal test, collision test against the KNOWN maze), and every
// time the accumulated step time exceeds scan_time scan the TRUE maze from the pose (scan_and_update_maze,
// :112-127), write the ray end cells into the known / scanned mazes and test the planned path for a crossing
// (check_no_obstacles_in_path, :158-181).  One workgroup: thread 0 integrates, threads 0..180 cast the rays,
// all threads scan the path.  The three mazes live in LDS for the whole launch.
__global__ void __launch_bounds__(256)
follow_plan_kernel(double* __restrict__ state_io, const float* __restrict__ actions, int n_actions, int action_idx,
                   const float* __restrict__ path, int P, float* __restrict__ known, const float* __restrict__ truth,
                   float* __restrict__ scanned, unsigned char* __restrict__ known_codes, int rows, int cols, double gx,
                   double gy, double dt, double scan_time, double* __restrict__ executed, int32_t* __restrict__ result) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int ncell = rows * cols, pad = (ncell + 15) & ~15;
  unsigned char* kn = lds;                 // known maze codes
  unsigned char* tr = lds + pad;           // true maze: 1 = occupied
  unsigned char* sc = lds + 2 * pad;       // scanned maze codes
  unsigned char* vis = lds + 3 * pad;      // cells visited by the current scan
  unsigned char* dirty = lds + 4 * pad;    // cells of known / scanned written by this launch
  __shared__ double s[6];
  __shared__ int sh_event, sh_obstacle, sh_scan, sh_done;
  const int tid = threadIdx.x;
  for (int i = tid; i < ncell; i += blockDim.x) {
    kn[i] = maze_code(known[i]);
    tr[i] = truth[i] == 1.0f ? 1 : 0;
    sc[i] = maze_code(scanned[i]);
    vis[i] = 0;
    dirty[i] = 0;
  }
  if (tid < 6) s[tid] = state_io[tid];
  if (tid == 0) { sh_event = -1; sh_obstacle = 0x7fffffff; sh_scan = 0; sh_done = 0; }
  __syncthreads();
  double t_acc = 0.0;                      // thread 0 only
  int idx = action_idx, n_scans = 0;
  const float hf = (float)((double)rows / 2.0), wf = (float)((double)cols / 2.0);
  while (idx < n_actions) {
    if (tid == 0) {
      double st[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) st[k] = s[k];
      car_euler_step(st, (double)actions[2 * idx], (double)actions[2 * idx + 1]);
      const double ex = st[0] - gx, ey = st[1] - gy;
      const bool done = sqrt(fma(ey, ey, ex * ex)) < 0.5;                        // car_env.py:346-351
      if (car_collides(st[0], st[1], st[2], kn, rows, cols)) {                   // base_planner.py:306 -> done is None
        sh_event = 2;
      } else {
        double* eo = executed + (size_t)(idx - action_idx) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) { s[k] = st[k]; eo[k] = st[k]; }
        sh_done = done ? 1 : 0;
        t_acc += dt;
        sh_scan = t_acc > scan_time ? 1 : 0;
        if (sh_scan) t_acc = 0.0;
      }
    }
    __syncthreads();
    if (sh_event == 2) break;
    ++idx;
    if (sh_scan) {
      ++n_scans;
      // pose in fractional cell units (col, row), yaw in radians (:113-116)
      const double px = (s[0] + (double)cols / 2.0) / 1.0, py = ((double)rows / 2.0 - s[1]) / 1.0, yaw = s[2];
      double d, ex = 0.0, ey = 0.0;
      bool h;
      if (tid < DITREE_LIDAR_RAYS) lidar_ray(px, py, yaw, tid, tr, rows, cols, vis, &d, &ex, &ey, &h);
      __syncthreads();
      for (int i = tid; i < ncell; i += blockDim.x) {                            // scanned[visited] = 2 (:121)
        if (vis[i]) { sc[i] = 2; dirty[i] = 1; vis[i] = 0; }
      }
      __syncthreads();
      if (tid < DITREE_LIDAR_RAYS) {                                             // end cells -> occupied (:119-122)
        const double fx = floor(ex), fy = floor(ey);
        if (fx >= 0.0 && fx < (double)cols && fy >= 0.0 && fy < (double)rows) {
          const int c = (int)fy * cols + (int)fx;
          kn[c] = 1;
          sc[c] = 1;
          dirty[c] = 1;
        }
      }
      __syncthreads();
      int first = 0x7fffffff;                                                    // :158-181 in the path's float32
      for (int i = tid; i < P; i += blockDim.x) {
        const float row = (hf - path[2 * i + 1]) / 1.0f, col = (path[2 * i] + wf) / 1.0f;
        const float fr = floorf(row), fc = floorf(col);
        if (fr >= 0.0f && fr < (float)rows && fc >= 0.0f && fc < (float)cols && sc[(int)fr * cols + (int)fc] == 1) {
          first = i;
          break;
        }
      }
      if (first != 0x7fffffff) atomicMin(&sh_obstacle, first);
      __syncthreads();
    }
    if (sh_done) { if (tid == 0) sh_event = 1; break; }
    if (sh_obstacle != 0x7fffffff) { if (tid == 0) sh_event = 3; break; }
    __syncthreads();                       // thread 0 rewrites sh_scan / s in the next iteration
  }
  __syncthreads();
  for (int i = tid; i < ncell; i += blockDim.x) {
    if (dirty[i]) {
      known[i] = (float)kn[i];
      scanned[i] = (float)sc[i];
    }
    known_codes[i] = kn[i];
  }
  if (tid < 6) state_io[tid] = s[tid];
  if (tid == 0) {
    result[0] = sh_event < 0 ? 0 : sh_event;
    result[1] = idx;
    result[2] = sh_obstacle == 0x7fffffff ? -1 : sh_obstacle;
    result[3] = n_scans;
  }
}
void launch_follow_plan(double* state_io, const float* actions, int n_actions, int action_idx, const float* path, int P,
                        float* known, const float* truth, float* scanned, unsigned char* known_codes, int rows, int cols,
                        double gx, double gy, double dt, double scan_time, double* executed, int32_t* result,
                        hipStream_t s) {
  size_t pad = ((size_t)rows * cols + 15) & ~(size_t)15;
  hipLaunchKernelGGL(follow_plan_kernel, dim3(1), dim3(256), 5 * pad, s, state_io, actions, n_actions, action_idx, path,
                     P, known, truth, scanned, known_codes, rows, cols, gx, gy, dt, scan_time, executed, result);
}

// ------------------------------------------------------------------------- round bookkeeping
__global__ void round_begin_kernel(int32_t* status, int32_t* chunks_run, int32_t* chunk_steps, int B, int n_chunks) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  status[b] = DITREE_ST_OK;
  chunks_run[b] = 0;
  for (int j = 0; j < n_chunks; ++j) chunk_steps[(size_t)b * n_chunks + j] = 0;
}
void launch_round_begin(int32_t* status, int32_t* chunks_run, int32_t* chunk_steps, int B, int n_chunks,
                        hipStream_t s) {
  hipLaunchKernelGGL(round_begin_kernel, dim3((B + 255) / 256), dim3(256), 0, s, status, chunks_run, chunk_steps, B,
                     n_chunks);
}

// ------------------------------------------------------------------------- alive compaction
// idx_out[0..n) = candidates whose status is still DITREE_ST_OK, in candidate order; *count = n.
// One workgroup, ordered prefix sum (the denoiser then runs on the n alive rows only).
__global__ void __launch_bounds__(1024) compact_alive_kernel(const int32_t* __restrict__ status, int B,
                                                             int32_t* __restrict__ idx_out, int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ budget, int next_chunk) {
  __shared__ int s_wave_sum[16];
  const int tid = threadIdx.x;
  int base = 0;
  for (int start = 0; start < B; start += blockDim.x) {
    const int b = start + tid;
    const int alive = (b < B && status[b] == DITREE_ST_OK && (budget == nullptr || next_chunk < budget[b])) ? 1 : 0;
    int v = alive;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int o = __shfl_up(v, d);
      if ((tid & 63) >= d) v += o;
    }
    if ((tid & 63) == 63) s_wave_sum[tid >> 6] = v;
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      if (w < (tid >> 6)) woff += s_wave_sum[w];
      total += s_wave_sum[w];
    }
    if (alive) idx_out[base + woff + v - 1] = b;
    base += total;
    __syncthreads();
  }
  if (tid == 0) *count = base;
}
void launch_compact_alive(const int32_t* status, int B, int32_t* idx_out, int32_t* count, hipStream_t s,
                          const int32_t* budget, int next_chunk) {
  hipLaunchKernelGGL(compact_alive_kernel, dim3(1), dim3(1024), 0, s, status, B, idx_out, count, budget, next_chunk);
}

// Ready list of a pool-scheduled early-exit round: the candidates that still have a chunk to run (status OK, chunks_run < their
// budget), ordered by (chunks finished, candidate) -- the ones furthest behind first, so nobody starves at the end of the
// list -- with, per entry, the row of the (B * n_chunks, ...) noise view its next denoiser call reads.  One workgroup; one
// ordered prefix-sum pass per chunk index (n_chunks <= 64, B <= a few 10 000: microseconds).
__global__ void __launch_bounds__(1024) compact_ready_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ chunks_run,
                                                             const int32_t* __restrict__ budget, int n_chunks, int B,
                                                             int32_t* __restrict__ idx_out, int32_t* __restrict__ nrow_out,
                                                             int32_t* __restrict__ count) {
  __shared__ int s_wave_sum[16];
  const int tid = threadIdx.x;
  int base = 0;
  for (int j = 0; j < n_chunks; ++j) {
    for (int start = 0; start < B; start += blockDim.x) {
      const int b = start + tid;
      const int rdy = (b < B && status[b] == DITREE_ST_OK && chunks_run[b] == j && j < (budget ? budget[b] : n_chunks)) ? 1 : 0;
      int v = rdy;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(v, d);
        if ((tid & 63) >= d) v += o;
      }
      if ((tid & 63) == 63) s_wave_sum[tid >> 6] = v;
      __syncthreads();
      int woff = 0, total = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
        if (w < (tid >> 6)) woff += s_wave_sum[w];
        total += s_wave_sum[w];
      }
      if (rdy) {
        idx_out[base + woff + v - 1] = b;
        nrow_out[base + woff + v - 1] = b * n_chunks + j;
      }
      base += total;
      __syncthreads();
    }
  }
  if (tid == 0) *count = base;
}
void launch_compact_ready(const int32_t* status, const int32_t* chunks_run, const int32_t* budget, int n_chunks, int B,
                          int32_t* idx_out, int32_t* nrow_out, int32_t* count, hipStream_t s) {
  hipLaunchKernelGGL(compact_ready_kernel, dim3(1), dim3(1024), 0, s, status, chunks_run, budget, n_chunks, B, idx_out, nrow_out, count);
}

// planners/RRT.py:149-152 for a round: candidate b is visit number num_visit[parent] + (earlier candidates of the round with
// the same parent) of its parent; its edge runs schedule[clip(visit)] chunks.  B^2 / 2 parent compares out of L2 (B <= 8192).
struct ScheduleArg { int n; int chunks[16]; };
__global__ void __launch_bounds__(256) chunk_budget_kernel(const int32_t* __restrict__ parent, int B,
                                                           const int32_t* __restrict__ num_visit, ScheduleArg sc,
                                                           int32_t* __restrict__ budget) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int p = parent[b];
  int k = num_visit[p];
  for (int q = 0; q < b; ++q) k += (parent[q] == p) ? 1 : 0;
  k = k < 0 ? 0 : (k > sc.n - 1 ? sc.n - 1 : k);
  budget[b] = sc.chunks[k];
}
void launch_chunk_budget(const int32_t* parent, int B, const int32_t* num_visit, const int32_t* chunks, int n,
                         int32_t* budget, hipStream_t s) {
  ScheduleArg sc{};
  sc.n = n;
  for (int i = 0; i < n && i < 16; ++i) sc.chunks[i] = chunks[i];
  hipLaunchKernelGGL(chunk_budget_kernel, dim3((B + 255) / 256), dim3(256), 0, s, parent, B, num_visit, sc, budget);
}

// rows of a strided f32 matrix gathered by candidate index (the chunk's noise for the alive candidates)
__global__ void gather_rows_f32_kernel(const float* __restrict__ src, int64_t src_stride, const int32_t* __restrict__ idx,
                                       float* __restrict__ dst, int row_floats, int n) {
  const int r = blockIdx.x;
  if (r >= n) return;
  const float* s = src + (size_t)idx[r] * src_stride;
  float* d = dst + (size_t)r * row_floats;
  for (int k = threadIdx.x; k < row_floats; k += blockDim.x) d[k] = s[k];
}
void launch_gather_rows_f32(const float* src, int64_t src_stride, const int32_t* idx, float* dst, int row_floats, int n,
                            hipStream_t s) {
  hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(n), dim3(128), 0, s, src, src_stride, idx, dst, row_floats, n);
}

// ------------------------------------------------------------------------- obstacle ahead
// planners/RRT.py:61-81: samples = linspace(0, 1.5, 30)[:, None] @ [[cos(-psi), sin(-psi)]] + (col, row) with
// (row, col) = cell_xy_to_rowcol(xy, floor_enable=False); astype('int') truncates toward zero; clip; any.
__device__ __forceinline__ bool obstacle_ahead_dev(double x, double y, double psi, const unsigned char* mz, int H, int W,
                                                   const AheadArg& ts) {
  const double row = ((double)H / 2.0 - y) / 1.0, col = (x + (double)W / 2.0) / 1.0;     // car_env.py:196-201
  double c, sn;
  sincos(-psi, &sn, &c);
  bool any = false;
#pragma unroll 1
  for (int i = 0; i < 30; ++i) {
    const double px = ts.t[i] * c + col, py = ts.t[i] * sn + row;
    // numpy's astype(int) of NaN / out-of-range is INT64_MIN -> clipped to 0
    long long qx = (px == px && fabs(px) < 9.0e18) ? (long long)px : (long long)-1;
    long long qy = (py == py && fabs(py) < 9.0e18) ? (long long)py : (long long)-1;
    const int ix = qx < 0 ? 0 : (qx > W - 1 ? W - 1 : (int)qx);
    const int iy = qy < 0 ? 0 : (qy > H - 1 ? H - 1 : (int)qy);
    any |= mz[iy * W + ix] != 0;
  }
  return any;
}
__global__ void obstacle_ahead_kernel(const unsigned char* __restrict__ maze, int rows, int cols,
                                      const double* __restrict__ state, int stride, int B, AheadArg ts,
                                      uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  stage_maze(lds, maze, rows * cols);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* s = state + (size_t)b * stride;
  out[b] = obstacle_ahead_dev(s[0], s[1], s[2], lds, rows, cols, ts) ? 1 : 0;
}
void launch_obstacle_ahead(const unsigned char* maze, int rows, int cols, const double* state, int stride, int B,
                           const AheadArg& ts, uint8_t* out, hipStream_t s) {
  size_t lds = ((size_t)rows * cols + 15) & ~(size_t)15;
  hipLaunchKernelGGL(obstacle_ahead_kernel, dim3((B + 255) / 256), dim3(256), lds, s, maze, rows, cols, state, stride, B,
                     ts, out);
}

// ------------------------------------------------------------------------- fallback selection
// planners/RRT.py:233-254 over nodes 1..n-1.  One workgroup; every thread scans a strided subset and keeps
// (key, index) with first-occurrence ties, then a block reduction.
__global__ void __launch_bounds__(1024) fallback_select_kernel(ditree_tree t, int n, double gx, double gy,
                                                               const double* __restrict__ path, int P,
                                                               int32_t* __restrict__ out_node) {
  __shared__ double s_key[1024];
  __shared__ int s_idx[1024];
  const int tid = threadIdx.x;
  // minimise `key`: cost for the goal-distance rule, -progress for the along-path rule
  double best = __builtin_huge_val();
  int bidx = 0x7fffffff;
  int free_seen = 0;
  for (int i = 1 + tid; i < n; i += blockDim.x) {
    const double x = t.xy[(size_t)i * 2], y = t.xy[(size_t)i * 2 + 1];
    const bool obs = t.obstacle_ahead != nullptr && t.obstacle_ahead[i] != 0;
    free_seen |= !obs;
    double key;
    if (path == nullptr) {
      const double dx = x - gx, dy = y - gy;
      key = sqrt(fma(dy, dy, dx * dx)) + 10e3 * (obs ? 1.0 : 0.0);      // np.linalg.norm (1-D) + 10e3 * flag
    } else {
      int prog = -1;
      if (!obs) {
        double bd = __builtin_huge_val();
        for (int k = 0; k < P; ++k) {
          const double dx = x - path[2 * k], dy = y - path[2 * k + 1];
          const double d = sqrt(dx * dx + dy * dy);                      // np.linalg.norm(axis=1): no fused dot
          if (d < bd) { bd = d; prog = k; }
        }
      }
      key = -(double)prog;
    }
    if (key < best) { best = key; bidx = i; }
  }
  s_key[tid] = best;
  s_idx[tid] = bidx;
  const int any_free = __syncthreads_or(free_seen);
  for (int off = blockDim.x >> 1; off > 0; off >>= 1) {
    if (tid < off) {
      const double ok = s_key[tid + off];
      const int oi = s_idx[tid + off];
      if (ok < s_key[tid] || (ok == s_key[tid] && oi < s_idx[tid])) { s_key[tid] = ok; s_idx[tid] = oi; }
    }
    __syncthreads();
  }
  // RRT.py:227-232: np.all(has_obstacle_ahead) (true for an empty list) -> no plan
  if (tid == 0) *out_node = (!any_free || s_idx[0] == 0x7fffffff) ? -1 : s_idx[0];
}
void launch_fallback_select(const ditree_tree& t, int n_nodes, double gx, double gy, const double* path_dev, int P,
                            int32_t* out_node, hipStream_t s) {
  hipLaunchKernelGGL(fallback_select_kernel, dim3(1), dim3(1024), 0, s, t, n_nodes, gx, gy, path_dev, P, out_node);
}

// ------------------------------------------------------------------------- accept + commit
// Which trees an accept works on (ditree_internal.h TreeSet): a forest, or a single tree as the forest of one tree.  A tree's
// counter row: [0] n_nodes [1] goal node [2] env.done latched [3] chunk iterations [4] candidates [5] sticky triggered
// [6] capacity overflow [7] phantom candidate (scratch).
__device__ __forceinline__ int32_t* tree_counters(const TreeSet& ts, int tr) { return ts.counters + (size_t)tr * 8; }
// The slice of the work-group's tree, blockIdx.x: its counter row, its candidates [lo, lo + n) of the round, its node slots
// [node_base, node_base + C), and its stats row -- formed in the BOUND instantiations alone, NULL in the others.
struct TreeSlice {
  int32_t* counters;
  int32_t* stats;
  int lo, n, node_base;
};
// false: the tree has no candidate in this round -- the work-group returns before any barrier and leaves the tree and its
// stats row untouched (as an empty round does).
template <bool BOUND>
__device__ __forceinline__ bool tree_slice(const TreeSet& ts, const ditree_round& r, int32_t* __restrict__ stats_rows,
                                           TreeSlice& sl) {
  const int tr = blockIdx.x;
  sl.lo = ts.off ? ts.off[tr] : 0;
  sl.n = ts.off ? ts.off[tr + 1] - sl.lo : r.B;
  if (sl.n <= 0) return false;
  sl.counters = tree_counters(ts, tr);
  sl.node_base = tr * ts.C;
  sl.stats = nullptr;
  if constexpr (BOUND) sl.stats = stats_rows + (size_t)tr * 4;
  return true;
}

// Phase 1 (one work-group per tree; trees run in parallel): the reference's sequential accept order (RRT.py:179-217) as a
// scan over the tree's candidates.  Node ids, the goal node and the phantom are written in the global numbering (node_base +
// local slot, lo + local candidate).  Every scanned candidate counts, adds its chunks and visits its parent.
//   first    (ditree_accept): the scan ends at the round's first goal row, or at the phantom row of the sticky-done emulation;
//            the rows behind it get no node.
//   best     (ditree_accept_best): every candidate in index order, nothing cut at a goal and no phantom.  The goal node is
//            chosen after the commit (accept_pick_kernel), so counters[1], [2] and [5] are not touched here.
//   bounded  (ditree_accept_bounded): as best, and on entry node_id[b] holds f = cost + h of candidate b (accept_cost_kernel); a
//            candidate that did not collide gets a slot only if f < U, U the tree's bound as of the round's start, else it is
//            pruned: node id -1, counted in stats[1] (since the tree's reset) and stats[3] (this round).  The overflow flag is
//            raised by unpruned rows alone, because only they are ranked.
//   SPARSE   (ditree_accept_sparse, best or bounded; include/ditree.h "sparse tree"): on entry sp->cand holds c and the cell of
//            every candidate and sp->scratch the smallest (c, candidate) of every cell that has one (sparse_cost_kernel).  Behind
//            the mode's own tests a candidate gets a slot only if it has no cell, reached the goal, or WON its cell: it is the
//            cell's contender and the cell holds no node or a dearer one.  The rest is dominated: node id -1, stats[0] and [3].
//            Once the ids are out, a winner with a slot becomes its cell's table entry and active, the node it displaced inactive
//            (stats[1]; a new cell: stats[2]); every other new node is inactive.  Only the contender of a cell reads or writes the
//            cell's table entry, so the order of the threads does not matter; the scratch entries go back to all ones behind the
//            last read.
struct SparseTree {                                    // the sparse descriptor's rows of the work-group's tree
  unsigned long long* table;
  unsigned long long* scratch;
  int32_t* stats;
};
__device__ __forceinline__ unsigned long long sparse_key(int c, int id) {
  return ((unsigned long long)(unsigned)c << 32) | (unsigned)id;
}
template <AcceptMode MODE, bool SPARSE = false>
__device__ __forceinline__ void accept_scan_tree(const TreeSlice& sl, int cap, int32_t* __restrict__ num_visit,
                                                 const ditree_round& r, int emulate_sticky, const int32_t* __restrict__ cost,
                                                 const SparseTree* st = nullptr, const int32_t* __restrict__ cand = nullptr,
                                                 uint8_t* __restrict__ active = nullptr) {
  __shared__ int s_first_goal, s_first_gac, s_iters, s_pruned;
  __shared__ int s_sparse[3];                          // SPARSE: dominated, retired, new cells
  __shared__ int s_wave_sum[16];
  int32_t* __restrict__ counters = sl.counters;
  const int32_t* __restrict__ status = r.status + sl.lo;
  const int32_t* __restrict__ chunks_run = r.chunks_run + sl.lo;
  const int32_t* __restrict__ parent = r.parent + sl.lo;
  int32_t* __restrict__ node_id = r.node_id + sl.lo;
  const int B = sl.n, tid = threadIdx.x;
  if (tid == 0) {
    s_iters = 0;
    if constexpr (MODE == AcceptMode::first) { s_first_goal = 0x7fffffff; s_first_gac = 0x7fffffff; }
    if constexpr (MODE == AcceptMode::bounded) s_pruned = 0;
    if constexpr (SPARSE) { s_sparse[0] = 0; s_sparse[1] = 0; s_sparse[2] = 0; }
  }
  __syncthreads();
  int last = B - 1, phantom = -1, goal_cand = -1, U = 0x7fffffff;
  bool latch_out = false;
  if constexpr (MODE == AcceptMode::first) {
    for (int b = tid; b < B; b += blockDim.x) {
      int st = status[b];
      if ((st & 0xff) == DITREE_ST_GOAL) atomicMin(&s_first_goal, b);
      if (emulate_sticky && (st & 0xff) == DITREE_ST_COLLIDED && (st & DITREE_ST_FLAG_GOAL_AT_COLLISION))
        atomicMin(&s_first_gac, b);
    }
    __syncthreads();
    const int g = s_first_goal, c = s_first_gac;
    const bool latched_in = emulate_sticky && counters[2] != 0;
    latch_out = latched_in;
    if (latched_in) {
      phantom = 0; last = 0; goal_cand = 0;
    } else if (c != 0x7fffffff && (g == 0x7fffffff || g > c)) {
      if (c + 1 < B) { phantom = c + 1; last = c + 1; goal_cand = c + 1; latch_out = true; }
      else { latch_out = true; }
    } else if (g != 0x7fffffff) {
      last = g; goal_cand = g;
    }
  }
  if constexpr (MODE == AcceptMode::bounded) U = bound_of(counters, cost);
  const int n0 = counters[0];
  // ordered prefix sum of accepted flags over candidates 0..last, 1024 at a time
  int base = 0;
  for (int start = 0; start <= last; start += blockDim.x) {
    const int b = start + tid;
    int acc = 0, it = 0;
    bool won = false;                                  // SPARSE: b won its cell
    if (b <= last) {
      const bool ph = MODE == AcceptMode::first && b == phantom;
      acc = ph ? 1 : ((status[b] & 0xff) != DITREE_ST_COLLIDED);
      if constexpr (MODE == AcceptMode::bounded) {
        if (acc && !(node_id[b] < U)) { acc = 0; atomicAdd(&s_pruned, 1); }
      }
      if constexpr (SPARSE) {
        const int cell = cand[2 * (sl.lo + b) + 1];
        if (acc && cell >= 0) {
          const int c = cand[2 * (sl.lo + b)];
          if (st->scratch[cell] == sparse_key(c, sl.lo + b)) {
            const unsigned long long rep = st->table[cell];
            won = rep == ~0ull || c < (int)(rep >> 32);
          }
          if (!won && (status[b] & 0xff) != DITREE_ST_GOAL) { acc = 0; atomicAdd(&s_sparse[0], 1); }
        }
      }
      it = ph ? 1 : chunks_run[b];
      atomicAdd(&num_visit[parent[b]], 1);
    }
    // wave inclusive scan
    int v = acc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int o = __shfl_up(v, d);
      if ((tid & 63) >= d) v += o;
    }
    int itw = it;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) itw += __shfl_xor(itw, m);
    if ((tid & 63) == 63) s_wave_sum[tid >> 6] = v;
    if ((tid & 63) == 0) atomicAdd(&s_iters, itw);
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < (tid >> 6); ++w) woff += s_wave_sum[w];
    int chunk_total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) chunk_total += s_wave_sum[w];
    if (b <= last) {
      int id = acc ? (n0 + base + woff + v - acc) : -1;   // n0 + exclusive rank
      if (id >= cap) id = -1;
      node_id[b] = id < 0 ? -1 : sl.node_base + id;
      if constexpr (SPARSE) {
        if (id >= 0) {
          const int gid = sl.node_base + id;
          active[gid] = won ? 1 : 0;
          if (won) {
            const int cell = cand[2 * (sl.lo + b) + 1];
            const unsigned long long rep = st->table[cell];
            st->table[cell] = sparse_key(cand[2 * (sl.lo + b)], gid);
            if (rep != ~0ull) { active[(int)(rep & 0xffffffffull)] = 0; atomicAdd(&s_sparse[1], 1); }
            else atomicAdd(&s_sparse[2], 1);
          }
        }
      }
    }
    base += chunk_total;
    __syncthreads();
  }
  if constexpr (SPARSE) {                              // every read of the contenders is behind the loop's last barrier
    for (int b = tid; b < B; b += blockDim.x) {
      const int cell = cand[2 * (sl.lo + b) + 1];
      if (cell >= 0) st->scratch[cell] = ~0ull;
    }
  }
  if constexpr (MODE == AcceptMode::first) {
    for (int b = last + 1 + tid; b < B; b += blockDim.x) node_id[b] = -1;
    __syncthreads();
  }
  if (tid == 0) {
    int n1 = n0 + base;
    if (n1 > cap) { n1 = cap; counters[6] = 1; }
    counters[0] = n1;
    if constexpr (MODE == AcceptMode::first) {
      if (goal_cand >= 0) counters[1] = node_id[goal_cand];
      counters[2] = (emulate_sticky && latch_out && phantom < 0) ? 1 : ((phantom >= 0) ? 1 : counters[2]);
      if (phantom >= 0) counters[5] = 1;
    }
    counters[3] += s_iters;
    counters[4] += last + 1;
    counters[7] = phantom < 0 ? -1 : sl.lo + phantom;
    if constexpr (MODE == AcceptMode::bounded) { sl.stats[1] += s_pruned; sl.stats[3] = s_pruned; }
    if constexpr (SPARSE) {
      st->stats[0] += s_sparse[0];
      st->stats[1] += s_sparse[1];
      st->stats[2] += s_sparse[2];
      st->stats[3] = s_sparse[0];
    }
  }
}
template <AcceptMode MODE>
__global__ void __launch_bounds__(1024)
accept_scan_kernel(ditree_tree t, ditree_round r, TreeSet ts, int emulate_sticky, BoundArg bd) {
  TreeSlice sl;
  if (!tree_slice<MODE == AcceptMode::bounded>(ts, r, bd.stats, sl)) return;
  accept_scan_tree<MODE>(sl, ts.C, t.num_visit, r, emulate_sticky, bd.cost);
}
// The pick of ditree_accept_best, after the commit: among the tree's goal candidates that got a node slot, the smallest
// (cost[node], candidate index); it replaces the incumbent counters[1] only when there is none or its cost is strictly smaller.
// Candidate indices are compared within the tree: the offset lo is common to all of them.
// BOUND (ditree_accept_bounded): thread 0, which wrote the incumbent, also writes the bound the next round will use and whether
// any node can still be open -- key[root] is the smallest key a tree can hold below its root, so key[root] >= U closes the
// whole tree.  stats: [0] U, [1] candidates pruned since the reset, [2] exhausted, [3] candidates pruned this round.
template <bool BOUND>
__global__ void __launch_bounds__(1024)
accept_pick_kernel(ditree_round r, TreeSet ts, const int32_t* __restrict__ cost, BoundArg bd) {
  TreeSlice sl;
  if (!tree_slice<BOUND>(ts, r, bd.stats, sl)) return;
  __shared__ unsigned long long s_best;
  const int32_t* __restrict__ status = r.status + sl.lo;
  const int32_t* __restrict__ node_id = r.node_id + sl.lo;
  const int tid = threadIdx.x;
  if (tid == 0) s_best = ~0ull;
  __syncthreads();
  for (int b = tid; b < sl.n; b += blockDim.x) {
    const int id = node_id[b];
    if ((status[b] & 0xff) == DITREE_ST_GOAL && id >= 0)  // a collided candidate's goal-at-collision flag is not a goal
      atomicMin(&s_best, ((unsigned long long)(unsigned)cost[id] << 32) | (unsigned)b);
  }
  __syncthreads();
  if (tid == 0) {
    if (s_best != ~0ull) {
      const int c = (int)(s_best >> 32), b = (int)(s_best & 0xffffffffull);
      const int inc = sl.counters[1];
      if (inc < 0 || c < cost[inc]) sl.counters[1] = node_id[b];
    }
    if constexpr (BOUND) {
      const int U = bound_of(sl.counters, cost);
      sl.stats[0] = U;
      sl.stats[2] = bd.key[sl.node_base] >= U ? 1 : 0;
    }
  }
}
// The pre-pass of a bounded accept, one wave per candidate: a goal reached in mid-chunk leaves all-zero rows behind it, so what
// a candidate's node would cost is known only after the zero-row filter -- the commit kernel's ballot over the rows of the
// chunks that ran.  f = cost[parent] + kept edge states + 1 + h(end xy) goes to node_id[b], where the scan reads it before it
// writes the id.  The candidate's tree is its parent's (parent / C), with that tree's counter row and goal.
// A tree without an incumbent prunes nothing: its candidates skip the count.
__global__ void __launch_bounds__(64)
accept_cost_kernel(ditree_tree t, ditree_round r, TreeSet ts, BoundArg bd) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int par = r.parent[b];
  const int tr = par / ts.C;
  const int U = bound_of(tree_counters(ts, tr), bd.cost);
  if (U == 0x7fffffff || (r.status[b] & 0xff) == DITREE_ST_COLLIDED) {
    if (lane == 0) r.node_id[b] = 0;
    return;
  }
  const int A = t.A, S = t.state_dim;
  const double* cs = r.states + (size_t)b * t.n_chunks * (A + 1) * S;
  const int rows_s = r.chunks_run[b] * (A + 1);
  int ns = 0;
  for (int row = 0; row < rows_s; ++row) {
    const double v = lane < S ? cs[(size_t)row * S + lane] : 0.0;
    if (__ballot(v != 0.0) != 0ull) ++ns;
  }
  if (lane == 0) {
    const double ex = r.end_state[(size_t)b * S], ey = r.end_state[(size_t)b * S + 1];
    r.node_id[b] = bd.cost[par] + ns + 1 + bound_h(ex, ey, bd.goal_xy[2 * tr], bd.goal_xy[2 * tr + 1], bd.goal_radius, bd.reach);
  }
}
// ---- sparse tree (include/ditree.h "sparse tree")
// The cell of a state in tree tr, -1 without one.  Each operation is one rounded f64 operation (this unit does not contract), the
// clamps are taken on the floored doubles, so a numpy restatement of the same expression gives the same cell bit for bit.  An
// index past the table's stride cannot come out of a validated descriptor; it is refused here all the same.
__device__ __forceinline__ int sparse_cell(const SparseArg& sp, int tr, double x, double y, double psi) {
  if (!isfinite(x) || !isfinite(y) || !isfinite(psi)) return -1;
  const double W = sp.extent[2 * tr], L = sp.extent[2 * tr + 1];
  const int nx = sp.dims[2 * tr], ny = sp.dims[2 * tr + 1];
  const double two_pi = 2.0 * 3.14159265358979323846;
  double fx = floor((x + W / 2.0) / sp.cell), fy = floor((y + L / 2.0) / sp.cell);
  fx = fx < 0.0 ? 0.0 : (fx > (double)(nx - 1) ? (double)(nx - 1) : fx);
  fy = fy < 0.0 ? 0.0 : (fy > (double)(ny - 1) ? (double)(ny - 1) : fy);
  const double a = psi - two_pi * floor(psi / two_pi);
  double fh = floor(a / sp.w);
  fh = fh < 0.0 ? 0.0 : (fh > (double)(sp.nh - 1) ? (double)(sp.nh - 1) : fh);
  const long long cell = ((long long)fy * nx + (long long)fx) * sp.nh + (long long)fh;
  return cell < (long long)sp.stride ? (int)cell : -1;
}
// the table words as the type the 64-bit atomicMin takes
__device__ __forceinline__ unsigned long long* sparse_words(uint64_t* p, int tr, int stride) {
  return reinterpret_cast<unsigned long long*>(p) + (size_t)tr * stride;
}
__device__ __forceinline__ SparseTree sparse_tree(const SparseArg& sp, int tr) {
  return SparseTree{sparse_words(sp.table, tr, sp.stride), sparse_words(sp.scratch, tr, sp.stride), sp.stats + (size_t)tr * 4};
}
// The pre-pass of a sparse accept, one wave per candidate (accept_cost_kernel's shape and row count): c and the cell of the
// candidate go to sp.cand, BOUND: f to node_id[b] as accept_cost_kernel leaves it.  A candidate that can still get a node by
// winning its cell -- not collided, a cell, BOUND: f < U -- enters the contest of that cell: one 64-bit atomicMin of (c, b), so the
// contender does not depend on the order of the waves.
template <bool BOUND>
__global__ void __launch_bounds__(64)
sparse_cost_kernel(ditree_tree t, ditree_round r, TreeSet ts, const int32_t* __restrict__ cost, BoundArg bd, SparseArg sp) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int par = r.parent[b];
  const int tr = par / ts.C;
  if ((r.status[b] & 0xff) == DITREE_ST_COLLIDED) {
    if (lane == 0) {
      if constexpr (BOUND) r.node_id[b] = 0;
      sp.cand[2 * b] = 0;
      sp.cand[2 * b + 1] = -1;
    }
    return;
  }
  const int A = t.A, S = t.state_dim;
  const double* cs = r.states + (size_t)b * t.n_chunks * (A + 1) * S;
  const int rows_s = r.chunks_run[b] * (A + 1);
  int ns = 0;
  for (int row = 0; row < rows_s; ++row) {
    const double v = lane < S ? cs[(size_t)row * S + lane] : 0.0;
    if (__ballot(v != 0.0) != 0ull) ++ns;
  }
  if (lane == 0) {
    const double* e = r.end_state + (size_t)b * S;
    const int c = cost[par] + ns + 1;
    bool in = true;
    if constexpr (BOUND) {
      const int U = bound_of(tree_counters(ts, tr), bd.cost);
      const int f = U == 0x7fffffff ? 0 : c + bound_h(e[0], e[1], bd.goal_xy[2 * tr], bd.goal_xy[2 * tr + 1], bd.goal_radius, bd.reach);
      r.node_id[b] = f;
      in = f < U;
    }
    const int cell = sparse_cell(sp, tr, e[0], e[1], e[2]);
    sp.cand[2 * b] = c;
    sp.cand[2 * b + 1] = cell;
    if (in && cell >= 0) atomicMin(sparse_words(sp.scratch, tr, sp.stride) + cell, sparse_key(c, b));
  }
}
template <AcceptMode MODE>
__global__ void __launch_bounds__(1024)
accept_scan_sparse_kernel(ditree_tree t, ditree_round r, TreeSet ts, BoundArg bd, const int32_t* __restrict__ cost, SparseArg sp) {
  TreeSlice sl;
  if (!tree_slice<MODE == AcceptMode::bounded>(ts, r, bd.stats, sl)) return;
  const SparseTree st = sparse_tree(sp, blockIdx.x);
  accept_scan_tree<MODE, true>(sl, ts.C, t.num_visit, r, 0, cost, &st, sp.cand, sp.active);
}
// ditree_sparse_rebuild, three launches over trees [first, first + n) (blockIdx.y): the rows of the table and the scratch to all
// ones and the stats row to zero; the minimum of (cost, slot) over the nodes of every cell; then a node is active iff it is its
// cell's minimum, counted per wave into stats[2].
__global__ void __launch_bounds__(256) sparse_clear_kernel(SparseArg sp, int first) {
  const int tr = first + blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sp.stride) return;
  sp.table[(size_t)tr * sp.stride + i] = ~0ull;
  sp.scratch[(size_t)tr * sp.stride + i] = ~0ull;
  if (i < 4) sp.stats[(size_t)tr * 4 + i] = 0;
}
template <bool FLAG>
__global__ void __launch_bounds__(256)
sparse_nodes_kernel(ditree_tree t, TreeSet ts, const int32_t* __restrict__ cost, SparseArg sp, int first) {
  const int tr = first + blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  int n = tree_counters(ts, tr)[0];
  n = n > ts.C ? ts.C : n;
  bool act = false;
  if (i < n) {
    const int id = tr * ts.C + i;
    const double* s = t.state + (size_t)id * t.state_dim;
    const int cell = sparse_cell(sp, tr, s[0], s[1], s[2]);
    if (cell >= 0) {
      unsigned long long* slot = sparse_words(sp.table, tr, sp.stride) + cell;
      if constexpr (FLAG) act = *slot == sparse_key(cost[id], id);
      else atomicMin(slot, sparse_key(cost[id], id));
    }
    if constexpr (FLAG) sp.active[id] = act ? 1 : 0;
  }
  if constexpr (FLAG) {
    const int cnt = __popcll(__ballot(act));
    if ((threadIdx.x & 63) == 0 && cnt > 0) atomicAdd(&sp.stats[(size_t)tr * 4 + 2], cnt);
  }
}
void launch_sparse_rebuild(const ditree_tree& t, const TreeSet& ts, const int32_t* cost, const SparseArg& sp, int first, int n,
                           hipStream_t s) {
  hipLaunchKernelGGL(sparse_clear_kernel, dim3((sp.stride + 255) / 256, n), dim3(256), 0, s, sp, first);
  const dim3 nodes((ts.C + 255) / 256, n);
  hipLaunchKernelGGL(sparse_nodes_kernel<false>, nodes, dim3(256), 0, s, t, ts, cost, sp, first);
  hipLaunchKernelGGL(sparse_nodes_kernel<true>, nodes, dim3(256), 0, s, t, ts, cost, sp, first);
}

// key[n] = cost[n] + h(xy[n]) for nodes [first, first + n) (ditree_bound_keys: the roots); node n belongs to tree n / C, C as
// in a TreeSet.
__global__ void bound_keys_kernel(const double2* __restrict__ xy, int first, int n, int C, BoundArg bd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = first + i, tr = k / C;
  const double2 p = xy[k];
  bd.key[k] = bd.cost[k] + bound_h(p.x, p.y, bd.goal_xy[2 * tr], bd.goal_xy[2 * tr + 1], bd.goal_radius, bd.reach);
}

// Phase 2: one wave per candidate copies the accepted edge into its node slot, dropping
// all-zero rows (RRT.py:196-199).  State / action width S / D at run time (car 6 / 2, ant 29 / 8; S, D <= 64: a lane per
// component, the zero-row test is one ballot).
// The node's tree is id / C (0 for a single tree, whose ids stay below its capacity): the phantom candidate is the one in that
// tree's counter row.
// cost != NULL (ditree_accept_best): cost[id] = rows of the path to the node = cost[parent] + kept edge states + 1; the
// parent is a node of an earlier round, so its cost is final.
// KEY (ditree_accept_bounded): key[id] = cost[id] + h(the node's xy, its tree's goal), written where cost is.  KEY = false
// does not read the trailing argument.
template <bool KEY>
__global__ void __launch_bounds__(64)
accept_commit_kernel(ditree_tree t, ditree_round r, const unsigned char* __restrict__ maze, int rows, int cols,
                     AheadArg ahead, TreeSet ts, int32_t* __restrict__ cost, BoundArg bd) {
  const int b = blockIdx.x;
  const int id = r.node_id[b];
  if (id < 0) return;
  const int lane = threadIdx.x;
  const int A = t.A, nC = t.n_chunks, S = t.state_dim, D = t.action_dim;
  const int tr = id / ts.C;
  const int phantom = tree_counters(ts, tr)[7];
  const int par = r.parent[b];
  const size_t es_cap = (size_t)nC * (A + 1), ea_cap = (size_t)nC * A;
  double* es = t.edge_states + (size_t)id * es_cap * S;
  double* ea = t.edge_actions + (size_t)id * ea_cap * D;
  const double* cs = r.states + (size_t)b * es_cap * S;
  const double* ca = r.actions + (size_t)b * ea_cap * D;
  int ns = 0, na = 0;
  double endv = 0.0;                                   // lane k < S: component k of the node's state
  // sharded rounds: the trajectories of candidates another rank expanded are not here -- their nodes get state, parent
  // and last action from the exchanged record, the edge rows stay with the owner (edge_owner)
  const bool own = r.shard == 0 || (b >= r.own_lo && b < r.own_lo + r.own_n);
  int owner = -1;
  if (b == phantom) {
    // frozen env step (car_env.py:254): the edge is [s, s] and the first sampled action
    if (lane < S) endv = t.state[(size_t)par * S + lane];
    const bool zero = __ballot(lane < S && endv != 0.0) == 0ull;
    if (!zero) {
      if (lane < S) { es[lane] = endv; es[S + lane] = endv; }
      ns = 2;
    }
    double fa = 0.0;
    if (lane < D) fa = r.first_action ? r.first_action[(size_t)b * D + lane] : ca[lane];
    if (__ballot(lane < D && fa != 0.0) != 0ull) {
      if (lane < D) ea[lane] = fa;
      na = 1;
    }
  } else if (!own) {
    if (lane < S) endv = r.end_state[(size_t)b * S + lane];
    owner = r.shard > 0 ? b / r.shard : 0;
    ns = -1;
    na = -1;
  } else {
    if (lane < S) endv = r.end_state[(size_t)b * S + lane];
    owner = r.shard > 0 ? b / r.shard : -1;
    const int run = r.chunks_run[b];
    const int rows_s = run * (A + 1), rows_a = run * A;
    // serial compaction per wave: rows are few (<= 72) and small
    for (int row = 0; row < rows_s; ++row) {
      const double v = lane < S ? cs[(size_t)row * S + lane] : 0.0;
      if (__ballot(v != 0.0) != 0ull) {
        if (lane < S) es[(size_t)ns * S + lane] = v;
        ++ns;
      }
    }
    for (int row = 0; row < rows_a; ++row) {
      const double v = lane < D ? ca[(size_t)row * D + lane] : 0.0;
      if (__ballot(v != 0.0) != 0ull) {
        if (lane < D) ea[(size_t)na * D + lane] = v;
        ++na;
      }
    }
  }
  if (lane < S) t.state[(size_t)id * S + lane] = endv;
  if (lane < 2) t.xy[(size_t)id * 2 + lane] = endv;
  const double psi = __shfl(endv, 2), ex = __shfl(endv, 0), ey = __shfl(endv, 1);
  if (lane == 0) {
    t.parent[id] = par;
    t.has_prev[id] = 1;
    t.num_visit[id] = 0;
    t.edge_nstates[id] = ns;
    t.edge_nactions[id] = na;
    if (cost != nullptr) cost[id] = cost[par] + ns + 1;
    if constexpr (KEY)
      bd.key[id] = cost[par] + ns + 1 + bound_h(ex, ey, bd.goal_xy[2 * tr], bd.goal_xy[2 * tr + 1], bd.goal_radius, bd.reach);
    if (t.edge_owner != nullptr) t.edge_owner[id] = owner;
    if (t.obstacle_ahead != nullptr)                                   // RRT.py:202-205 (run_type > 0)
      t.obstacle_ahead[id] = obstacle_ahead_dev(ex, ey, psi, maze, rows, cols, ahead) ? 1 : 0;
  }
  if (lane < D) {
    double la;
    // a lane reads back what it stored itself (same address, program order)
    if (r.last_action != nullptr && b != phantom) la = r.last_action[(size_t)b * D + lane];     // exchanged record
    else la = (na > 0) ? ea[(size_t)(na - 1) * D + lane] : 0.0;
    t.last_action[(size_t)id * D + lane] = la;
  }
  if (t.hist != nullptr) {
    // what the first sampler call of a child will see (RRT.py:146-147: parent_states_seq, fm_policy.py:96-102: its last
    // obs_history = 3 rows): valid rows at the END of the node's three slots
    double* h = t.hist + (size_t)id * 3 * S;
    int n;
    if (ns >= 0) {
      n = ns < 3 ? ns : 3;
      for (int q = 0; q < n; ++q)
        if (lane < S) h[(size_t)(3 - n + q) * S + lane] = es[(size_t)(ns - n + q) * S + lane];
    } else {
      n = r.hist_n[b];
      for (int q = 3 - n; q < 3; ++q)
        if (lane < S) h[(size_t)q * S + lane] = r.hist[((size_t)b * 3 + q) * S + lane];
    }
    if (lane == 0) t.hist_n[id] = n;
  }
}

// ---- candidate records of a sharded round (include/ditree.h "Candidate record"): R = S + 2 D + 2 [+ 3 S] doubles
__device__ __forceinline__ bool row_is_zero(const double* p, int n) {
  bool z = true;
  for (int k = 0; k < n; ++k) z &= (p[k] == 0.0);
  return z;
}
__global__ void round_pack_kernel(ditree_tree t, ditree_round r, double* __restrict__ rec, int R) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= r.B) return;
  const int A = t.A, nC = t.n_chunks, S = t.state_dim, D = t.action_dim;
  double* o = rec + (size_t)b * R;
  for (int k = 0; k < S; ++k) o[k] = r.end_state[(size_t)b * S + k];
  const double* ca = r.actions + (size_t)b * nC * A * D;
  // last kept (non-zero) action row of the chunks that ran: what accept_commit_kernel derives from the compacted edge
  double* la = o + S;
  for (int k = 0; k < D; ++k) la[k] = 0.0;
  for (int row = r.chunks_run[b] * A - 1; row >= 0; --row) {
    if (!row_is_zero(ca + (size_t)row * D, D)) {
      for (int k = 0; k < D; ++k) la[k] = ca[(size_t)row * D + k];
      break;
    }
  }
  for (int k = 0; k < D; ++k) o[S + D + k] = ca[k];
  int n = 0;
  if (t.hist != nullptr) {
    // the last <= 3 kept state rows, valid rows at the end of the three slots
    const double* cs = r.states + (size_t)b * nC * (A + 1) * S;
    double* h = o + S + 2 * D + 2;
    for (int k = 0; k < 3 * S; ++k) h[k] = 0.0;
    for (int row = r.chunks_run[b] * (A + 1) - 1; row >= 0 && n < 3; --row) {
      if (!row_is_zero(cs + (size_t)row * S, S)) {
        for (int k = 0; k < S; ++k) h[(size_t)(2 - n) * S + k] = cs[(size_t)row * S + k];
        ++n;
      }
    }
  }
  int32_t* oi = (int32_t*)(o + S + 2 * D);
  oi[0] = r.parent[b]; oi[1] = r.status[b]; oi[2] = r.chunks_run[b]; oi[3] = n;
}
__global__ void round_unpack_kernel(ditree_tree t, ditree_round r, const double* __restrict__ rec, int R) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= r.B) return;
  const int S = t.state_dim, D = t.action_dim;
  const double* o = rec + (size_t)b * R;
  for (int k = 0; k < S; ++k) r.end_state[(size_t)b * S + k] = o[k];
  for (int k = 0; k < D; ++k) {
    r.last_action[(size_t)b * D + k] = o[S + k];
    r.first_action[(size_t)b * D + k] = o[S + D + k];
  }
  const int32_t* oi = (const int32_t*)(o + S + 2 * D);
  r.parent[b] = oi[0]; r.status[b] = oi[1]; r.chunks_run[b] = oi[2];
  if (t.hist != nullptr) {
    r.hist_n[b] = oi[3];
    const double* h = o + S + 2 * D + 2;
    for (int k = 0; k < 3 * S; ++k) r.hist[(size_t)b * 3 * S + k] = h[k];
  }
}
int record_doubles(const ditree_tree& t) { return t.state_dim + 2 * t.action_dim + 2 + (t.hist ? 3 * t.state_dim : 0); }
void launch_round_pack(const ditree_tree& t, const ditree_round& r, double* rec, hipStream_t s) {
  hipLaunchKernelGGL(round_pack_kernel, dim3((r.B + 127) / 128), dim3(128), 0, s, t, r, rec, record_doubles(t));
}
void launch_round_unpack(const ditree_tree& t, const ditree_round& r, const double* rec, hipStream_t s) {
  hipLaunchKernelGGL(round_unpack_kernel, dim3((r.B + 127) / 128), dim3(128), 0, s, t, r, rec, record_doubles(t));
}

// The accept of a round on the trees `ts`: scan -> commit; best: with the cost column, then the pick; bounded (bd != NULL,
// cost = bd->cost): the cost pre-pass first, the commit writes the key column too, the pick the stats rows.  sp != NULL (best or
// bounded): the sparse rule's pre-pass and scan in their place.
void launch_accept(const ditree_tree& t, const ditree_round& r, const TreeSet& ts, AcceptMode mode, int emulate_sticky,
                   int32_t* cost, const BoundArg* bd, const unsigned char* maze, int rows, int cols, const AheadArg& ahead,
                   hipStream_t s, const SparseArg* sp) {
  const BoundArg b = bd ? *bd : BoundArg{};
  const dim3 trees(ts.T), cands(r.B);
  const bool bounded = mode == AcceptMode::bounded;
  if (sp) {            // best or bounded under the sparse rule: its own pre-pass and scan, then the mode's commit and pick
    hipLaunchKernelGGL(bounded ? sparse_cost_kernel<true> : sparse_cost_kernel<false>, cands, dim3(64), 0, s, t, r, ts, cost, b, *sp);
    hipLaunchKernelGGL(bounded ? accept_scan_sparse_kernel<AcceptMode::bounded> : accept_scan_sparse_kernel<AcceptMode::best>, trees,
                       dim3(1024), 0, s, t, r, ts, b, cost, *sp);
  } else {
    const auto scan = mode == AcceptMode::first  ? accept_scan_kernel<AcceptMode::first>
                      : mode == AcceptMode::best ? accept_scan_kernel<AcceptMode::best>
                                                 : accept_scan_kernel<AcceptMode::bounded>;
    if (bounded) hipLaunchKernelGGL(accept_cost_kernel, cands, dim3(64), 0, s, t, r, ts, b);
    hipLaunchKernelGGL(scan, trees, dim3(1024), 0, s, t, r, ts, emulate_sticky, b);
  }
  hipLaunchKernelGGL(bounded ? accept_commit_kernel<true> : accept_commit_kernel<false>, cands, dim3(64), 0, s, t, r, maze, rows,
                     cols, ahead, ts, cost, b);
  if (mode != AcceptMode::first)
    hipLaunchKernelGGL(bounded ? accept_pick_kernel<true> : accept_pick_kernel<false>, trees, dim3(1024), 0, s, r, ts, cost, b);
}
void launch_bound_keys(const double* xy, int first, int n, int C, const BoundArg& bd, hipStream_t s) {
  hipLaunchKernelGGL(bound_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const double2*)xy, first, n, C, bd);
}


// ------------------------------------------------------------------------- re-planning on a kept tree (ditree_tree_rebase)
// include/ditree.h "re-planning on a kept tree".  src is read only; every kernel derives the node count and the device-side
// refusal from src itself, so all of them take the same branch.  The flag words of the keep passes are (ancestor << 1) | ok,
// ancestor -1 = the chain has reached the anchor (ok: nothing on it is blocked) or left the subtree (ok = 0).
__device__ __forceinline__ int rebase_nodes(const ditree_tree& src) {
  const int n = src.counters[0];
  return n > src.capacity ? src.capacity : n;
}
__device__ __forceinline__ int rebase_status(const ditree_tree& src, const RebaseArg& a, int n) {
  if (a.anchor >= n) return DITREE_REBASE_E_ANCHOR;
  if (a.fresh_root) {
    const int ns = src.edge_nstates[a.anchor], na = src.edge_nactions[a.anchor];
    if (!(a.drop_states > 0 && a.drop_states < ns && a.drop_actions >= 0 && a.drop_actions < na)) return DITREE_REBASE_E_DROP;
  }
  return 0;
}
// One wave per node: is any kept row of its edge, or its state, in collision on the staged maze?  The anchor keeps the rows
// from drop_states on (a fresh root) or none (it becomes the root).  A NaN row collides (ball_collides: out of the map).
__global__ void __launch_bounds__(256)
rebase_valid_kernel(ditree_tree src, RebaseArg a, const unsigned char* __restrict__ maze, int rows, int cols,
                    int32_t* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  stage_maze(lds, maze, rows * cols);
  const int n = rebase_nodes(src);
  if (rebase_status(src, a, n) != 0) return;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= n) return;
  const int par = m == a.anchor ? -1 : src.parent[m];
  if (m < a.anchor || (m != a.anchor && (par < a.anchor || par >= m))) {       // (accept appends in order: parent < child)
    if (lane == 0) flag[m] = -2;
    return;
  }
  const int S = src.state_dim, cap = src.n_chunks * (src.A + 1);
  int ns = src.edge_nstates[m];
  ns = ns < 0 ? 0 : (ns > cap ? cap : ns);
  const int first = m == a.anchor ? (a.fresh_root ? a.drop_states : ns) : 0;
  const double* es = src.edge_states + (size_t)m * cap * S;
  const double* st = src.state + (size_t)m * S;
  bool bad = false;
  for (int r = first + lane; r <= ns; r += 64) {               // row ns: the node's own state
    const double* p = r < ns ? es + (size_t)r * S : st;
    bad |= car_collides(p[0], p[1], p[2], lds, rows, cols);
  }
  const bool blocked = __ballot(bad) != 0ull;
  if (lane == 0) flag[m] = par * 2 + (blocked ? 0 : 1);
}
// One pointer-doubling pass: a chain of 2^k hops is covered after k passes.
__global__ void __launch_bounds__(256)
rebase_keep_pass_kernel(ditree_tree src, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= rebase_nodes(src)) return;
  int v = in[m];
  const int anc = v >> 1;
  if (anc >= 0) {
    const int w = in[anc];
    v = (w >> 1) * 2 + (v & w & 1);
  }
  out[m] = v;
}
// New ids = exclusive scan of the keep flags (+ 1 behind a fresh root), 1024 nodes at a time, and dst's counter row.  An
// anchor that becomes the root is kept even when the car's own pose collides: its flag then only cuts off what hangs below.
// A refused call writes its status to dst->counters[0] and nothing else.
__global__ void __launch_bounds__(1024)
rebase_scan_kernel(ditree_tree src, ditree_tree dst, RebaseArg a, const int32_t* __restrict__ flag, int32_t* __restrict__ new_id) {
  __shared__ int s_wave_sum[16];
  __shared__ int s_goal;
  const int tid = threadIdx.x;
  const int n = rebase_nodes(src);
  const int status = rebase_status(src, a, n);
  if (status != 0) {
    if (tid == 0) dst.counters[0] = status;
    return;
  }
  const int goal = src.counters[1];
  if (tid == 0) s_goal = -1;
  __syncthreads();
  int base = a.fresh_root ? 1 : 0;
  for (int start = 0; start < n; start += blockDim.x) {
    const int m = start + tid;
    const int keep = m < n ? ((flag[m] & 1) | (!a.fresh_root && m == a.anchor)) : 0;
    int v = keep;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int o = __shfl_up(v, d);
      if ((tid & 63) >= d) v += o;
    }
    if ((tid & 63) == 63) s_wave_sum[tid >> 6] = v;
    __syncthreads();
    int woff = 0, total = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
      if (w < (tid >> 6)) woff += s_wave_sum[w];
      total += s_wave_sum[w];
    }
    if (m < n) {
      const int id = keep ? base + woff + v - 1 : -1;
      new_id[m] = id;
      if (m == goal) s_goal = id;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    dst.counters[0] = base;
    dst.counters[1] = s_goal;
    for (int k = 2; k < 7; ++k) dst.counters[k] = 0;
    dst.counters[7] = -1;
  }
}
// One wave per kept node moves it to its new slot (accept_commit_kernel's fields).  The edge rows of the car are whole double2
// pairs (S = 6, D = 2), so a node's edge is one flat copy; the anchor's starts behind its dropped rows.  The obstacle-ahead
// flag is evaluated on the current maze, as the commit does for a new node; the root's is 0, as DeviceTree.reset leaves it.
__global__ void __launch_bounds__(256)
rebase_move_kernel(ditree_tree src, ditree_tree dst, RebaseArg a, const int32_t* __restrict__ new_id,
                   const int32_t* __restrict__ cost_src, int32_t* __restrict__ cost_dst, const unsigned char* __restrict__ maze,
                   int rows, int cols, AheadArg ahead) {
  const int n = rebase_nodes(src);
  if (rebase_status(src, a, n) != 0) return;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= n) return;
  const int S = src.state_dim, D = src.action_dim;
  const bool anchor = m == a.anchor, root = anchor && !a.fresh_root;
  if (anchor && a.fresh_root) {                        // node 0, whether or not the anchor survives behind it
    if (lane < S) dst.state[lane] = a.root[lane];
    if (lane < 2) dst.xy[lane] = a.root[lane];
    if (lane < D) dst.last_action[lane] = 0.0;
    if (lane == 0) {
      dst.parent[0] = -1;
      dst.has_prev[0] = 0;
      dst.num_visit[0] = 0;
      dst.edge_nstates[0] = 0;
      dst.edge_nactions[0] = 0;
      if (cost_dst != nullptr) cost_dst[0] = 1;
      if (dst.edge_owner != nullptr) dst.edge_owner[0] = -1;
      if (dst.obstacle_ahead != nullptr) dst.obstacle_ahead[0] = 0;
    }
  }
  const int id = new_id[m];
  if (id < 0) return;
  const int es_cap = src.n_chunks * (src.A + 1), ea_cap = src.n_chunks * src.A;
  int ns = min(max(src.edge_nstates[m], 0), es_cap), na = min(max(src.edge_nactions[m], 0), ea_cap);
  int s0 = 0, a0 = 0;
  if (root) { ns = 0; na = 0; }
  else if (anchor) { s0 = a.drop_states; a0 = a.drop_actions; ns = max(ns - s0, 0); na = max(na - a0, 0); }
  const double2* es = (const double2*)(src.edge_states + ((size_t)m * es_cap + s0) * S);
  const double2* ea = (const double2*)(src.edge_actions + ((size_t)m * ea_cap + a0) * D);
  double2* ds = (double2*)(dst.edge_states + (size_t)id * es_cap * S);
  double2* da = (double2*)(dst.edge_actions + (size_t)id * ea_cap * D);
  for (int k = lane; k < ns * S / 2; k += 64) ds[k] = es[k];
  for (int k = lane; k < na * D / 2; k += 64) da[k] = ea[k];
  double sv = 0.0;
  if (lane < S) {
    sv = src.state[(size_t)m * S + lane];
    dst.state[(size_t)id * S + lane] = sv;
  }
  if (lane < 2) dst.xy[(size_t)id * 2 + lane] = sv;
  if (lane < D) dst.last_action[(size_t)id * D + lane] = root ? 0.0 : src.last_action[(size_t)m * D + lane];
  const double ex = __shfl(sv, 0), ey = __shfl(sv, 1), psi = __shfl(sv, 2);
  if (lane == 0) {
    // the anchor's cost: 1 as the root, else the fresh root's row + its kept edge rows + its own state
    const int c_anchor = a.fresh_root ? 2 + src.edge_nstates[a.anchor] - a.drop_states : 1;
    dst.parent[id] = anchor ? (a.fresh_root ? 0 : -1) : new_id[src.parent[m]];
    dst.has_prev[id] = root ? 0 : src.has_prev[m];
    dst.num_visit[id] = src.num_visit[m];
    dst.edge_nstates[id] = ns;
    dst.edge_nactions[id] = na;
    if (cost_dst != nullptr) cost_dst[id] = anchor ? c_anchor : cost_src[m] - cost_src[a.anchor] + c_anchor;
    if (dst.edge_owner != nullptr) dst.edge_owner[id] = src.edge_owner != nullptr ? src.edge_owner[m] : -1;
    if (dst.obstacle_ahead != nullptr)
      dst.obstacle_ahead[id] = (!root && obstacle_ahead_dev(ex, ey, psi, maze, rows, cols, ahead)) ? 1 : 0;
  }
}
// scratch: [0, cap) and [cap, 2 cap) the two flag buffers of the keep passes, [2 cap, 3 cap) the new ids.
void launch_tree_rebase(const ditree_tree& src, const ditree_tree& dst, const RebaseArg& a, const int32_t* cost_src,
                        int32_t* cost_dst, int32_t* scratch, const unsigned char* maze, int rows, int cols, const AheadArg& ahead,
                        hipStream_t s) {
  const int cap = src.capacity;
  int32_t* buf[2] = {scratch, scratch + cap};
  int32_t* new_id = scratch + 2 * (size_t)cap;
  const size_t lds = ((size_t)rows * cols + 15) & ~(size_t)15;
  const dim3 waves((cap + 3) / 4), threads((cap + 255) / 256);
  hipLaunchKernelGGL(rebase_valid_kernel, waves, dim3(256), lds, s, src, a, maze, rows, cols, buf[0]);
  int cur = 0;
  for (int64_t hops = 1; hops < cap; hops *= 2, cur ^= 1)
    hipLaunchKernelGGL(rebase_keep_pass_kernel, threads, dim3(256), 0, s, src, buf[cur], buf[cur ^ 1]);
  hipLaunchKernelGGL(rebase_scan_kernel, dim3(1), dim3(1024), 0, s, src, dst, a, buf[cur], new_id);
  hipLaunchKernelGGL(rebase_move_kernel, waves, dim3(256), 0, s, src, dst, a, new_id, cost_src, cost_dst, maze, rows, cols, ahead);
}
