// Lidar ray march and maze cell codes shared by the units that scan on the device (geom_kernels.hip: lidar_scan_kernel and
// the plan follower; mppi_mission_kernels.hip: the MPPI mission loop).  Units that include this header are compiled with
// -ffp-contract=off: the only fused operations are the explicit fma() calls that restate the reference's LAPACK / BLAS.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ bool border_solve(double rx, double ry, double dx, double dy, double b0, double b1,
                                             double* t, double* s) {
  // np.linalg.solve([[rx, -dx], [ry, -dy]], b) as OpenBLAS evaluates it (verified bit-exact on
  // the build host): partial pivoting, multiplier scaled by the reciprocal pivot, FMA updates,
  // true divisions in the back substitution.  lidar_2d_sim.py:69-77.
  double a00 = rx, a01 = -dx, a10 = ry, a11 = -dy;
  if (fabs(a10) > fabs(a00)) {
    double t0 = a00; a00 = a10; a10 = t0;
    t0 = a01; a01 = a11; a11 = t0;
    t0 = b0; b0 = b1; b1 = t0;
  }
  if (a00 == 0.0) return false;
  double l = a10 * (1.0 / a00);
  double u11 = fma(-l, a01, a11);
  if (u11 == 0.0) return false;                          // LinAlgError: singular (ray parallel to border)
  double y1 = fma(-l, b0, b1);
  double x1 = y1 / u11;
  double x0 = fma(-a01, x1, b0) / a00;
  *t = x0;
  *s = x1;
  return true;
}

// One ray of Lidar2DSim._cast_ray + the endpoint re-derivation of scan() (lidar_2d_sim.py:18-98).  `mz` holds
// 1 for occupied cells, visited cells are OR-ed into `vis`.
__device__ __forceinline__ void lidar_ray(double x0, double y0, double yaw, int ray, const unsigned char* mz, int rows,
                                          int cols, unsigned char* vis, double* d_out, double* ex_out, double* ey_out,
                                          bool* hit_out) {
  // x runs along columns, y along rows: width = cols, height = rows.  The reference unpacks maze_data.shape the other
  // way round (:51), which is the same arithmetic on a square map and raises on any other; there this is the build's own
  // definition.
  const double mw = (double)cols, mh = (double)rows;
  const double angle = -180.0 + 2.0 * (double)ray;                 // np.arange(-180, 182, 2)
  const double ang = (yaw + angle) * (M_PI / 180.0);               // np.deg2rad(yaw + angle) (:53-54)
  double rx, ry;
  sincos(ang, &ry, &rx);
  // borders Left, Right, Bottom, Top (:57-62): origin b0, direction d
  const double bx[4] = {0.0, mw, 0.0, 0.0}, by[4] = {0.0, 0.0, 0.0, mh};
  const double dxs[4] = {0.0, 0.0, mw, mw}, dys[4] = {mh, mh, 0.0, 0.0};
  double lx = x0, ly = y0;
  bool found = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (found) continue;
    double t, s;
    if (border_solve(rx, ry, dxs[k], dys[k], bx[k] - x0, by[k] - y0, &t, &s)) {
      if (t >= 0.0 && s <= 1.0 && s >= 0.0) {                        // :74
        lx = t * rx + x0;
        ly = t * ry + y0;
        found = true;
      }
    }
  }
  const double vx = lx - x0, vy = ly - y0;
  const double len = sqrt(fma(vy, vy, vx * vx));                     // np.linalg.norm (ddot = one fma)
  const double step = 0.1 / len;                                     // :85
  // len(np.arange(0, 1, step)) = ceil((1 - 0) / step)
  double nf = ceil(1.0 / step);
  long long n = (found && nf > 0.0 && nf < 1e9) ? (long long)nf : 0;
  bool h = false;
  double ox = lx, oy = ly;
  for (long long i = 0; i < n; ++i) {
    double t = (double)i * step;                                     // arange value start + i*delta
    double px = x0 + t * vx, py = y0 + t * vy;                       // :86
    double fx = floor(px), fy = floor(py);
    int qx = fx >= 0.0 ? (fx < mw ? (int)fx : cols - 1) : 0;         // clip to [0, maze_width-1]  (:89)
    int qy = fy >= 0.0 ? (fy < mh ? (int)fy : rows - 1) : 0;         // clip to [0, maze_height-1]
    // maze_data[q_y, q_x] (:91): q_y indexes rows, q_x columns; both are inside the map after the clip
    if (mz[qy * cols + qx] == 1) {
      h = true;
      ox = px;
      oy = py;
      break;
    }
    vis[qy * cols + qx] = 1;                                         // benign race: all writers store 1
  }
  double ex = ox - x0, ey = oy - y0;
  double d = sqrt(fma(ey, ey, ex * ex));                             // :96
  d = d < 0.0 ? 0.0 : (d > 300.0 ? 300.0 : d);                       // scan(): np.clip(d, 0, max_range) (:33)
  *d_out = d;
  *ex_out = x0 + d * rx;                                             // :36-39
  *ey_out = y0 + d * ry;
  *hit_out = h;
}

// f32 maze value -> u8 cell code (what ditree_upload_maze stores): integers 0..255 as they are, anything else 255
__device__ __forceinline__ unsigned char maze_code(float v) {
  int c = (int)v;
  return (v == (float)c && c >= 0 && c < 256) ? (unsigned char)c : (unsigned char)255;
}
