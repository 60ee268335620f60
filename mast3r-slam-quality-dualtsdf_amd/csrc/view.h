// The camera of every kernel that draws or projects through one, each convention stated once (DESIGN.md "Cameras and
// views"): pose rotation, projection, pixel rays, the watertight shear, the pixel-to-thread map, the host check.  The
// kernels' outputs are pinned bit for bit to numpy statements (tests/raycast_numpy.py and its siblings) and the build has
// -ffp-contract=off: every grouping below is part of the definition.
#pragma once
#include "common.h"

namespace mslam {

// A pose is f32[8] = (t[3], q[4] = x y z w, s): world = s R(q) camera + t.
// out = R(q) v = (v + w u) + q x u, u = 2 q x v, in exactly this grouping.  A caller that rotates by the conjugate
// passes the negated vector part; the negation is exact.  `out` must not alias `v`.
__device__ __forceinline__ void view_rotate(const double q[4], const double v[3], double out[3]) {
  const double u0 = 2.0 * (q[1] * v[2] - q[2] * v[1]);
  const double u1 = 2.0 * (q[2] * v[0] - q[0] * v[2]);
  const double u2 = 2.0 * (q[0] * v[1] - q[1] * v[0]);
  out[0] = (v[0] + q[3] * u0) + (q[1] * u2 - q[2] * u1);
  out[1] = (v[1] + q[3] * u1) + (q[2] * u0 - q[0] * u2);
  out[2] = (v[2] + q[3] * u2) + (q[0] * u1 - q[1] * u0);
}

struct ViewCamera {
  double fx, fy, cx, cy;
  int h, w;
  double near, far;
};

struct ViewProjection {
  bool in_view;
  double u, v;       // pixel coordinates, centres at integers
  double r, z;       // |p - o| in world units; the depth X2 along the optical axis
  double v3[3];      // p - o
};

// A point against one view: v = p - o, X = R(conj q) v, r = |v|, u = fx X0 / X2 + cx, v = fy X1 / X2 + cy; in view when
// X2 > 0, the pixel lies in the image (-0.5 <= u < w - 0.5, the same for v and h) and near <= r <= far.  Every
// comparison is false on a NaN.  What else a caller asks of the point (finiteness, a normal) it tests itself.
__device__ __forceinline__ ViewProjection view_project(const double p[3], const float* __restrict__ pose8,
                                                       const ViewCamera& c) {
  ViewProjection out;
  out.v3[0] = p[0] - (double)pose8[0], out.v3[1] = p[1] - (double)pose8[1], out.v3[2] = p[2] - (double)pose8[2];
  const double qc[4] = {-(double)pose8[3], -(double)pose8[4], -(double)pose8[5], (double)pose8[6]};
  double X[3];
  view_rotate(qc, out.v3, X);
  out.r = sqrt((out.v3[0] * out.v3[0] + out.v3[1] * out.v3[1]) + out.v3[2] * out.v3[2]);
  out.u = c.fx * X[0] / X[2] + c.cx;
  out.v = c.fy * X[1] / X[2] + c.cy;
  out.z = X[2];
  out.in_view = X[2] > 0.0 && out.u >= -0.5 && out.u < (double)c.w - 0.5 && out.v >= -0.5 &&
                out.v < (double)c.h - 0.5 && out.r >= c.near && out.r <= c.far;
  return out;
}

// The world ray of pixel i: origin o = t, direction d = R(q) rays[i] (not normalised, not scaled).
__device__ __forceinline__ void view_ray(const float* __restrict__ rays, size_t i, const float* __restrict__ pose8,
                                         double o[3], double d[3]) {
  const double q[4] = {(double)pose8[3], (double)pose8[4], (double)pose8[5], (double)pose8[6]};
  const double c[3] = {(double)rays[3 * i], (double)rays[3 * i + 1], (double)rays[3 * i + 2]};
  view_rotate(q, c, d);
#pragma unroll
  for (int a = 0; a < 3; a++) o[a] = (double)pose8[a];
}

// K >= 0: component K, a compile-time choice; K = -1: component k.
template <int K>
__device__ __forceinline__ double rc_pick(double a0, double a1, double a2, int k) {
  if (K >= 0) return K == 0 ? a0 : (K == 1 ? a1 : a2);
  return k == 0 ? a0 : (k == 1 ? a1 : a2);
}

struct ViewShear {
  int kx, ky, kz;
  double sx, sy, sz;
  int perm;          // 2 kz + (d[kz] < 0); -1 when the direction is zero or not finite: such a ray cannot be cast
};

// The set-up of the watertight intersection (Woop, Benthin, Wald 2013): kz the largest axis of d, kx, ky the two after
// it in cyclic order, swapped when d[kz] < 0 so that the winding is kept, and the shear sx, sy = d[kx], d[ky] / d[kz],
// sz = 1 / d[kz].  The numbers are computed for any d; whether the ray can be cast is the flag `perm`.
__device__ __forceinline__ ViewShear view_shear(const double d[3]) {
  ViewShear s;
  const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
  int kz = a1 > a0 ? 1 : 0;
  if (a2 > (kz ? a1 : a0)) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dz = rc_pick<-1>(d[0], d[1], d[2], kz);
  if (dz < 0.0) {
    const int t = kx;
    kx = ky, ky = t;
  }
  s.kx = kx, s.ky = ky, s.kz = kz;
  s.sx = rc_pick<-1>(d[0], d[1], d[2], kx) / dz;
  s.sy = rc_pick<-1>(d[0], d[1], d[2], ky) / dz;
  s.sz = 1.0 / dz;
  const bool castable = a0 < INFINITY && a1 < INFINITY && a2 < INFINITY && (a0 > 0.0 || a1 > 0.0 || a2 > 0.0);
  s.perm = castable ? 2 * kz + (dz < 0.0 ? 1 : 0) : -1;
  return s;
}

// Image-shaped launches: 16x16 pixels per 256-thread block, 8x8 per wave (2x2 waves), so that a wave's rays or points
// meet neighbouring voxels or faces.  view_pixel(px, py) / view_tile_grid always tile (the TSDF kernels);
// view_pixel(h, px, py) / view_grid take h = 1 as a list, 256 consecutive rays per block (the mesh kernels).
constexpr int kViewBlock = 256;

__device__ __forceinline__ void view_pixel(int& px, int& py) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

__device__ __forceinline__ void view_pixel(int h, long long& px, int& py) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  px = h == 1 ? (long long)blockIdx.x * kViewBlock + tid : blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  py = h == 1 ? 0 : blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

static inline dim3 view_tile_grid(int h, int w) { return dim3(blocks_for(w, 16), blocks_for(h, 16)); }
static inline dim3 view_grid(int h, int w) { return h == 1 ? dim3(blocks_for(w, kViewBlock)) : view_tile_grid(h, w); }

static inline bool view_finite(double x) { return x - x == 0.0; }

// The checks that the view entry points share; MSLAM_OK, or MSLAM_EINVAL with the error text set.  K4 = (fx, fy, cx,
// cy), or null for an entry point without intrinsics.  `strict`: far > near with a finite span (the TSDF march divides
// by it); otherwise near <= far.  A NaN in near or far fails either.
static int view_check(const char* what, int num_views, int h, int w, const double* K4, double near, double far,
                      bool strict) {
  MSLAM_REQUIRE(num_views >= 0 && h >= 0 && w >= 0, "%s: bad image size: negative", what);
  MSLAM_REQUIRE((int64_t)h * w < (1ll << 31) && (int64_t)h * w * num_views < (1ll << 31) && num_views <= 65535,
                "%s: bad image size: %d views of %d x %d pixels are outside the int32 index range", what, num_views, h,
                w);
  MSLAM_REQUIRE(!K4 || (view_finite(K4[0]) && view_finite(K4[1]) && view_finite(K4[2]) && view_finite(K4[3])),
                "%s: non-finite intrinsics", what);
  if (strict)
    MSLAM_REQUIRE(far > near && far - near < INFINITY, "%s: far must exceed near by a finite span", what);
  else
    MSLAM_REQUIRE(near <= far, "%s: near must not exceed far", what);
  return MSLAM_OK;
}

}  // namespace mslam
