// Cloud views: the z-buffer splat of a point cloud into pinhole views, its resolve into range / index / hit / rgb
// images, and the observed rule of observed_cloud_points.  Semantics in DESIGN.md "Cloud views"; tests/cloudview_numpy.py
// states the same definitions, operation by operation, in numpy.  Everything is f64 on the f32 inputs and the build has
// -ffp-contract=off, so a * b + c below is two roundings, as in numpy.  The projection is the one of observed_points
// (tests/raycast_numpy.view_rays), with its grouping of sums.
//
// THE Z-BUFFER.  One u64 per pixel and view, all ones when empty.  A point in view covers the square |dx|, |dy| <= rho
// around its pixel, clipped to the image, and every covered pixel takes the minimum of
//     key = (bits of f32(r) as u32) << 32 | index,       r = |p - o| >= 0,
// so the order of the keys is the order of (f32 range, index): the nearest range wins, then the lowest index.  A
// minimum does not depend on the order of its operands, so neither does the image depend on the order in which points,
// waves or views run, and two launches on the same inputs give the same bytes.
//
// STRUCTURE.  One thread per (point, view); the view is blockIdx.y, so pose and intrinsics are wave-uniform.  The
// footprint loop issues one 64-bit no-return atomic minimum per pixel it has to lower, and none where the pixel already
// holds a key that is not above its own (see cv_splat_kernel).  No LDS, no returned atomic, no compare-and-swap loop.
#include "common.h"
#include "view.h"

namespace mslam {

constexpr int kCvBlock = 256;
constexpr unsigned long long kCvEmpty = ~0ull;

struct CvProjection {
  bool in_view;
  int px, py;
  double r, z;
};

// A cloud point against one view (view.h view_project, with its grouping of sums): a point with a non-finite coordinate
// is in no view, and the pixel is the nearest centre.
__device__ __forceinline__ CvProjection cv_project(const float* __restrict__ p3, const float* __restrict__ pose8,
                                                   const ViewCamera& c) {
  CvProjection out;
  const double p[3] = {(double)p3[0], (double)p3[1], (double)p3[2]};
  const ViewProjection pr = view_project(p, pose8, c);
  const bool finite = fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY;
  out.in_view = finite && pr.in_view;
  // in view, u + 0.5 lies in [0, w): the min is a guard against an index outside the image and changes no value
  out.px = out.in_view ? min((int)floor(pr.u + 0.5), c.w - 1) : 0;
  out.py = out.in_view ? min((int)floor(pr.v + 0.5), c.h - 1) : 0;
  out.r = pr.r;
  out.z = pr.z;
  return out;
}

// kCount: a measurement build of the same loop; counters[0] += footprint pixels visited, counters[1] += atomics issued.
template <bool kCount>
__global__ __launch_bounds__(kCvBlock) void cv_splat_kernel(const float* __restrict__ points, int n,
                                                            const float* __restrict__ poses, ViewCamera cam, int radius,
                                                            double half_size_f, int max_radius,
                                                            unsigned long long* __restrict__ zbuf,
                                                            unsigned long long* __restrict__ counters) {
  const long long i = (long long)blockIdx.x * kCvBlock + threadIdx.x;
  const int view = blockIdx.y;
  unsigned long long visited = 0, issued = 0;
  if (i < n) {
    const CvProjection pr = cv_project(points + 3 * i, poses + 8 * (size_t)view, cam);
    if (pr.in_view) {
      int rho = radius;
      if (half_size_f >= 0.0) {
        // min(max_radius, max(radius, floor(0.5 point_size max(fx, fy) / X2))), the min before the conversion
        double g = floor(half_size_f / pr.z);
        g = g > (double)radius ? g : (double)radius;
        g = g < (double)max_radius ? g : (double)max_radius;
        rho = (int)g;
      }
      const unsigned long long key =
          ((unsigned long long)__float_as_uint((float)pr.r) << 32) | (unsigned long long)(unsigned)i;
      unsigned long long* z = zbuf + (size_t)view * cam.h * cam.w;
      const int x0 = max(pr.px - rho, 0), x1 = min(pr.px + rho, cam.w - 1);
      const int y0 = max(pr.py - rho, 0), y1 = min(pr.py + rho, cam.h - 1);
      for (int y = y0; y <= y1; y++) {
        for (int x = x0; x <= x1; x++) {
          unsigned long long* cell = z + (size_t)y * cam.w + x;
          if (kCount) visited++;
          // The plain load may be stale - another point's atomic may have lowered the pixel since.  Keys only fall
          // during a launch, so the pixel's true value is <= what was read: when the read value is already <= key,
          // the minimum with key would change nothing, and the skip is right.  A stale read can only be too HIGH, and
          // then the atomic is issued although it was not needed: a redundant atomic, never a wrong skip.
          if (*cell <= key) continue;
          atomicMin(cell, key);                        // result unused: the no-return form
          if (kCount) issued++;
        }
      }
    }
  }
  if (kCount) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      visited += __shfl_down(visited, off, kWave);
      issued += __shfl_down(issued, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && visited) {
      atomicAdd(counters, visited);
      atomicAdd(counters + 1, issued);
    }
  }
}

// One thread per pixel of every view: hit, index (-1), range = f32(f64(r32) / s) (0), rgb = the winner's colour (0).
__global__ __launch_bounds__(kCvBlock) void cv_resolve_kernel(const unsigned long long* __restrict__ zbuf,
                                                              const float* __restrict__ poses, int hw, int total,
                                                              const uint8_t* __restrict__ colors, int n,
                                                              float* __restrict__ range, int32_t* __restrict__ index,
                                                              uint8_t* __restrict__ hit, uint8_t* __restrict__ rgb) {
  const long long i = (long long)blockIdx.x * kCvBlock + threadIdx.x;
  if (i >= total) return;
  const unsigned long long key = zbuf[i];
  const bool has = key != kCvEmpty;
  const int idx = has ? (int)(unsigned)(key & 0xffffffffull) : -1;
  float rng = 0.0f;
  if (has) {
    const double s = (double)poses[8 * (size_t)(i / hw) + 7];
    rng = (float)((double)__uint_as_float((unsigned)(key >> 32)) / s);
  }
  range[i] = rng;
  index[i] = idx;
  hit[i] = has ? 1 : 0;
  if (rgb) {
    const bool read = has && idx >= 0 && idx < n;      // a key of this cloud's splat names one of its points
#pragma unroll
    for (int c = 0; c < 3; c++) rgb[3 * i + c] = read ? colors[3 * (size_t)idx + c] : (uint8_t)0;
  }
}

// One thread per (query, view).  Every writer stores the same 1, and a query that an earlier launch (or another view
// of this one) has marked leaves at once; `seen` is never cleared here.
__global__ __launch_bounds__(kCvBlock) void cv_visible_kernel(const float* __restrict__ queries, int m,
                                                              const unsigned long long* __restrict__ zbuf,
                                                              const float* __restrict__ poses, ViewCamera cam, double tol,
                                                              double rel_tol, uint8_t* __restrict__ seen) {
  const long long i = (long long)blockIdx.x * kCvBlock + threadIdx.x;
  const int view = blockIdx.y;
  if (i >= m || seen[i]) return;
  const CvProjection pr = cv_project(queries + 3 * i, poses + 8 * (size_t)view, cam);
  if (!pr.in_view) return;
  const unsigned long long key = zbuf[((size_t)view * cam.h + pr.py) * cam.w + pr.px];
  // the query's own range rounded to f32 first, so that a point that wins its pixel sees itself at tol = rel_tol = 0
  const double own = (double)(float)pr.r, win = (double)__uint_as_float((unsigned)(key >> 32));
  if (key == kCvEmpty || own <= win * (1.0 + rel_tol) + tol) seen[i] = 1;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_cloud_view_splat(const float* points, int num_points, const float* poses, int num_views, double fx,
                                      double fy, double cx, double cy, int h, int w, double near, double far,
                                      int radius, double point_size, int max_radius, uint64_t* zbuf, uint64_t* counters,
                                      void* stream) {
  const char* what = "cloud_view_splat";
  MSLAM_REQUIRE(num_points >= 0, "%s: negative size", what);
  const double K4[4] = {fx, fy, cx, cy};
  if (int rc = view_check(what, num_views, h, w, K4, near, far, false)) return rc;
  MSLAM_REQUIRE(0 <= radius && radius <= max_radius && max_radius <= MSLAM_CLOUD_VIEW_MAX_RADIUS,
                "%s: need 0 <= radius <= max_radius <= %d, got %d and %d", what, MSLAM_CLOUD_VIEW_MAX_RADIUS, radius,
                max_radius);
  MSLAM_REQUIRE(point_size < 0.0 || view_finite(point_size), "%s: point_size must be finite (negative: none)", what);
  const size_t pixels = (size_t)num_views * h * w;
  if (pixels == 0) return MSLAM_OK;
  MSLAM_REQUIRE(zbuf && poses && (points || num_points == 0), "%s: null pointer", what);
  if (int rc = check_hip(hipMemsetAsync(zbuf, 0xff, pixels * sizeof(uint64_t), (hipStream_t)stream),
                         "cloud_view_splat memset"))
    return rc;
  if (num_points == 0) return MSLAM_OK;
  const ViewCamera cam = {fx, fy, cx, cy, h, w, near, far};
  const double half_size_f = point_size < 0.0 ? -1.0 : 0.5 * point_size * (fx > fy ? fx : fy);
  const dim3 grid(blocks_for(num_points, kCvBlock), (unsigned)num_views);
  hipLaunchKernelGGL(counters ? cv_splat_kernel<true> : cv_splat_kernel<false>, grid, dim3(kCvBlock), 0,
                     (hipStream_t)stream, points, num_points, poses, cam, radius, half_size_f, max_radius,
                     (unsigned long long*)zbuf, (unsigned long long*)counters);
  MSLAM_LAUNCH_CHECK("cloud_view_splat");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_view_resolve(const uint64_t* zbuf, const float* poses, int num_views, int h, int w,
                                        const uint8_t* colors, int num_points, float* range, int32_t* index,
                                        uint8_t* hit, uint8_t* rgb, void* stream) {
  const char* what = "cloud_view_resolve";
  MSLAM_REQUIRE(num_points >= 0, "%s: negative size", what);
  if (int rc = view_check(what, num_views, h, w, nullptr, 0.0, 0.0, false)) return rc;
  // the colours of an empty cloud may be a null pointer: nothing is read from them
  MSLAM_REQUIRE(rgb ? (colors || num_points == 0) : !colors, "%s: colors and rgb go together", what);
  const int64_t total = (int64_t)num_views * h * w;
  if (total == 0) return MSLAM_OK;
  MSLAM_REQUIRE(zbuf && poses && range && index && hit, "%s: null pointer", what);
  hipLaunchKernelGGL(cv_resolve_kernel, dim3(blocks_for(total, kCvBlock)), dim3(kCvBlock), 0, (hipStream_t)stream,
                     (const unsigned long long*)zbuf, poses, h * w, (int)total, colors, num_points, range, index, hit,
                     rgb);
  MSLAM_LAUNCH_CHECK("cloud_view_resolve");
  return MSLAM_OK;
}

extern "C" int mslam_cloud_view_visible(const float* queries, int num_queries, const uint64_t* zbuf, const float* poses,
                                        int num_views, double fx, double fy, double cx, double cy, int h, int w,
                                        double near, double far, double tol, double rel_tol, uint8_t* seen,
                                        void* stream) {
  const char* what = "cloud_view_visible";
  MSLAM_REQUIRE(num_queries >= 0, "%s: negative size", what);
  const double K4[4] = {fx, fy, cx, cy};
  if (int rc = view_check(what, num_views, h, w, K4, near, far, false)) return rc;
  MSLAM_REQUIRE(tol >= 0.0 && rel_tol >= 0.0, "%s: tol and rel_tol must be >= 0", what);
  if (num_queries == 0 || (size_t)num_views * h * w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(queries && zbuf && poses && seen, "%s: null pointer", what);
  const ViewCamera cam = {fx, fy, cx, cy, h, w, near, far};
  const dim3 grid(blocks_for(num_queries, kCvBlock), (unsigned)num_views);
  hipLaunchKernelGGL(cv_visible_kernel, grid, dim3(kCvBlock), 0, (hipStream_t)stream, queries, num_queries,
                     (const unsigned long long*)zbuf, poses, cam, tol, rel_tol, seen);
  MSLAM_LAUNCH_CHECK("cloud_view_visible");
  return MSLAM_OK;
}
