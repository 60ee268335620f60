// What the mesh topology files (holes, smoothing, decimation, simplification, components) share: which faces count, a
// binary search, and the f64 point arithmetic behind their bit-exact promises.  The build has
// -ffp-contract=off: every product, sum and difference below is rounded on its own, in the order written, so a call here
// gives the bits of the same expression written out.
#pragma once
#include "common.h"

namespace mslam {

// all three indices in [0, nv)
__device__ __forceinline__ bool tp_in_range(int a, int b, int c, int nv) {
  return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
}

// a COUNTING face: indices in [0, nv), pairwise different
__device__ __forceinline__ bool tp_counts(int a, int b, int c, int nv) {
  return tp_in_range(a, b, c, nv) && a != b && b != c && a != c;
}

// the first position of `sorted` (ascending, n entries) that is >= v; positions are computed in I
template <class T, class I>
__device__ __forceinline__ I tp_lower(const T* __restrict__ sorted, I n, T v) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the position of v in `sorted` when it occurs exactly once, else -1
template <class T, class I>
__device__ __forceinline__ I tp_once(const T* __restrict__ sorted, I n, T v) {
  const I p = tp_lower(sorted, n, v);
  if (p >= n || sorted[p] != v) return -1;
  return (p + 1 < n && sorted[p + 1] == v) ? -1 : p;
}

// vertex i of an f32[V,3] array, widened
__device__ __forceinline__ void tp_point(const float* __restrict__ v, int i, double (&p)[3]) {
  p[0] = (double)v[3 * (size_t)i], p[1] = (double)v[3 * (size_t)i + 1], p[2] = (double)v[3 * (size_t)i + 2];
}

__device__ __forceinline__ void tp_sub(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
  r[0] = a[0] - b[0], r[1] = a[1] - b[1], r[2] = a[2] - b[2];
}

__device__ __forceinline__ void tp_cross(const double (&u)[3], const double (&v)[3], double (&r)[3]) {
  r[0] = u[1] * v[2] - u[2] * v[1];
  r[1] = u[2] * v[0] - u[0] * v[2];
  r[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ double tp_dot(const double (&u)[3], const double (&v)[3]) {
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

}  // namespace mslam
