// Triangle helpers shared by the mesh-quality kernels (mesh_distance.hip) and the mesh-alignment kernels
// (mesh_align.hip): the validity rule, the closest point of a triangle by Voronoi regions, the per-tile boxes and the
// distance from a point to a box.  Semantics in DESIGN.md "Mesh quality"; tests/meshdist_numpy.py states the same
// definitions, operation by operation, in numpy.  Everything is f64 on the f32 inputs and the build has
// -ffp-contract=off, so a * b + c below is two roundings, as in numpy.  The invariant that makes culling by these boxes
// exact is in the header comment of mesh_distance.hip.
#pragma once
#include <math.h>

#include "common.h"

namespace mslam {

constexpr int kMdTile = 128;      // triangles per LDS tile and per box; tests/test_mesh_metrics_gpu.py states it too
constexpr int kMdBlock = 256;     // one point per thread
constexpr int kMdTriDoubles = 10; // a, b, c, valid

__device__ __forceinline__ double md_dot(double ax, double ay, double az, double bx, double by, double bz) {
  return ax * bx + ay * by + az * bz;
}

// Face f as nine f64 coordinates t[0..8] = a, b, c and t[9] = 1 (valid) or 0; an invalid face is all zeros.  nsq, when
// given, receives |(b - a) x (c - a)|^2.
__device__ __forceinline__ bool md_load_tri(const float* __restrict__ vert, const int32_t* __restrict__ faces, int f,
                                            int nf, int nv, double* t, double* nsq = nullptr) {
  bool valid = false;
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < kMdTriDoubles; k++) t[k] = 0.0;
  if (f < nf) {
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {
      double v[9];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        v[d] = (double)vert[3 * (size_t)ia + d];
        v[3 + d] = (double)vert[3 * (size_t)ib + d];
        v[6 + d] = (double)vert[3 * (size_t)ic + d];
      }
      const double abx = v[3] - v[0], aby = v[4] - v[1], abz = v[5] - v[2];
      const double acx = v[6] - v[0], acy = v[7] - v[1], acz = v[8] - v[2];
      const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
      valid = nx != 0.0 || ny != 0.0 || nz != 0.0;
      if (valid) {
        n2 = md_dot(nx, ny, nz, nx, ny, nz);
#pragma unroll
        for (int k = 0; k < 9; k++) t[k] = v[k];
        t[9] = 1.0;
      }
    }
  }
  if (nsq) *nsq = n2;
  return valid;
}

// Closest point q[0..2] of the triangle t to p (Ericson, Real-Time Collision Detection 5.1.5): vertex regions A, B,
// edge AB, vertex C, edges AC, BC, interior, in that order.  tests/meshdist_numpy.py `closest` is this, line by line.
__device__ __forceinline__ void md_closest(double px, double py, double pz, const double* t, double* q) {
  const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double d1 = md_dot(abx, aby, abz, apx, apy, apz), d2 = md_dot(acx, acy, acz, apx, apy, apz);
  double qx = ax, qy = ay, qz = az;
  if (!(d1 <= 0.0 && d2 <= 0.0)) {
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double d3 = md_dot(abx, aby, abz, bpx, bpy, bpz), d4 = md_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0 && d4 <= d3) {
      qx = bx, qy = by, qz = bz;
    } else {
      const double vc = d1 * d4 - d3 * d2;
      if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        qx = ax + v * abx, qy = ay + v * aby, qz = az + v * abz;
      } else {
        const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
        const double d5 = md_dot(abx, aby, abz, cpx, cpy, cpz), d6 = md_dot(acx, acy, acz, cpx, cpy, cpz);
        if (d6 >= 0.0 && d5 <= d6) {
          qx = cx, qy = cy, qz = cz;
        } else {
          const double vb = d5 * d2 - d1 * d6;
          if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            qx = ax + w * acx, qy = ay + w * acy, qz = az + w * acz;
          } else {
            const double va = d3 * d6 - d5 * d4;
            const double e1 = d4 - d3, e2 = d5 - d6;
            if (va <= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
              const double w = e1 / (e1 + e2);
              qx = bx + w * (cx - bx), qy = by + w * (cy - by), qz = bz + w * (cz - bz);
            } else {
              const double denom = 1.0 / ((va + vb) + vc);
              const double v = vb * denom, w = vc * denom;
              qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
            }
          }
        }
      }
    }
  }
  q[0] = qx, q[1] = qy, q[2] = qz;
}

// Squared distance from p to the triangle t: |p - q|^2 for the closest point q above
__device__ __forceinline__ double md_dist2(double px, double py, double pz, const double* t) {
  double q[3];
  md_closest(px, py, pz, t, q);
  const double rx = px - q[0], ry = py - q[1], rz = pz - q[2];
  return md_dot(rx, ry, rz, rx, ry, rz);
}

// box[6 * tile + ...] = lo.xyz, hi.xyz over the vertices of the tile's valid faces; (+inf, -inf) for a tile without one.
// static: one copy per translation unit that includes this header.
static __global__ __launch_bounds__(64) void md_box_kernel(const float* __restrict__ vert,
                                                           const int32_t* __restrict__ faces, int nf, int nv,
                                                           double* __restrict__ box) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = lane; k < kMdTile; k += kWave) {
    double t[kMdTriDoubles];
    if (md_load_tri(vert, faces, tile * kMdTile + k, nf, nv, t)) {
#pragma unroll
      for (int j = 0; j < 9; j++) {
        lo[j % 3] = fmin(lo[j % 3], t[j]);
        hi[j % 3] = fmax(hi[j % 3], t[j]);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 3; d++) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[d] = fmin(lo[d], __shfl_down(lo[d], off, kWave));
      hi[d] = fmax(hi[d], __shfl_down(hi[d], off, kWave));
    }
    if (lane == 0) {
      box[6 * (size_t)tile + d] = lo[d];
      box[6 * (size_t)tile + 3 + d] = hi[d];
    }
  }
}

// Squared distance from p to the box b, and the square of the largest coordinate magnitude of either
__device__ __forceinline__ double md_box_lb2(double px, double py, double pz, const double* __restrict__ b,
                                             double* s2) {
  const double dx = fmax(fmax(b[0] - px, px - b[3]), 0.0);
  const double dy = fmax(fmax(b[1] - py, py - b[4]), 0.0);
  const double dz = fmax(fmax(b[2] - pz, pz - b[5]), 0.0);
  double s = fmax(fmax(fabs(px), fabs(py)), fabs(pz));
#pragma unroll
  for (int k = 0; k < 6; k++) s = fmax(s, fabs(b[k]));
  *s2 = s * s;
  return md_dot(dx, dy, dz, dx, dy, dz);
}

}  // namespace mslam
