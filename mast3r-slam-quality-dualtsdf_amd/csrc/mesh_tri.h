// Triangle helpers shared by the mesh-quality kernels (mesh_distance.hip) and the mesh-alignment kernels
// (mesh_align.hip): the validity rule, the closest point of a triangle by Voronoi regions, the per-tile boxes, the
// distance from a point to a box, the home-tile search md_home_tile, md_scan, the one culled nearest-element scan that
// md_distance_kernel and ma_step_kernel call over triangles (MdTri) and cd_distance_kernel of cloud.hip over points
// (MdPoint), md_walk, the same block-wide walk over groups and tiles keeping what a policy object says (kn_kernel of
// cloud_knn.hip: the k best), the index builder md_build_index, and md_index_arg, the host checks of an index handed
// to an entry point.  Semantics in DESIGN.md "Mesh quality";
// tests/meshdist_numpy.py states the same definitions, operation by operation, in numpy.  Everything is f64 on the f32
// inputs and the build has -ffp-contract=off, so a * b + c below is two roundings, as in numpy.
//
// THE INVARIANT that makes culling exact.  md_dist2(p, f) is |p - q|^2 for a computed point q of face f: a vertex
// itself, a + v (b - a) with a computed 0 <= v <= 1 (both ends of an edge region's division are ordered, and rounding
// is monotone), or a point of the face's plane.  A tile's box holds every vertex of its valid faces exactly (f32
// values in f64), so it holds each face, and q lies within eps of the box, eps a small multiple of the rounding unit
// times the largest coordinate S in play: |p - q| >= lb - eps, where lb is the distance from p to the box.  In the
// interior region an in-plane error of q adds to the distance from the plane, and a foot point wrongly taken for
// interior lies outside the face by no more than the same in-plane error.  The scan keeps
// best = min over scanned faces, and with culling also ub, the value of some real face (so the final minimum is
// <= ub).  A tile is skipped only when, for every point of the wave (scan) or block (staging),
//     lb2 > min(best, ub) * (1 + 2^-20) + 2^-27 * S^2 .
// lb2 itself carries 4 roundings (relative 2^-51, inside the 2^-20), and 2^-27 S^2 >= 2 lb eps for eps = 2^-30 S, a
// closest-point error four million times the rounding unit: the slack is there for sliver triangles, and it costs
// nothing, because a tile worth skipping is centimetres away and 2^-27 S^2 is (1e-4 S)^2.  So every face of a skipped
// tile has md_dist2 > min(best, ub) >= the final minimum: it is neither the minimum nor a tie, and the output is the
// one of the plain ascending scan with its strict `<`, bit for bit.  tests/test_mesh_metrics_gpu.py is the judge.
//
// WITH AN INDEX (mesh_index.hip, DESIGN.md "Mesh index") tile t holds the faces order[128 t + k] instead of the faces
// 128 t + k, so a tile is a compact patch whatever order the caller's faces are in.  `faces` itself is never permuted:
// the staging follows `order` (each entry range-checked first) and keeps the face's ORIGINAL index beside its corners,
// and the scan's rule becomes  d < best || (d == best && f < best_f)  on that original index.  The minimum over a set
// and the lowest index that attains it do not depend on the order of the visit, so the output is still that of the plain
// ascending scan of the caller's mesh, bit for bit, and the argument above goes through unchanged: a tile is skipped
// only when each of its faces is strictly worse than a real face.
// THE GROUP LEVEL.  Above the tiles lie the boxes of groups of 32 consecutive tiles.  Before a group's tiles are
// considered, every lane applies the very same test to the group's box, and when the whole block agrees the group is
// passed over without its 32 barriers.  That is exact by the same proof: the group's box contains each of its tiles'
// boxes, so its lb is no larger and its S no smaller than any tile's, and
//     lb2(group) > min(best, ub) (1 + 2^-20) + 2^-27 S(group)^2
// puts every face of every tile of the group strictly beyond min(best, ub), by the invariant read with the group's box
// in the place of the tile's (it, too, holds every vertex of its valid faces exactly).  tests/test_mesh_index_gpu.py is
// the judge.
#pragma once
#include <math.h>

#include "common.h"

namespace mslam {

constexpr int kMdTile = 128;      // triangles per LDS tile and per box; tests/test_mesh_metrics_gpu.py states it too
constexpr int kMdBlock = 256;     // one point per thread
constexpr int kMdTriDoubles = 10; // a, b, c, valid
constexpr int kMdGroup = 32;      // tiles per group box of a mesh index; tests/test_mesh_index_gpu.py states it too

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

// WHAT A TILE HOLDS is a stateless trait type Prim: MdTri here, MdPoint in cloud.hip.  It names a source struct Src and
// count(src), its elements; kDoubles, the f64 words of a slot, the last of them the valid tag (0: invalid);
// load(src, i, t), which fills slot t from element i (all zeros and false for i >= count or an invalid element); and
// dist2(px, py, pz, t).  Static inline functions, no state, no callables: md_scan<MdTri, .> is the text a scan written
// for triangles alone would be (DESIGN.md "Where the walk lives").
struct MdTri {
  struct Src {
    const float* vert;
    const int32_t* faces;
    int nf, nv;
  };
  static constexpr int kDoubles = kMdTriDoubles;
  static __host__ __device__ __forceinline__ int count(const Src s) { return s.nf; }
  static __device__ __forceinline__ bool load(const Src s, int f, double* t) {
    return md_load_tri(s.vert, s.faces, f, s.nf, s.nv, t);
  }
  static __device__ __forceinline__ double dist2(double px, double py, double pz, const double* t) {
    return md_dist2(px, py, pz, t);
  }
};

// Slot i of the tiles: element i itself, or with an index order[i], range-checked before it is followed (n: none).
__device__ __forceinline__ int md_slot(const int32_t* __restrict__ order, int i, int n) {
  if (!order || i >= n) return i;
  const int f = order[i];
  return (unsigned)f < (unsigned)n ? f : n;
}

// box[6 * tile + ...] = lo.xyz, hi.xyz over the coordinates of the tile's valid elements (a face's three corners, a
// point); (+inf, -inf) for a tile without one.  `order`, when given, names the elements of the tiles (md_slot).
// static: one copy per translation unit that includes this header.
template <class Prim>
static __global__ __launch_bounds__(64) void md_box_kernel(const typename Prim::Src src,
                                                           const int32_t* __restrict__ order,
                                                           double* __restrict__ box) {
  const int tile = blockIdx.x, lane = threadIdx.x, n = Prim::count(src);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int k = lane; k < kMdTile; k += kWave) {
    double t[Prim::kDoubles];
    if (Prim::load(src, md_slot(order, tile * kMdTile + k, n), t)) {
#pragma unroll
      for (int j = 0; j < Prim::kDoubles - 1; j++) {
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

// gbox[6 * group + c]: min (c < 3) or max of component c over the boxes of the group's tiles.  An empty tile's
// (+inf, -inf) changes nothing, and a group of empty tiles keeps it.
static __global__ __launch_bounds__(256) void md_group_kernel(const double* __restrict__ box, int ntiles, int ngroups,
                                                              double* __restrict__ gbox) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * ngroups) return;
  const int g = i / 6, c = i % 6;
  const int t1 = min(ntiles, (g + 1) * kMdGroup);
  double x = c < 3 ? INFINITY : -INFINITY;
  for (int t = g * kMdGroup; t < t1; t++) {
    const double y = box[6 * (size_t)t + c];
    x = c < 3 ? fmin(x, y) : fmax(x, y);
  }
  gbox[i] = x;
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

struct MdNearest {
  double dist2;   // md_dist2 to the nearest valid face, +inf without one
  int face;       // the lowest index of a face at that distance, -1 without one
  int skipped;    // the tiles this lane's wave did not scan
};

// Slot `tid` of `tile` into LDS.  kIndexed: the element is order[128 tile + tid] and the tag of a valid one is 1 + its
// original index (exact in a double), which the scans read back for the tie rule.
template <class Prim, bool kIndexed>
__device__ __forceinline__ void md_stage(const typename Prim::Src src, const int32_t* __restrict__ order, int tile,
                                         int tid, double* s_tri) {
  const int f = md_slot(kIndexed ? order : nullptr, tile * kMdTile + tid, Prim::count(src));
  double* t = s_tri + tid * Prim::kDoubles;
  if (Prim::load(src, f, t) && kIndexed) t[Prim::kDoubles - 1] = (double)f + 1.0;
}

// The home tile of a block: the tile whose box is nearest to q0, the lowest on ties, -1 without a tile or with every
// box at +inf (an infinite coordinate; a NaN one is at distance 0 along its axis).  Wave 0 searches, every thread of
// the block calls and gets the same answer.  s_home: one LDS word.
__device__ __forceinline__ int md_home_tile(double q0x, double q0y, double q0z, const double* __restrict__ box,
                                            int ntiles, int* s_home) {
  const int lane = threadIdx.x & (kWave - 1);
  if (threadIdx.x / kWave == 0) {
    double m = INFINITY, s2;
    int mt = -1;
    for (int t = lane; t < ntiles; t += kWave) {
      const double lb2 = md_box_lb2(q0x, q0y, q0z, box + 6 * (size_t)t, &s2);
      if (lb2 < m) m = lb2, mt = t;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double om = __shfl_down(m, off, kWave);
      const int ot = __shfl_down(mt, off, kWave);
      if (ot >= 0 && (mt < 0 || om < m || (om == m && ot < mt))) m = om, mt = ot;
    }
    if (lane == 0) *s_home = mt;
  }
  __syncthreads();
  return *s_home;
}

// WHAT A LANE KEEPS of the elements it meets is a policy object Acc, a local of the calling kernel: KnList of
// cloud_knn.hip, the k best.  bound() is the value the skip test compares a box with: an element strictly beyond it
// changes nothing the lane keeps.  offer<kIndexed>(d, tag, slot) takes an element at squared distance d from a valid
// slot: `tag` is the slot's last word, 1 + the original index when tagged (md_stage), `slot` its place in the tiles.
// A plain struct with inline members: no callables, nothing captured.  md_scan below is the same walk over one best
// {best, ub, best_f}, written out: as a policy of md_walk it was measured and held for two of its three kernels
// (DESIGN.md "Where the walk lives").

// The `cnt` slots of the staged tile `tile` offered to this lane's acc
template <class Prim, bool kIndexed, class Acc>
__device__ __forceinline__ void md_offer_tile(const double* s_tri, int tile, int cnt, double px, double py, double pz,
                                              Acc& acc) {
  for (int k = 0; k < cnt; k++) {
    const double* t = s_tri + k * Prim::kDoubles;           // one address for the whole wave: an LDS broadcast
    if (t[Prim::kDoubles - 1] != 0.0)
      acc.template offer<kIndexed>(Prim::dist2(px, py, pz, t), t[Prim::kDoubles - 1], tile * kMdTile + k);
  }
}

// THE WALK over groups and tiles, block-wide: the group vote, the tile vote, the staging, and the one
// __syncthreads_and at each vote that is also the barrier before the next staging.  Every thread of the block calls
// it, also one without a point (`has` false): it reaches the same barriers and never keeps a tile in.  `cull` 0 votes
// nothing away.  ntiles: the tiles of src.  `done`: a tile the caller has offered to acc already, passed over here and
// counted neither as scanned nor as skipped, also when its group is voted away (-1: none; with the constant the test
// and the subtraction fold away).  Returns the tiles this lane's wave did not scan.  s_tri: kMdTile * Prim::kDoubles
// doubles of LDS.  Both vote sites are inlined into the calling kernel's own body (DESIGN.md "Where the walk lives").
template <class Prim, bool kIndexed, class Acc>
__device__ __forceinline__ int md_walk(double px, double py, double pz, bool has, const typename Prim::Src src,
                                       int cull, const double* __restrict__ box, const double* __restrict__ gbox,
                                       const int32_t* __restrict__ order, double* s_tri, int ntiles, int done,
                                       Acc& acc) {
  const int tid = threadIdx.x;
  const int nf = Prim::count(src);
  int n_skipped = 0;
  // without an index: one "group" of all tiles, and the loops below are the plain tile loop
  const int ngroups = kIndexed ? (ntiles + kMdGroup - 1) / kMdGroup : 1;
  for (int g = 0; g < ngroups; g++) {
    const int t0 = kIndexed ? g * kMdGroup : 0, t1 = kIndexed ? min(ntiles, t0 + kMdGroup) : ntiles;
    if (kIndexed && cull && gbox) {
      bool lane_skips = !has;
      if (has) {
        double s2;
        const double lb2 = md_box_lb2(px, py, pz, gbox + 6 * (size_t)g, &s2);
        lane_skips = lb2 > acc.bound() * (1.0 + 0x1p-20) + 0x1p-27 * s2;
      }
      // also the barrier between the last tile's reads and the next staging
      if (__syncthreads_and(lane_skips)) {
        n_skipped += t1 - t0 - (done >= t0 && done < t1 ? 1 : 0);
        continue;
      }
    }
    for (int tile = t0; tile < t1; tile++) {
      if (tile == done) continue;                    // the same for the whole block
      bool lane_skips = !has;
      if (cull && has) {
        double s2;
        const double lb2 = md_box_lb2(px, py, pz, box + 6 * (size_t)tile, &s2);
        lane_skips = lb2 > acc.bound() * (1.0 + 0x1p-20) + 0x1p-27 * s2;
      }
      const bool wave_skips = cull && __all(lane_skips);
      // also the barrier between the last tile's reads and this tile's staging
      if (__syncthreads_and(cull && lane_skips)) {
        n_skipped++;
        continue;
      }
      if (tid < kMdTile) md_stage<Prim, kIndexed>(src, order, tile, tid, s_tri);
      __syncthreads();
      if (wave_skips) {
        n_skipped++;
        continue;
      }
      md_offer_tile<Prim, kIndexed>(s_tri, tile, min(kMdTile, nf - tile * kMdTile), px, py, pz, acc);
    }
  }
  return n_skipped;
}

// The nearest valid element (face of the mesh, point of the cloud) to this lane's point p.  Every thread of the block
// calls it, also one without a point (`has` false): it reaches the same barriers and never keeps a tile in.
// `cull` 0 is the plain ascending scan.  With `cull` the two parameters that may differ per lane, neither of which
// changes an output bit, are
//   ub         the lane's starting bound: +inf, or md_dist2(p, any valid face), which is the value of a real face
//              and so all the invariant above asks of it;
//   need_home  the lane has no such face yet.  When some lane of the block with a point says so, the block stages
//              its home tile, the one whose box is nearest to the block's first point q0 (which tile it is changes
//              no output), and those lanes take ub from its faces.
// kIndexed (see the header comment): the tiles follow `order`, ties go to the lowest original index, and `gbox`, when
// given, holds the boxes of the groups of kMdGroup tiles.  Without it `order` and `gbox` are not read.
// s_tri: kMdTile * Prim::kDoubles doubles of LDS; s_home: one LDS word.
template <class Prim, bool kIndexed>
__device__ __forceinline__ MdNearest md_scan(double px, double py, double pz, bool has, double q0x, double q0y,
                                             double q0z, const typename Prim::Src src, int cull,
                                             const double* __restrict__ box, double* s_tri, int* s_home, double ub,
                                             bool need_home, const int32_t* __restrict__ order = nullptr,
                                             const double* __restrict__ gbox = nullptr) {
  const int tid = threadIdx.x;
  const int nf = Prim::count(src);
  const int ntiles = (nf + kMdTile - 1) / kMdTile;

  if (cull && __syncthreads_or(has && need_home)) {
    const int home = md_home_tile(q0x, q0y, q0z, box, ntiles, s_home);
    if (home >= 0) {
      // before the staging branch, not inside `if (need_home)`: formed there, home * kMdTile is merged with the
      // staging's copy of it at the join of a divergent branch, and the loop below runs on vector counters (DESIGN.md
      // "Where the walk lives")
      const int cnt = min(kMdTile, nf - home * kMdTile);
      if (tid < kMdTile) md_stage<Prim, kIndexed>(src, order, home, tid, s_tri);
      __syncthreads();
      if (need_home) {
        for (int k = 0; k < cnt; k++) {
          const double* t = s_tri + k * Prim::kDoubles;
          // fmin: a NaN distance never becomes the bound
          if (t[Prim::kDoubles - 1] != 0.0) ub = fmin(ub, Prim::dist2(px, py, pz, t));
        }
      }
    }
  }

  // md_walk's loops with one best in the place of the policy object (why they are written out: DESIGN.md "Where the
  // walk lives").  Without an index: one "group" of all tiles, and the loops below are the plain tile loop
  double best = INFINITY;
  int best_f = -1, n_skipped = 0;
  const int ngroups = kIndexed ? (ntiles + kMdGroup - 1) / kMdGroup : 1;
  for (int g = 0; g < ngroups; g++) {
    const int t0 = kIndexed ? g * kMdGroup : 0, t1 = kIndexed ? min(ntiles, t0 + kMdGroup) : ntiles;
    if (kIndexed && cull && gbox) {
      bool lane_skips = !has;
      if (has) {
        double s2;
        const double lb2 = md_box_lb2(px, py, pz, gbox + 6 * (size_t)g, &s2);
        lane_skips = lb2 > fmin(best, ub) * (1.0 + 0x1p-20) + 0x1p-27 * s2;
      }
      // also the barrier between the last tile's reads and the next staging
      if (__syncthreads_and(lane_skips)) {
        n_skipped += t1 - t0;
        continue;
      }
    }
    for (int tile = t0; tile < t1; tile++) {
      bool lane_skips = !has;
      if (cull && has) {
        double s2;
        const double lb2 = md_box_lb2(px, py, pz, box + 6 * (size_t)tile, &s2);
        lane_skips = lb2 > fmin(best, ub) * (1.0 + 0x1p-20) + 0x1p-27 * s2;
      }
      const bool wave_skips = cull && __all(lane_skips);
      // also the barrier between the last tile's reads and this tile's staging
      if (__syncthreads_and(cull && lane_skips)) {
        n_skipped++;
        continue;
      }
      if (tid < kMdTile) md_stage<Prim, kIndexed>(src, order, tile, tid, s_tri);
      __syncthreads();
      if (wave_skips) {
        n_skipped++;
        continue;
      }
      const int cnt = min(kMdTile, nf - tile * kMdTile);
      for (int k = 0; k < cnt; k++) {
        const double* t = s_tri + k * Prim::kDoubles;       // one address for the whole wave: an LDS broadcast
        if (t[Prim::kDoubles - 1] != 0.0) {
          const double d = Prim::dist2(px, py, pz, t);
          if (kIndexed) {
            const int f = (int)t[Prim::kDoubles - 1] - 1;
            if (d < best || (d == best && f < best_f)) best = d, best_f = f;
          } else if (d < best) {
            best = d, best_f = tile * kMdTile + k;
          }
        }
      }
    }
  }
  return {best, best_f, n_skipped};
}

// workspace bytes of the boxes of nf faces, and of the per-wave skip counts of n points (four waves per block)
inline size_t md_box_bytes(int nf) { return (size_t)blocks_for(nf, kMdTile) * 6 * sizeof(double); }
inline size_t md_count_bytes(int n) { return (size_t)blocks_for(n, kMdBlock) * 4 * sizeof(int32_t); }

// A mesh index's workspace: the tile boxes, as above but of the tiles in `order`, then the boxes of the groups
inline int md_groups(int nf) { return (int)blocks_for(blocks_for(nf, kMdTile), kMdGroup); }
inline size_t md_index_bytes(int nf) { return md_box_bytes(nf) + (size_t)md_groups(nf) * 6 * sizeof(double); }
inline const double* md_index_gbox(const void* index, int nf) {
  return (const double*)((const char*)index + md_box_bytes(nf));
}

// The boxes of the tiles of the > 0 elements of src -> box; `order` null: the tiles of the caller's element order
template <class Prim>
inline void md_launch_boxes(const typename Prim::Src src, const int32_t* order, double* box, hipStream_t stream) {
  hipLaunchKernelGGL(md_box_kernel<Prim>, dim3(blocks_for(Prim::count(src), kMdTile)), dim3(kWave), 0, stream, src,
                     order, box);
}

// The error of entry point `what` whose `thing` ("workspace", "index") is too small
inline int md_too_small(const char* what, const char* thing, size_t have, size_t need) {
  set_error("%s: %s of %zu bytes, %zu needed", what, thing, have, need);
  return MSLAM_ENOMEM;
}

// The `levels` of entry point `what`; an entry point that tests it ahead of its early return calls this by itself
inline int md_levels_arg(const char* what, int levels) {
  if (levels == 1 || levels == 2) return MSLAM_OK;
  set_error("%s: levels must be 1 (tiles) or 2 (tiles and groups)", what);
  return MSLAM_EINVAL;
}

// What the scans take of an index: all null for the plain scan; gbox null at `levels` 1
struct MdIndexArg {
  const int32_t* order;
  const double *box, *gbox;
};

// The index argument (order, index, index_bytes, levels) of entry point `what` over a target of n elements -> *arg.
// The plain scan (no order, or no element to index) asks nothing of `index`; an order needs its index, large enough.
// Every entry point calls it where its own checks stand, so which degenerate calls it refuses is the entry point's
// (tests/test_index_arg_gpu.py has the table).  An entry point without a `levels` parameter passes 2.
inline int md_index_arg(const char* what, int n, const int32_t* order, const void* index, size_t index_bytes,
                        int levels, MdIndexArg* arg) {
  *arg = {nullptr, nullptr, nullptr};
  if (int rc = md_levels_arg(what, levels)) return rc;
  if (!order || n == 0) return MSLAM_OK;
  if (!index) {
    set_error("%s: an order needs its index", what);
    return MSLAM_EINVAL;
  }
  if (index_bytes < md_index_bytes(n)) return md_too_small(what, "index", index_bytes, md_index_bytes(n));
  *arg = {order, (const double*)index, levels == 2 ? md_index_gbox(index, n) : nullptr};
  return MSLAM_OK;
}

// MSLAM_LAUNCH_CHECK for an entry point whose name is known at run time: the status to return after the launches
inline int md_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) set_error("%s launch: %s", what, hipGetErrorString(e));
  return e == hipSuccess ? MSLAM_OK : MSLAM_EHIP;
}

// An index's workspace of entry point `what` filled for the > 0 elements of src in `order`: the size check, the tile
// boxes, the group boxes above them, the launch check.
template <class Prim>
inline int md_build_index(const typename Prim::Src src, const int32_t* order, void* workspace, size_t workspace_bytes,
                          const char* what, hipStream_t stream) {
  const int n = Prim::count(src), ntiles = (int)blocks_for(n, kMdTile), ngroups = md_groups(n);
  if (workspace_bytes < md_index_bytes(n)) return md_too_small(what, "workspace", workspace_bytes, md_index_bytes(n));
  double* box = (double*)workspace;
  md_launch_boxes<Prim>(src, order, box, stream);
  hipLaunchKernelGGL(md_group_kernel, dim3(blocks_for(6 * ngroups, 256)), dim3(256), 0, stream, (const double*)box,
                     ntiles, ngroups, box + 6 * (size_t)ntiles);
  return md_launched(what);
}

}  // namespace mslam
