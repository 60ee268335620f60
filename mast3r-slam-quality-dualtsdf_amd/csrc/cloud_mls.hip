// Cloud smoothing: one step of the moving-least-squares projection in its plane form (Levin; Alexa et al.): every query
// moves onto the weighted least-squares plane of the cloud within a radius of it.  Semantics in DESIGN.md "Cloud
// smoothing"; tests/cloud_mls_numpy.py states the same definition, operation by operation, in numpy.  Everything is
// f64 on the f32 inputs in one fixed order and the build has -ffp-contract=off, so a * b + c below is two roundings.
//
// THE DEFINITION.  For query p and a valid point q of the cloud, d2 is MdPoint::dist2, the sum cloud_distance uses.  q
// JOINS when d2 <= h2 and, in the gated form, its normal passes the gate.  inv = 1 / h2 once; u = 1 - d2 inv, w = u u,
// so a neighbour at exactly d2 == h2 joins with weight 0: it counts and adds nothing.  With r = q - p in f64, per
// joining neighbour in the order the walk offers them:
//     S0 += w;
//     wx = w rx;  S1x += wx;  Sxx += wx rx;  Sxy += wx ry;  Sxz += wx rz;
//     wy = w ry;  S1y += wy;  Syy += wy ry;  Syz += wy rz;
//     wz = w rz;  S1z += wz;  Szz += wz rz;
//     count += 1.
// After the walk m = S1 / S0 and C = S2 / S0 - m m^T entry by entry (zeros unless S0 > 0: a neighbourhood that lies on
// the rim of the ball altogether has no plane), kn_jacobi3 on C, and the tail of kn_normals_kernel of cloud_knn.hip,
// restated in ml_finish below: the column of the smallest eigenvalue, normalised, its largest component made positive;
// degenerate when count < 3 or lmid <= 2^-40 lmax; the curvature fmax(lmin, 0) / ((l0 + l1) + l2).  Then
// t = (nx mx + ny my) + nz mz and out = (float)(p + (strength t) n) per component; t n does not depend on n's sign.
// A query STAYS - out_points holds the input's f32 bits, the normal is (0, 0, 0), the curvature NaN - when it has a
// non-finite coordinate, when count < min_points, when count < 3 or when it is degenerate.
//
// THE ORDER OF THE SUM IS THE WALK'S: ascending point index when `order` is NULL, ascending slot - order[0], order[1],
// ... - with an index.  An f64 sum depends on its order, so unlike the integer count of cloud_cluster.hip this entry
// has one statement per order, and the plain and the indexed form differ by rounding.  Levels 1 and 2 give the same
// bytes as each other and as the unculled walk in the same order, by "WHY THE CONSTANT BOUND IS EXACT" at the head of
// cloud_cluster.hip read word for word: the policy's bound() is the constant h2 (-inf for a lane without a query), a
// skipped tile or group holds only points with d2 > h2 strictly, those do not join, and leaving out terms that are not
// there changes no sum.
//
// THE GATE.  With query_normals and point_normals a neighbour j also has to pass
// fabs((ax bx + ay by) + az bz) >= cos_gate, a the query's normal and b point_normals[j] in f64.  A query whose normal
// is (0, 0, 0) or non-finite is not gated.  A neighbour's non-finite normal is staged as (0, 0, 0), so it fails every
// cos_gate > 0, as a zero one does.  The absolute value makes the sign of either normal immaterial.  The gated kernel
// stages tiles of MdPointN - x y z, nx ny nz, tag; 7 KB of LDS - over the same position-only boxes of the CloudIndex;
// the ungated kernel stages MdPoint and never reads a normal.
//
// THE NEIGHBOUR'S COORDINATES.  md_offer_tile hands offer() the squared distance, the tag and the slot; the policy
// holds the pointer to the staged tile and reads slot & (kMdTile - 1) of it: one LDS address per wave, a broadcast,
// and the very words dist2 was computed from.
//
// One query per thread, kMdBlock threads, ten f64 accumulators per lane.  No atomics, no waiting between blocks, every
// loop bounded by a tile count or the 16 sweeps of the Jacobi.  out_points may alias neither queries nor points: other
// blocks still read them.
#include "cloud_point.h"
#include "jacobi3.h"

namespace mslam {

constexpr int kMlMoments = MSLAM_CLOUD_MLS_MOMENTS;

// A tile slot of the gated form: x y z, the normal, and the tag LAST, where md_offer_tile and md_stage look for it.
// The boxes and the index are MdPoint's: only md_stage and md_offer_tile are instantiated with this trait.
struct MdPointN {
  struct Src {
    const float* points;
    const float* normals;
    int n;
  };
  static constexpr int kDoubles = 7;
  static __host__ __device__ __forceinline__ int count(const Src s) { return s.n; }
  static __device__ __forceinline__ bool load(const Src s, int j, double* p) {
#pragma unroll
    for (int k = 0; k < kDoubles; k++) p[k] = 0.0;
    if (j >= s.n) return false;
    const float x = s.points[3 * (size_t)j], y = s.points[3 * (size_t)j + 1], z = s.points[3 * (size_t)j + 2];
    if (!cd_finite(x, y, z)) return false;
    const float a = s.normals[3 * (size_t)j], b = s.normals[3 * (size_t)j + 1], c = s.normals[3 * (size_t)j + 2];
    p[0] = (double)x, p[1] = (double)y, p[2] = (double)z, p[6] = (double)j + 1.0;
    if (cd_finite(a, b, c)) p[3] = (double)a, p[4] = (double)b, p[5] = (double)c;
    return true;
  }
  static __device__ __forceinline__ double dist2(double px, double py, double pz, const double* q) {
    return MdPoint::dist2(px, py, pz, q);
  }
};

// What a lane keeps (the policy md_walk asks for): h2 (-inf for a lane without a query), the query, its normal when
// gated, the staged tile, and the ten sums with the count
template <class Prim>
struct MlSums {
  static constexpr bool kGated = Prim::kDoubles == MdPointN::kDoubles;
  double h2, inv, px, py, pz;
  double ax, ay, az, cos_gate;
  bool gated;
  const double* tile;
  double s0, s1x, s1y, s1z, sxx, sxy, sxz, syy, syz, szz;
  int count;
  __device__ __forceinline__ double bound() const { return h2; }
  template <bool kIndexed>
  __device__ __forceinline__ void offer(double d, double, int slot) {
    if (!(d <= h2)) return;
    const double* q = tile + (slot & (kMdTile - 1)) * Prim::kDoubles;
    if (kGated && gated) {
      if (!(fabs((ax * q[3] + ay * q[4]) + az * q[5]) >= cos_gate)) return;
    }
    const double u = 1.0 - d * inv, w = u * u;
    const double rx = q[0] - px, ry = q[1] - py, rz = q[2] - pz;
    s0 += w;
    const double wx = w * rx;
    s1x += wx, sxx += wx * rx, sxy += wx * ry, sxz += wx * rz;
    const double wy = w * ry;
    s1y += wy, syy += wy * ry, syz += wy * rz;
    const double wz = w * rz;
    s1z += wz, szz += wz * rz;
    count += 1;
  }
};

// From the sums to the plane: the moments, the Jacobi and the tail of kn_normals_kernel (cloud_knn.hip) restated for the
// sign rule without a viewpoint - the same operations in the same order, so that kernel's text stays as it is.
// Returns whether the query moves; n: the signed unit normal, *t the signed distance to the plane along it (zeros when
// it stays), l: the diagonal after the sweeps, *curv the curvature (NaN when it stays).
template <class Prim>
__device__ __forceinline__ bool ml_finish(const MlSums<Prim>& a, bool has, int min_points, double* l, double* n,
                                          double* t, float* curv) {
  double mx = 0.0, my = 0.0, mz = 0.0, xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  if (a.s0 > 0.0) {
    mx = a.s1x / a.s0, my = a.s1y / a.s0, mz = a.s1z / a.s0;
    xx = a.sxx / a.s0 - mx * mx, xy = a.sxy / a.s0 - mx * my, xz = a.sxz / a.s0 - mx * mz;
    yy = a.syy / a.s0 - my * my, yz = a.syz / a.s0 - my * mz, zz = a.szz / a.s0 - mz * mz;
  }
  double A[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  kn_jacobi3(A, V);
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  int lo = 0;
  double lmin = l0;
  if (l1 < lmin) lo = 1, lmin = l1;
  if (l2 < lmin) lo = 2, lmin = l2;
  const double lmax = fmax(fmax(l0, l1), l2);
  const double lmid = fmax(fmin(l0, l1), fmin(fmax(l0, l1), l2));
  const bool degenerate = a.count < 3 || lmid <= 0x1p-40 * lmax;
  double nx = lo == 0 ? V[0][0] : lo == 1 ? V[0][1] : V[0][2];
  double ny = lo == 0 ? V[1][0] : lo == 1 ? V[1][1] : V[1][2];
  double nz = lo == 0 ? V[2][0] : lo == 1 ? V[2][1] : V[2][2];
  double n2 = 0.0;
  n2 += nx * nx, n2 += ny * ny, n2 += nz * nz;
  const double inv = 1.0 / sqrt(n2);
  nx = nx * inv, ny = ny * inv, nz = nz * inv;
  double big = nx;
  if (fabs(ny) > fabs(big)) big = ny;
  if (fabs(nz) > fabs(big)) big = nz;
  if (big < 0.0) nx = -nx, ny = -ny, nz = -nz;
  const bool moves = has && a.count >= min_points && !degenerate;
  l[0] = l0, l[1] = l1, l[2] = l2;
  n[0] = moves ? nx : 0.0, n[1] = moves ? ny : 0.0, n[2] = moves ? nz : 0.0;
  *t = moves ? (nx * mx + ny * my) + nz * mz : 0.0;
  *curv = moves ? (float)(fmax(lmin, 0.0) / ((l0 + l1) + l2)) : NAN;
  return moves;
}

template <class Prim, bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void ml_step_kernel(
    const float* __restrict__ queries, int n, const typename Prim::Src src, double h2, int min_points, double strength,
    const float* __restrict__ query_normals, double cos_gate, const int32_t* __restrict__ order,
    const double* __restrict__ box, const double* __restrict__ gbox, int32_t* __restrict__ skipped,
    float* __restrict__ out_points, float* __restrict__ out_normals, float* __restrict__ out_curvature,
    int32_t* __restrict__ out_count, double* __restrict__ moments) {
  __shared__ double s_pts[kMdTile * Prim::kDoubles];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kMdBlock + tid;
  const bool in_range = i < (size_t)n;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (in_range) qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  const bool has = in_range && cd_finite(qx, qy, qz);
  const double px = (double)qx, py = (double)qy, pz = (double)qz;
  const int num_points = Prim::count(src);
  const int ntiles = (num_points + kMdTile - 1) / kMdTile;

  MlSums<Prim> acc;
  acc.h2 = has ? h2 : -INFINITY, acc.inv = 1.0 / h2, acc.px = px, acc.py = py, acc.pz = pz;
  acc.ax = acc.ay = acc.az = 0.0, acc.cos_gate = cos_gate, acc.gated = false;
  if (MlSums<Prim>::kGated && has) {
    const float a = query_normals[3 * i], b = query_normals[3 * i + 1], c = query_normals[3 * i + 2];
    if (cd_finite(a, b, c) && (a != 0.0f || b != 0.0f || c != 0.0f))
      acc.ax = (double)a, acc.ay = (double)b, acc.az = (double)c, acc.gated = true;
  }
  acc.tile = s_pts;
  acc.s0 = acc.s1x = acc.s1y = acc.s1z = acc.sxx = acc.sxy = acc.sxz = acc.syy = acc.syz = acc.szz = 0.0;
  acc.count = 0;
  const int n_skipped =
      md_walk<Prim, kIndexed>(px, py, pz, has, src, kIndexed, box, gbox, order, s_pts, ntiles, -1, acc);

  if (in_range) {
    double l[3], nrm[3], t;
    float curv;
    const bool moves = ml_finish<Prim>(acc, has, min_points, l, nrm, &t, &curv);
    const double st = strength * t;
    out_points[3 * i] = moves ? (float)(px + st * nrm[0]) : qx;
    out_points[3 * i + 1] = moves ? (float)(py + st * nrm[1]) : qy;
    out_points[3 * i + 2] = moves ? (float)(pz + st * nrm[2]) : qz;
    out_normals[3 * i] = (float)nrm[0], out_normals[3 * i + 1] = (float)nrm[1], out_normals[3 * i + 2] = (float)nrm[2];
    out_curvature[i] = curv;
    out_count[i] = acc.count;
    if (moments) {
      double* mom = moments + kMlMoments * i;
      mom[0] = acc.s0, mom[1] = acc.s1x, mom[2] = acc.s1y, mom[3] = acc.s1z;
      mom[4] = acc.sxx, mom[5] = acc.sxy, mom[6] = acc.sxz, mom[7] = acc.syy, mom[8] = acc.syz, mom[9] = acc.szz;
      mom[10] = l[0], mom[11] = l[1], mom[12] = l[2];
      mom[13] = nrm[0], mom[14] = nrm[1], mom[15] = nrm[2], mom[16] = t, mom[17] = 0.0;
    }
  }
  if (skipped && (tid & (kWave - 1)) == 0) skipped[4 * (size_t)blockIdx.x + tid / kWave] = n_skipped;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_cloud_mls_step(const float* queries, int n, const float* points, int num_points, double h2,
                                    int min_points, double strength, const float* query_normals,
                                    const float* point_normals, double cos_gate, const int32_t* order,
                                    const void* index, size_t index_bytes, int levels, int32_t* skip_counts,
                                    float* out_points, float* out_normals, float* out_curvature, int32_t* out_count,
                                    double* moments, void* stream) {
  MSLAM_REQUIRE(n >= 0 && num_points >= 0, "cloud_mls_step: negative size");
  MSLAM_REQUIRE(h2 > 0.0 && isfinite(h2), "cloud_mls_step: h2 must be finite and > 0, got %g", h2);
  MSLAM_REQUIRE(min_points >= 1, "cloud_mls_step: min_points must be >= 1, got %d", min_points);
  MSLAM_REQUIRE(strength >= 0.0 && strength <= 1.0, "cloud_mls_step: strength must be in [0, 1], got %g", strength);
  // both or neither; NULL may stand for the array that has no rows
  MSLAM_REQUIRE((query_normals != nullptr) == (point_normals != nullptr) || (query_normals ? num_points == 0 : n == 0),
                "cloud_mls_step: query_normals and point_normals go together");
  MSLAM_REQUIRE(!(query_normals || point_normals) || (cos_gate >= 0.0 && cos_gate <= 1.0),
                "cloud_mls_step: cos_gate must be in [0, 1], got %g", cos_gate);
  MdIndexArg ix;
  if (int rc = md_index_arg("cloud_mls_step", num_points, order, index, index_bytes, levels, &ix)) return rc;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(queries && out_points && out_normals && out_curvature && out_count, "cloud_mls_step: null pointer");
  MSLAM_REQUIRE(num_points == 0 || points, "cloud_mls_step: null pointer");
  const dim3 grid(blocks_for(n, kMdBlock)), block(kMdBlock);
  if (query_normals) {
    const MdPointN::Src src = {points, point_normals, num_points};
    const auto kernel = ix.order ? ml_step_kernel<MdPointN, true> : ml_step_kernel<MdPointN, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, queries, n, src, h2, min_points, strength,
                       query_normals, cos_gate, ix.order, ix.box, ix.gbox, skip_counts, out_points, out_normals,
                       out_curvature, out_count, moments);
  } else {
    const MdPoint::Src src = {points, num_points};
    const auto kernel = ix.order ? ml_step_kernel<MdPoint, true> : ml_step_kernel<MdPoint, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, queries, n, src, h2, min_points, strength,
                       query_normals, cos_gate, ix.order, ix.box, ix.gbox, skip_counts, out_points, out_normals,
                       out_curvature, out_count, moments);
  }
  MSLAM_LAUNCH_CHECK("cloud_mls_step");
  return MSLAM_OK;
}
