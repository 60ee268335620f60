// Ray casting against a triangle mesh: depth / normal views of any mesh and the occlusion test of observed_points.
// Semantics in DESIGN.md "Mesh ray casting"; tests/raycast_numpy.py states the same definitions, operation by
// operation, in numpy.  Everything is f64 on the f32 inputs and the build has -ffp-contract=off, so a * b - c below is
// two roundings, as in numpy.
//
// The intersection is the two-sided watertight test of Woop, Benthin and Wald (2013): the ray's largest axis kz becomes
// the depth axis, the vertices are translated to the ray's origin and sheared so that the ray runs along +z, and the
// three edge functions U, V, W of the sheared x, y decide.  The sheared coordinates of a vertex depend on the ray and the
// vertex only, and x y' - y x' is the exact negative of y x' - x y', so two faces that share an edge see opposite signs
// of its edge function and a ray through a shared edge or vertex hits at least one of them.
//
// Structure: md_scan's.  One ray per thread, 8x8 pixels per wave (h = 1: 256 consecutive rays per block), the faces
// staged through LDS in the 128-face tiles of mesh_tri.h in index order, every lane reading one address (a broadcast).
// When all rays of a wave share kz and the sign of d[kz] - the rule for a pinhole view - the axis permutation is a
// compile-time constant of the tile loop; otherwise each lane selects its axes.  Both run the same operations.
//
// CULLING (rc_box_skips).  For a vertex v of a tile's valid face, every step of its sheared coordinates is a monotone
// function of one input: q = v - o, p = S q[kz], x = q[kx] - p, z = Sz q[kz], and rounding keeps order.  The tile's box
// holds v exactly, so the same operations on the box's ends give intervals [xl, xh], [yl, yh], [zl, zh] that hold the
// COMPUTED x, y, z of every such vertex, with no margin needed.  Then
//   depth    a hit has U, V, W of one sign, so t = ((U Az + V Bz) + W Cz) / det is a convex combination of the three z
//            up to 8 roundings relative to the largest |z| (no cancellation in det): zl - eps <= t <= zh + eps for
//            eps = 2^-40 max(|zl|, |zh|), 2^10 times the bound.  A tile with zl - eps > min(best, far) or
//            zh + eps < near holds no face that could replace `best` (strict: a tie is not skipped).
//   lateral  the sign of a computed edge function is the exact sign of x y' - y x' on the computed coordinates, or zero.
//            When the rectangle [xl, xh] x [yl, yh] excludes the origin strictly, the exact U, V, W of a face in it have
//            mixed signs (U Ax + V Bx + W Cx = 0), so the computed ones pass the sign test only if every one of the
//            minority sign rounds to zero: the three sheared vertices are collinear with the origin to the last bit, a
//            face seen edge-on whose "hit" is rounding noise.  DESIGN.md states this exception; it is the one case in
//            which the culled scan could differ from the plain one.
//
// WITH AN INDEX (mesh_index.hip; mesh_tri.h's header comment) the tiles follow `order`, a tie on t goes to the lowest
// ORIGINAL face index, so the output is the plain ascending cast's whatever the order of the visit, and the same
// rc_box_skips is put to the box of each group of 32 tiles before its tiles are considered.  Both arguments above hold
// for ANY box that holds the vertices - the shear is monotone per input, and a group's box holds every tile's - so a
// skipped group holds no face that could replace `best`.  The lateral test's edge-on exception is the same one, for
// the same faces, no wider: a face whose three sheared vertices are collinear with the origin to the last bit.
// Nothing is written except the outputs (and, when asked for, the per-wave skip counts).
#include "mesh_tri.h"
#include "view.h"

namespace mslam {

struct RcRay {
  double o[3], d[3];
  double po[3];          // o[kx], o[ky], o[kz]
  double sx, sy, sz;
  int kx, ky, kz;
  int perm;              // 2 kz + (d[kz] < 0), -1 for a lane without a castable ray
};

static_assert(kMdBlock == kViewBlock, "the cast's blocks are the view's");

// The faces of the staged tile against this lane's ray; KX, KY, KZ >= 0: the wave's common permutation, -1: the lane's.
// kIndexed: the face's original index comes from its slot (md_stage) and a tie on t goes to the lowest.
template <bool kIndexed, int KX, int KY, int KZ>
__device__ __forceinline__ void rc_scan_tile(const RcRay& r, const double* s_tri, int cnt, int f0, double near,
                                             double far, double& best, int& best_f) {
  for (int k = 0; k < cnt; k++) {
    const double* t = s_tri + k * kMdTriDoubles;         // one address for the whole wave: an LDS broadcast
    if (t[9] == 0.0) continue;
    double x[3], y[3], z[3];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const double q0 = t[3 * v] - r.o[0], q1 = t[3 * v + 1] - r.o[1], q2 = t[3 * v + 2] - r.o[2];
      const double qx = rc_pick<KX>(q0, q1, q2, r.kx), qy = rc_pick<KY>(q0, q1, q2, r.ky);
      const double qz = rc_pick<KZ>(q0, q1, q2, r.kz);
      x[v] = qx - r.sx * qz;
      y[v] = qy - r.sy * qz;
      z[v] = r.sz * qz;
    }
    const double U = x[2] * y[1] - y[2] * x[1];
    const double V = x[0] * y[2] - y[0] * x[2];
    const double W = x[1] * y[0] - y[1] * x[0];
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) continue;
    const double det = (U + V) + W;
    if (det == 0.0) continue;
    const double tt = ((U * z[0] + V * z[1]) + W * z[2]) / det;
    if (!(tt >= near && tt <= far)) continue;
    if (kIndexed) {
      const int f = (int)t[9] - 1;
      if (tt < best || (tt == best && f < best_f)) best = tt, best_f = f;
    } else if (tt < best) {
      best = tt, best_f = f0 + k;
    }
  }
}

// true when no face of the tile with box b can replace the lane's best (see CULLING above); lim = min(best, far).
// Every comparison is false on a NaN, so a box that cannot be judged is kept.
__device__ __forceinline__ bool rc_box_skips(const RcRay& r, const double* __restrict__ b, double near, double lim) {
  const double qxl = rc_pick<-1>(b[0], b[1], b[2], r.kx) - r.po[0], qxh = rc_pick<-1>(b[3], b[4], b[5], r.kx) - r.po[0];
  const double qyl = rc_pick<-1>(b[0], b[1], b[2], r.ky) - r.po[1], qyh = rc_pick<-1>(b[3], b[4], b[5], r.ky) - r.po[1];
  const double qzl = rc_pick<-1>(b[0], b[1], b[2], r.kz) - r.po[2], qzh = rc_pick<-1>(b[3], b[4], b[5], r.kz) - r.po[2];
  const double pxa = r.sx * qzl, pxb = r.sx * qzh, pya = r.sy * qzl, pyb = r.sy * qzh;
  const double xl = qxl - fmax(pxa, pxb), xh = qxh - fmin(pxa, pxb);
  const double yl = qyl - fmax(pya, pyb), yh = qyh - fmin(pya, pyb);
  const double za = r.sz * qzl, zb = r.sz * qzh;
  const double zl = fmin(za, zb), zh = fmax(za, zb);
  const double eps = 0x1p-40 * fmax(fabs(zl), fabs(zh));
  return xl > 0.0 || xh < 0.0 || yl > 0.0 || yh < 0.0 || zl - eps > lim || zh + eps < near;
}

// kIndexed: the tiles follow `order`, `gbox` (may be null) holds the group boxes, and `skipped` (may be null) receives,
// per wave, the tiles it did not scan -> skipped[4 * block + wave]; without it none of the three is read or written.
template <bool kIndexed>
__global__ __launch_bounds__(kMdBlock) void rc_kernel(const float* __restrict__ rays, int h, int w,
                                                      const float* __restrict__ pose8,
                                                      const float* __restrict__ vert,
                                                      const int32_t* __restrict__ faces, int nf, int nv, double near,
                                                      double far, int cull, const double* __restrict__ box,
                                                      const int32_t* __restrict__ order,
                                                      const double* __restrict__ gbox, int32_t* __restrict__ skipped,
                                                      float* __restrict__ range, float* __restrict__ normal,
                                                      uint8_t* __restrict__ hit, int32_t* __restrict__ face,
                                                      double* __restrict__ t64) {
  __shared__ double s_tri[kMdTile * kMdTriDoubles];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  long long px;
  int py;
  view_pixel(h, px, py);
  const bool has = px < w && py < h;
  const size_t i = (size_t)py * w + (size_t)px;

  RcRay r;
  r.perm = -1;
  r.kx = r.ky = r.kz = 0;
  r.sx = r.sy = r.sz = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) r.o[a] = r.d[a] = r.po[a] = 0.0;
  if (has) {
    view_ray(rays, i, pose8, r.o, r.d);
    const ViewShear s = view_shear(r.d);
    if (s.perm >= 0) {                    // a zero or non-finite direction misses
      r.kx = s.kx, r.ky = s.ky, r.kz = s.kz;
      r.sx = s.sx, r.sy = s.sy, r.sz = s.sz;
      r.po[0] = rc_pick<-1>(r.o[0], r.o[1], r.o[2], s.kx);
      r.po[1] = rc_pick<-1>(r.o[0], r.o[1], r.o[2], s.ky);
      r.po[2] = rc_pick<-1>(r.o[0], r.o[1], r.o[2], s.kz);
      r.perm = s.perm;
    }
  }
  const bool casts = r.perm >= 0;
  // the wave's common permutation, or -1 when its rays disagree (or none casts)
  const unsigned long long active = __ballot(casts);
  int wave_perm = -1;
  if (active) {
    wave_perm = __shfl(r.perm, __ffsll((long long)active) - 1, kWave);
    if (!__all(!casts || r.perm == wave_perm)) wave_perm = -1;
  }

  const int ntiles = (nf + kMdTile - 1) / kMdTile;
  double best = INFINITY;
  int best_f = -1, n_skipped = 0;
  // without an index: one "group" of all tiles, and the loops below are the plain tile loop
  const int ngroups = kIndexed ? (ntiles + kMdGroup - 1) / kMdGroup : 1;
  for (int g = 0; g < ngroups; g++) {
    const int t0 = kIndexed ? g * kMdGroup : 0, t1 = kIndexed ? min(ntiles, t0 + kMdGroup) : ntiles;
    if (kIndexed && cull && gbox) {
      // the same test on the group's box; also the barrier between the last tile's reads and the next staging
      const bool lane_skips = !casts || rc_box_skips(r, gbox + 6 * (size_t)g, near, fmin(best, far));
      if (__syncthreads_and(lane_skips)) {
        n_skipped += t1 - t0;
        continue;
      }
    }
    for (int tile = t0; tile < t1; tile++) {
      bool lane_skips = !casts;
      if (cull && casts) lane_skips = rc_box_skips(r, box + 6 * (size_t)tile, near, fmin(best, far));
      const bool wave_skips = __all(lane_skips);
      // also the barrier between the last tile's reads and this tile's staging
      if (__syncthreads_and(lane_skips)) {
        n_skipped++;
        continue;
      }
      if (tid < kMdTile) md_stage<MdTri, kIndexed>({vert, faces, nf, nv}, order, tile, tid, s_tri);
      __syncthreads();
      if (wave_skips) {
        n_skipped++;
        continue;
      }
      const int cnt = min(kMdTile, nf - tile * kMdTile), f0 = tile * kMdTile;
      switch (wave_perm) {
        case 0: rc_scan_tile<kIndexed, 1, 2, 0>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        case 1: rc_scan_tile<kIndexed, 2, 1, 0>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        case 2: rc_scan_tile<kIndexed, 2, 0, 1>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        case 3: rc_scan_tile<kIndexed, 0, 2, 1>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        case 4: rc_scan_tile<kIndexed, 0, 1, 2>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        case 5: rc_scan_tile<kIndexed, 1, 0, 2>(r, s_tri, cnt, f0, near, far, best, best_f); break;
        default:
          if (casts) rc_scan_tile<kIndexed, -1, -1, -1>(r, s_tri, cnt, f0, near, far, best, best_f);
      }
    }
  }
  if (kIndexed && skipped && lane == 0)
    skipped[4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + wave] = n_skipped;
  if (!has) return;
  if (!casts) best = INFINITY, best_f = -1;      // such a lane ran along in its wave's scan; its ray misses

  float out_range = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f};
  if (best_f >= 0) {
    double t[kMdTriDoubles];
    md_load_tri(vert, faces, best_f, nf, nv, t);
    const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
    const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const double len = sqrt(md_dot(nx, ny, nz, nx, ny, nz));
    const double sign = md_dot(nx, ny, nz, r.d[0], r.d[1], r.d[2]) > 0.0 ? -1.0 : 1.0;    // towards the origin
    out_n[0] = (float)(sign * (nx / len));
    out_n[1] = (float)(sign * (ny / len));
    out_n[2] = (float)(sign * (nz / len));
    out_range = (float)(best / (double)pose8[7]);
  }
  range[i] = out_range;
  normal[3 * i] = out_n[0], normal[3 * i + 1] = out_n[1], normal[3 * i + 2] = out_n[2];
  hit[i] = best_f >= 0 ? 1 : 0;
  if (face) face[i] = best_f;
  if (t64) t64[i] = best;
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_mesh_raycast_workspace_bytes(int num_faces) {
  return num_faces > 0 ? md_box_bytes(num_faces) : 0;
}

extern "C" int mslam_mesh_raycast_boxes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_raycast_boxes: negative size");
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && workspace && (vertices || num_vertices == 0), "mesh_raycast_boxes: null pointer");
  if (workspace_bytes < md_box_bytes(num_faces))
    return md_too_small("mesh_raycast_boxes", "workspace", workspace_bytes, md_box_bytes(num_faces));
  md_launch_boxes<MdTri>({vertices, faces, num_faces, num_vertices}, nullptr, (double*)workspace, (hipStream_t)stream);
  MSLAM_LAUNCH_CHECK("mesh_raycast_boxes");
  return MSLAM_OK;
}

// Both casts after their argument checks.  Plain: culled (`cull`) by the boxes `box` of mslam_mesh_raycast_boxes.
// `indexed`: the tiles follow `order`, `box` is a mesh index, its groups are used at `levels` 2, and `skip_counts` (may
// be null) receives the per-wave counts.
static int rc_cast_impl(const char* what, bool indexed, const float* rays, int h, int w, const float* pose8,
                        const float* vertices, const int32_t* faces, int num_faces, int num_vertices, double near,
                        double far, int cull, const void* box, size_t box_bytes, const int32_t* order, int levels,
                        int32_t* skip_counts, float* range, float* normal, uint8_t* hit, int32_t* face, double* t64,
                        void* stream) {
  MdIndexArg ix = {nullptr, (const double*)box, nullptr};
  if (indexed) {
    if (int rc = md_index_arg(what, num_faces, order, box, box_bytes, levels, &ix)) return rc;
  } else if (cull && box_bytes < md_box_bytes(num_faces)) {
    return md_too_small(what, "workspace", box_bytes, md_box_bytes(num_faces));
  }
  hipLaunchKernelGGL(indexed ? rc_kernel<true> : rc_kernel<false>, view_grid(h, w), dim3(kMdBlock), 0,
                     (hipStream_t)stream, rays, h, w, pose8, vertices, faces, num_faces, num_vertices, near, far, cull,
                     ix.box, ix.order, ix.gbox, skip_counts, range, normal, hit, face, t64);
  return md_launched(what);
}

extern "C" int mslam_mesh_raycast(const float* rays, int h, int w, const float* pose8, const float* vertices,
                                  const int32_t* faces, int num_faces, int num_vertices, double near, double far,
                                  int skip, const void* workspace, size_t workspace_bytes, float* range, float* normal,
                                  uint8_t* hit, int32_t* face, double* t64, void* stream) {
  if (int rc = view_check("mesh_raycast", 1, h, w, nullptr, near, far, false)) return rc;
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_raycast: negative size");
  if (h == 0 || w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(rays && pose8 && range && normal && hit, "mesh_raycast: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && (vertices || num_vertices == 0)), "mesh_raycast: null pointer");
  const int cull = skip && num_faces > 0;
  MSLAM_REQUIRE(!cull || workspace, "mesh_raycast: the culled scan needs the workspace of mesh_raycast_boxes");
  return rc_cast_impl("mesh_raycast", false, rays, h, w, pose8, vertices, faces, num_faces, num_vertices, near, far,
                      cull, workspace, workspace_bytes, nullptr, 0, nullptr, range, normal, hit, face, t64, stream);
}

extern "C" int mslam_mesh_raycast_blocks(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  const dim3 grid = view_grid(h, w);
  return (int)(grid.x * grid.y);
}

extern "C" int mslam_mesh_raycast_indexed(const float* rays, int h, int w, const float* pose8, const float* vertices,
                                          const int32_t* faces, int num_faces, int num_vertices, double near,
                                          double far, const int32_t* order, const void* index, size_t index_bytes,
                                          int levels, int32_t* skip_counts, float* range, float* normal, uint8_t* hit,
                                          int32_t* face, double* t64, void* stream) {
  if (int rc = view_check("mesh_raycast_indexed", 1, h, w, nullptr, near, far, false)) return rc;
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_raycast_indexed: negative size");
  if (int rc = md_levels_arg("mesh_raycast_indexed", levels)) return rc;
  if (h == 0 || w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(rays && pose8 && range && normal && hit, "mesh_raycast_indexed: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && order && index && (vertices || num_vertices == 0)),
                "mesh_raycast_indexed: null pointer");
  return rc_cast_impl("mesh_raycast_indexed", true, rays, h, w, pose8, vertices, faces, num_faces, num_vertices, near,
                      far, num_faces > 0, index, index_bytes, order, levels, skip_counts, range, normal, hit, face,
                      t64, stream);
}
