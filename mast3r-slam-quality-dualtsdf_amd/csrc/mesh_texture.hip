// Mesh textures: the keyframe images baked into a per-face atlas, and the shading of a ray cast from vertex colours or
// from that atlas.  Semantics in DESIGN.md "Mesh textures"; tests/texture_numpy.py states the same definitions, operation
// by operation, in numpy.  Everything is f64 on the f32 inputs and the build has -ffp-contract=off, so a * b + c below is
// two roundings, as in numpy.
//
// THE ATLAS is a pure function of (F, R): face f is half f & 1 of cell f >> 1, a cell is R + 1 texels wide and R high,
// the cells lie row-major in `cols` columns.  Half 0 owns the cell-local texels i + j <= R - 1, half 1 the rest through
// the mirror (i, j) -> (R - i, R - 1 - j).  A point with barycentrics (alpha, beta, gamma) of a half-0 face lies at local
// (m + beta s, m + gamma s), m = 0.5, s = R - 3.5, so x + y <= R - 2.5 and the four texels of a bilinear footprint
// inside the closed triangle all belong to the face.
//
// THE BAKE is four kinds of launch, each one thread per texel in 256-thread blocks: every texel is owned by one thread
// and the views are added in index order, so there are no atomics and the result is bit-identical from call to call.
//   tx_rays_kernel        per view: the texel's world point, the view rule's geometric tests, the occlusion ray
//   (mslam_mesh_raycast   the caller casts those rays with h = 1; a zero direction misses at no cost in tiles)
//   tx_accumulate_kernel  per view: the occlusion test on t64, the weight, the bilinear sample, the four sums
//   tx_resolve_kernel     once: sums -> colour, or the fallback
// Nothing is written except the outputs.
#include "mesh_tri.h"

namespace mslam {

constexpr int kTxBlock = 256;

struct TxAtlas {
  int nf, R, cols, W;     // faces, texels per cell, cells per row, atlas width (R + 1) cols
};

// The face that owns texel n of the atlas (-1: none) and the texel's local coordinates in that face's half-0 frame.
__device__ __forceinline__ int tx_owner(const TxAtlas& at, int n, int* li, int* lj) {
  const int x = n % at.W, y = n / at.W;
  const int cx = x / (at.R + 1), cy = y / at.R;
  const long long c = (long long)cy * at.cols + cx;
  const int i = x - cx * (at.R + 1), j = y - cy * at.R;
  const int half = i + j > at.R - 1 ? 1 : 0;
  const long long f = 2 * c + half;
  *li = half ? at.R - i : i;
  *lj = half ? at.R - 1 - j : j;
  return f < at.nf ? (int)f : -1;
}

// (alpha, beta, gamma) of local texel (li, lj): negative ones set to 0, the three divided by their sum.
__device__ __forceinline__ void tx_bary(int R, int li, int lj, double* b) {
  const double s = (double)R - 3.5;
  double beta = ((double)li - 0.5) / s, gamma = ((double)lj - 0.5) / s;
  double alpha = (1.0 - beta) - gamma;
  alpha = alpha < 0.0 ? 0.0 : alpha, beta = beta < 0.0 ? 0.0 : beta, gamma = gamma < 0.0 ? 0.0 : gamma;
  const double tot = (alpha + beta) + gamma;
  b[0] = alpha / tot, b[1] = beta / tot, b[2] = gamma / tot;
}

// The three vertex indices of face f when all lie in [0, nv).
__device__ __forceinline__ bool tx_face(const int32_t* __restrict__ faces, int f, int nv, int* idx) {
  idx[0] = faces[3 * (size_t)f], idx[1] = faces[3 * (size_t)f + 1], idx[2] = faces[3 * (size_t)f + 2];
  return (unsigned)idx[0] < (unsigned)nv && (unsigned)idx[1] < (unsigned)nv && (unsigned)idx[2] < (unsigned)nv;
}

// Atlas coordinates of (beta, gamma) on face f, texel centres at integers; (x0, y0): the cell's origin.
__device__ __forceinline__ void tx_atlas_xy(int f, double beta, double gamma, int R, int cols, double* x, double* y,
                                            int* x0, int* y0) {
  const double s = (double)R - 3.5;
  double lx = 0.5 + beta * s, ly = 0.5 + gamma * s;
  if (f & 1) lx = (double)R - lx, ly = (double)(R - 1) - ly;
  const int c = f >> 1;
  *x0 = (c % cols) * (R + 1), *y0 = (c / cols) * R;
  *x = (double)*x0 + lx, *y = (double)*y0 + ly;
}

__global__ __launch_bounds__(kTxBlock) void tx_layout_kernel(TxAtlas at, int n, int32_t* __restrict__ owner) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  int li, lj;
  owner[i] = tx_owner(at, i, &li, &lj);
}

__global__ __launch_bounds__(kTxBlock) void tx_rays_kernel(TxAtlas at, int n, const float* __restrict__ vert,
                                                           const int32_t* __restrict__ faces, int nv,
                                                           const float* __restrict__ pose8, double fx, double fy,
                                                           double cx, double cy, int h, int w, double near, double far,
                                                           double cos_min, float* __restrict__ dir,
                                                           double* __restrict__ r_out, double* __restrict__ cos_out,
                                                           double* __restrict__ uv) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  float d[3] = {0.0f, 0.0f, 0.0f};
  double r = 0.0, cs = 0.0, u = 0.0, vv = 0.0;
  int li, lj, idx[3];
  const int f = tx_owner(at, i, &li, &lj);
  if (f >= 0 && tx_face(faces, f, nv, idx)) {
    double b[3], A[3], B[3], C[3], p[3], v[3];
    tx_bary(at.R, li, lj, b);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      A[k] = (double)vert[3 * (size_t)idx[0] + k];
      B[k] = (double)vert[3 * (size_t)idx[1] + k];
      C[k] = (double)vert[3 * (size_t)idx[2] + k];
      p[k] = (b[0] * A[k] + b[1] * B[k]) + b[2] * C[k];
      v[k] = p[k] - (double)pose8[k];
    }
    const double abx = B[0] - A[0], aby = B[1] - A[1], abz = B[2] - A[2];
    const double acx = C[0] - A[0], acy = C[1] - A[1], acz = C[2] - A[2];
    double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len, ny = ny / len, nz = nz / len;
    // the conjugate quaternion: camera from world
    const double q0 = -(double)pose8[3], q1 = -(double)pose8[4], q2 = -(double)pose8[5], q3 = (double)pose8[6];
    const double u0 = 2.0 * (q1 * v[2] - q2 * v[1]);
    const double u1 = 2.0 * (q2 * v[0] - q0 * v[2]);
    const double u2 = 2.0 * (q0 * v[1] - q1 * v[0]);
    const double X = (v[0] + q3 * u0) + (q1 * u2 - q2 * u1);
    const double Y = (v[1] + q3 * u1) + (q2 * u0 - q0 * u2);
    const double Z = (v[2] + q3 * u2) + (q0 * u1 - q1 * u0);
    const double rr = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double pu = fx * X / Z + cx, pv = fy * Y / Z + cy;
    const double c = -((nx * v[0] + ny * v[1]) + nz * v[2]) / rr;
    const bool finite_n = fabs(nx) < INFINITY && fabs(ny) < INFINITY && fabs(nz) < INFINITY;   // false on a NaN
    if (finite_n && Z > 0.0 && pu >= -0.5 && pu < (double)w - 0.5 && pv >= -0.5 && pv < (double)h - 0.5 &&
        rr >= near && rr <= far && c >= cos_min && c > 0.0) {
      d[0] = (float)(v[0] / rr), d[1] = (float)(v[1] / rr), d[2] = (float)(v[2] / rr);
      r = rr, cs = c, u = pu, vv = pv;
    }
  }
  dir[3 * (size_t)i] = d[0], dir[3 * (size_t)i + 1] = d[1], dir[3 * (size_t)i + 2] = d[2];
  r_out[i] = r, cos_out[i] = cs;
  uv[2 * (size_t)i] = u, uv[2 * (size_t)i + 1] = vv;
}

// Bilinear sample of a row-major f32 image with 3 channels at the four corners given, a + f (b - a) along x, then y.
__device__ __forceinline__ void tx_bilinear(const float* __restrict__ img, size_t i00, size_t i01, size_t i10,
                                            size_t i11, double fx, double fy, double* out) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double a = (double)img[3 * i00 + c], b = (double)img[3 * i01 + c];
    const double e = (double)img[3 * i10 + c], g = (double)img[3 * i11 + c];
    const double top = a + fx * (b - a), bot = e + fx * (g - e);
    out[c] = top + fy * (bot - top);
  }
}

__global__ __launch_bounds__(kTxBlock) void tx_accumulate_kernel(int n, const double* __restrict__ t64,
                                                                 const double* __restrict__ r_in,
                                                                 const double* __restrict__ cos_in,
                                                                 const double* __restrict__ uv,
                                                                 const float* __restrict__ image, int h, int w,
                                                                 const float* __restrict__ pose8, double tol,
                                                                 double* __restrict__ sums,
                                                                 int32_t* __restrict__ views) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  const double cs = cos_in[i], r = r_in[i];
  if (!(cs > 0.0) || !(t64[i] >= r - tol)) return;
  const double sc = (double)pose8[7];
  const double wgt = (cs * (sc / r)) * (sc / r);
  const double uc = fmin(fmax(uv[2 * (size_t)i], 0.0), (double)w - 1.0);
  const double vc = fmin(fmax(uv[2 * (size_t)i + 1], 0.0), (double)h - 1.0);
  const double xf = fmin(floor(uc), (double)w - 2.0), yf = fmin(floor(vc), (double)h - 2.0);
  const int x0 = (int)xf, y0 = (int)yf;                  // in [0, w - 2] x [0, h - 2]: uc, vc are clamped
  double col[3];
  const size_t i00 = (size_t)y0 * w + x0;
  tx_bilinear(image, i00, i00 + 1, i00 + w, i00 + w + 1, uc - xf, vc - yf, col);
  double* s = sums + 4 * (size_t)i;
  s[0] += wgt;
  s[1] += wgt * col[0], s[2] += wgt * col[1], s[3] += wgt * col[2];
  views[i] += 1;
}

__global__ __launch_bounds__(kTxBlock) void tx_resolve_kernel(TxAtlas at, int n, const int32_t* __restrict__ faces,
                                                              int nv, const double* __restrict__ sums,
                                                              const float* __restrict__ colors, double default_color,
                                                              float* __restrict__ atlas) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  int li, lj, idx[3];
  const int f = tx_owner(at, i, &li, &lj);
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (f >= 0) {
    const double* s = sums + 4 * (size_t)i;
    if (s[0] > 0.0) {
#pragma unroll
      for (int c = 0; c < 3; c++) out[c] = (float)(s[1 + c] / s[0]);
    } else if (colors && tx_face(faces, f, nv, idx)) {
      double b[3];
      tx_bary(at.R, li, lj, b);
#pragma unroll
      for (int c = 0; c < 3; c++)
        out[c] = (float)((b[0] * (double)colors[3 * (size_t)idx[0] + c] + b[1] * (double)colors[3 * (size_t)idx[1] + c]) +
                         b[2] * (double)colors[3 * (size_t)idx[2] + c]);
    } else {
      out[0] = out[1] = out[2] = (float)default_color;
    }
  }
  atlas[3 * (size_t)i] = out[0], atlas[3 * (size_t)i + 1] = out[1], atlas[3 * (size_t)i + 2] = out[2];
}

__device__ __forceinline__ double tx_pick(double a0, double a1, double a2, int k) {
  return k == 0 ? a0 : (k == 1 ? a1 : a2);
}

// The colour of every hit pixel of a ray cast: steps 1-4 of the intersection (mesh_raycast.hip) for the one face hit,
// the same operations in the same order, then (U, V, W) / det as the barycentrics of a, b, c.  The pixel-to-thread map
// is the cast's: 8x8 pixels per wave, h = 1 a plain list.
__global__ __launch_bounds__(kMdBlock) void tx_shade_kernel(const int32_t* __restrict__ face,
                                                            const float* __restrict__ rays, int h, int w,
                                                            const float* __restrict__ pose8,
                                                            const float* __restrict__ vert,
                                                            const int32_t* __restrict__ faces, int nf, int nv,
                                                            const float* __restrict__ colors,
                                                            const float* __restrict__ atlas, int R, int cols,
                                                            float* __restrict__ rgb) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long px = h == 1 ? (long long)blockIdx.x * kMdBlock + tid : blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int py = h == 1 ? 0 : blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (!(px < w && py < h)) return;
  const size_t i = (size_t)py * w + (size_t)px;
  float out[3] = {0.0f, 0.0f, 0.0f};
  const int f = face[i];
  int idx[3];
  if ((unsigned)f < (unsigned)nf && tx_face(faces, f, nv, idx)) {
    const double q[4] = {(double)pose8[3], (double)pose8[4], (double)pose8[5], (double)pose8[6]};
    const double c[3] = {(double)rays[3 * i], (double)rays[3 * i + 1], (double)rays[3 * i + 2]};
    const double u0 = 2.0 * (q[1] * c[2] - q[2] * c[1]);
    const double u1 = 2.0 * (q[2] * c[0] - q[0] * c[2]);
    const double u2 = 2.0 * (q[0] * c[1] - q[1] * c[0]);
    const double d0 = (c[0] + q[3] * u0) + (q[1] * u2 - q[2] * u1);
    const double d1 = (c[1] + q[3] * u1) + (q[2] * u0 - q[0] * u2);
    const double d2 = (c[2] + q[3] * u2) + (q[0] * u1 - q[1] * u0);
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    int kz = a1 > a0 ? 1 : 0;
    if (a2 > (kz ? a1 : a0)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = tx_pick(d0, d1, d2, kz);
    if (dz < 0.0) {
      const int s = kx;
      kx = ky, ky = s;
    }
    const double sx = tx_pick(d0, d1, d2, kx) / dz, sy = tx_pick(d0, d1, d2, ky) / dz;
    double x[3], y[3];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const double q0 = (double)vert[3 * (size_t)idx[v]] - (double)pose8[0];
      const double q1 = (double)vert[3 * (size_t)idx[v] + 1] - (double)pose8[1];
      const double q2 = (double)vert[3 * (size_t)idx[v] + 2] - (double)pose8[2];
      const double qz = tx_pick(q0, q1, q2, kz);
      x[v] = tx_pick(q0, q1, q2, kx) - sx * qz;
      y[v] = tx_pick(q0, q1, q2, ky) - sy * qz;
    }
    const double U = x[2] * y[1] - y[2] * x[1];
    const double V = x[0] * y[2] - y[0] * x[2];
    const double W = x[1] * y[0] - y[1] * x[0];
    const double det = (U + V) + W;
    if (colors) {
#pragma unroll
      for (int k = 0; k < 3; k++)
        out[k] = (float)(((U * (double)colors[3 * (size_t)idx[0] + k] + V * (double)colors[3 * (size_t)idx[1] + k]) +
                          W * (double)colors[3 * (size_t)idx[2] + k]) / det);
    } else {
      const double beta = V / det, gamma = W / det;
      if (fabs(beta) < INFINITY && fabs(gamma) < INFINITY) {           // false on a NaN: det = 0
        double ax, ay, col[3];
        int x0c, y0c;
        tx_atlas_xy(f, beta, gamma, R, cols, &ax, &ay, &x0c, &y0c);
        const double xf = floor(ax), yf = floor(ay);
        // the integer corners, clamped into the cell [x0c, x0c + R] x [y0c, y0c + R - 1] (a guard; the doubles first,
        // so that the conversion is defined for any beta, gamma)
        const int xi = (int)fmin(fmax(xf, (double)x0c - 1.0), (double)(x0c + R) + 1.0);
        const int yi = (int)fmin(fmax(yf, (double)y0c - 1.0), (double)(y0c + R - 1) + 1.0);
        const int xa = min(max(xi, x0c), x0c + R), xb = min(max(xi + 1, x0c), x0c + R);
        const int ya = min(max(yi, y0c), y0c + R - 1), yb = min(max(yi + 1, y0c), y0c + R - 1);
        const size_t Wd = (size_t)cols * (R + 1);
        tx_bilinear(atlas, ya * Wd + xa, ya * Wd + xb, yb * Wd + xa, yb * Wd + xb, ax - xf, ay - yf, col);
        out[0] = (float)col[0], out[1] = (float)col[1], out[2] = (float)col[2];
      }
    }
  }
  rgb[3 * i] = out[0], rgb[3 * i + 1] = out[1], rgb[3 * i + 2] = out[2];
}

// The checked atlas of (F, R, cols, rows) -> at, n = H W texels; false with the error set.
static bool tx_atlas_arg(const char* what, int num_faces, int texels, int cols, int rows, TxAtlas* at, int* n) {
  const int64_t cells = ((int64_t)num_faces + 1) >> 1;
  if (num_faces < 0 || texels < 4 || cols < 0 || rows < 0 || (int64_t)cols * rows < cells) {
    set_error("%s: an atlas of %d x %d cells of %d texels does not hold %d faces (texels >= 4)", what, rows, cols, texels,
              num_faces);
    return false;
  }
  const int64_t total = (int64_t)rows * texels * cols * ((int64_t)texels + 1);
  if (total >= (1ll << 31) || 3 * (int64_t)num_faces >= (1ll << 31)) {
    set_error("%s: %lld texels / %d faces are outside the int32 index range", what, (long long)total, num_faces);
    return false;
  }
  *at = TxAtlas{num_faces, texels, cols, cols * (texels + 1)};
  *n = (int)total;
  return true;
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_texture_layout(int num_faces, int texels, int cols, int rows, int32_t* owner, void* stream) {
  TxAtlas at;
  int n;
  if (!tx_atlas_arg("mesh_texture_layout", num_faces, texels, cols, rows, &at, &n)) return MSLAM_EINVAL;
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(owner, "mesh_texture_layout: null pointer");
  hipLaunchKernelGGL(tx_layout_kernel, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at, n,
                     owner);
  MSLAM_LAUNCH_CHECK("mesh_texture_layout");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_rays(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                       int texels, int cols, int rows, const float* pose8, double fx, double fy,
                                       double cx, double cy, int h, int w, double near, double far, double cos_min,
                                       float* dir, double* r, double* cos, double* uv, void* stream) {
  TxAtlas at;
  int n;
  if (!tx_atlas_arg("mesh_texture_rays", num_faces, texels, cols, rows, &at, &n)) return MSLAM_EINVAL;
  MSLAM_REQUIRE(num_vertices >= 0, "mesh_texture_rays: negative size");
  MSLAM_REQUIRE(h >= 2 && w >= 2, "mesh_texture_rays: an image must be at least 2x2, got %dx%d", h, w);
  MSLAM_REQUIRE(near <= far && cos_min == cos_min, "mesh_texture_rays: near must not exceed far, cos_min not be NaN");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && pose8 && dir && r && cos && uv && (vertices || num_vertices == 0),
                "mesh_texture_rays: null pointer");
  hipLaunchKernelGGL(tx_rays_kernel, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at, n,
                     vertices, faces, num_vertices, pose8, fx, fy, cx, cy, h, w, near, far, cos_min, dir, r, cos, uv);
  MSLAM_LAUNCH_CHECK("mesh_texture_rays");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_accumulate(const double* t64, const double* r, const double* cos, const double* uv,
                                             const float* image, int h, int w, const float* pose8, double tol, int n,
                                             double* sums, int32_t* views, void* stream) {
  MSLAM_REQUIRE(n >= 0, "mesh_texture_accumulate: negative size");
  MSLAM_REQUIRE(h >= 2 && w >= 2 && (int64_t)h * w < (1ll << 31),
                "mesh_texture_accumulate: an image must be at least 2x2 and within int32, got %dx%d", h, w);
  MSLAM_REQUIRE(tol == tol, "mesh_texture_accumulate: tol is NaN");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(t64 && r && cos && uv && image && pose8 && sums && views, "mesh_texture_accumulate: null pointer");
  hipLaunchKernelGGL(tx_accumulate_kernel, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, n, t64,
                     r, cos, uv, image, h, w, pose8, tol, sums, views);
  MSLAM_LAUNCH_CHECK("mesh_texture_accumulate");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_resolve(const int32_t* faces, int num_faces, int num_vertices, int texels, int cols,
                                          int rows, const double* sums, const float* colors, double default_color,
                                          float* atlas, void* stream) {
  TxAtlas at;
  int n;
  if (!tx_atlas_arg("mesh_texture_resolve", num_faces, texels, cols, rows, &at, &n)) return MSLAM_EINVAL;
  MSLAM_REQUIRE(num_vertices >= 0, "mesh_texture_resolve: negative size");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && sums && atlas, "mesh_texture_resolve: null pointer");
  hipLaunchKernelGGL(tx_resolve_kernel, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at, n,
                     faces, num_vertices, sums, colors, default_color, atlas);
  MSLAM_LAUNCH_CHECK("mesh_texture_resolve");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_shade(const int32_t* face, const float* rays, int h, int w, const float* pose8,
                                const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                const float* colors, const float* atlas, int texels, int cols, int rows, float* rgb,
                                void* stream) {
  MSLAM_REQUIRE(h >= 0 && w >= 0 && (int64_t)h * w < (1ll << 31), "mesh_shade: bad image size");
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_shade: negative size");
  MSLAM_REQUIRE((colors != nullptr) != (atlas != nullptr), "mesh_shade: give either colors or an atlas");
  if (atlas) {
    TxAtlas at;
    int n;
    if (!tx_atlas_arg("mesh_shade", num_faces, texels, cols, rows, &at, &n)) return MSLAM_EINVAL;
  }
  if (h == 0 || w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(face && rays && pose8 && rgb, "mesh_shade: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && (vertices || num_vertices == 0)), "mesh_shade: null pointer");
  const dim3 grid = h == 1 ? dim3(blocks_for(w, kMdBlock)) : dim3((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16));
  hipLaunchKernelGGL(tx_shade_kernel, grid, dim3(kMdBlock), 0, (hipStream_t)stream, face, rays, h, w, pose8, vertices,
                     faces, num_faces, num_vertices, colors, atlas, texels, cols, rgb);
  MSLAM_LAUNCH_CHECK("mesh_shade");
  return MSLAM_OK;
}
