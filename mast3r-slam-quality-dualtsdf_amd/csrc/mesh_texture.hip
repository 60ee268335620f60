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
#include "view.h"

namespace mslam {

constexpr int kTxBlock = 256;
static_assert(kMdBlock == kViewBlock, "the shade's blocks are the view's");

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

__device__ __forceinline__ int tx_texel(const TxAtlas& at, int n, int* R, int* li, int* lj) {
  *R = at.R;
  return tx_owner(at, n, li, lj);
}

// THE SIZED ATLAS (DESIGN.md "Mesh textures: sized atlas"): every face has its own R_f, one of kTxClasses values, and the
// cells of one class lie in one band.  Only the layout kernels below know the packing; they write `owner` i32[H,W] and
// `cell` i32[F,4] = (x0, y0, R_f, half), and the sized rays, resolve and shade recover the cell-local texel from those
// two: i = x - x0, j = y - y0, mirrored for half 1.  From there on the arithmetic is the uniform atlas's.
struct TxSized {
  const int32_t* owner;   // [H W]
  const int32_t* cell;    // [nf, 4]
  int nf, W;
};

__device__ __forceinline__ int tx_texel(const TxSized& at, int n, int* R, int* li, int* lj) {
  const int f = at.owner[n];
  *R = 4, *li = 0, *lj = 0;
  if ((unsigned)f >= (unsigned)at.nf) return -1;
  const int32_t* c = at.cell + 4 * (size_t)f;
  const int i = n % at.W - c[0], j = n / at.W - c[1];
  *R = c[2];
  *li = c[3] ? c[2] - i : i;
  *lj = c[3] ? c[2] - 1 - j : j;
  return f;
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

// Atlas coordinates of (beta, gamma) on the face that is half `half` of the cell of R texels at (x0, y0), texel centres
// at integers.
__device__ __forceinline__ void tx_atlas_xy(int half, double beta, double gamma, int R, int x0, int y0, double* x,
                                            double* y) {
  const double s = (double)R - 3.5;
  double lx = 0.5 + beta * s, ly = 0.5 + gamma * s;
  if (half) lx = (double)R - lx, ly = (double)(R - 1) - ly;
  *x = (double)x0 + lx, *y = (double)y0 + ly;
}

__global__ __launch_bounds__(kTxBlock) void tx_layout_kernel(TxAtlas at, int n, int32_t* __restrict__ owner) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  int li, lj;
  owner[i] = tx_owner(at, i, &li, &lj);
}

template <class Atlas>
__global__ __launch_bounds__(kTxBlock) void tx_rays_kernel(Atlas at, int n, const float* __restrict__ vert,
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
  int R, li, lj, idx[3];
  const int f = tx_texel(at, i, &R, &li, &lj);
  if (f >= 0 && tx_face(faces, f, nv, idx)) {
    double b[3], A[3], B[3], C[3], p[3];
    tx_bary(R, li, lj, b);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      A[k] = (double)vert[3 * (size_t)idx[0] + k];
      B[k] = (double)vert[3 * (size_t)idx[1] + k];
      C[k] = (double)vert[3 * (size_t)idx[2] + k];
      p[k] = (b[0] * A[k] + b[1] * B[k]) + b[2] * C[k];
    }
    const double abx = B[0] - A[0], aby = B[1] - A[1], abz = B[2] - A[2];
    const double acx = C[0] - A[0], acy = C[1] - A[1], acz = C[2] - A[2];
    double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len, ny = ny / len, nz = nz / len;
    const ViewCamera cam = {fx, fy, cx, cy, h, w, near, far};
    const ViewProjection pr = view_project(p, pose8, cam);
    const double* v = pr.v3;
    const double c = -((nx * v[0] + ny * v[1]) + nz * v[2]) / pr.r;
    const bool finite_n = fabs(nx) < INFINITY && fabs(ny) < INFINITY && fabs(nz) < INFINITY;   // false on a NaN
    if (finite_n && pr.in_view && c >= cos_min && c > 0.0) {
      d[0] = (float)(v[0] / pr.r), d[1] = (float)(v[1] / pr.r), d[2] = (float)(v[2] / pr.r);
      r = pr.r, cs = c, u = pr.u, vv = pr.v;
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

template <class Atlas>
__global__ __launch_bounds__(kTxBlock) void tx_resolve_kernel(Atlas at, int n, const int32_t* __restrict__ faces,
                                                              int nv, const double* __restrict__ sums,
                                                              const float* __restrict__ colors, double default_color,
                                                              float* __restrict__ atlas) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  int R, li, lj, idx[3];
  const int f = tx_texel(at, i, &R, &li, &lj);
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (f >= 0) {
    const double* s = sums + 4 * (size_t)i;
    if (s[0] > 0.0) {
#pragma unroll
      for (int c = 0; c < 3; c++) out[c] = (float)(s[1 + c] / s[0]);
    } else if (colors && tx_face(faces, f, nv, idx)) {
      double b[3];
      tx_bary(R, li, lj, b);
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
                                                            const int32_t* __restrict__ face_cell, int aH, int aW,
                                                            float* __restrict__ rgb) {
  long long px;
  int py;
  view_pixel(h, px, py);
  if (!(px < w && py < h)) return;
  const size_t i = (size_t)py * w + (size_t)px;
  float out[3] = {0.0f, 0.0f, 0.0f};
  const int f = face[i];
  int idx[3];
  if ((unsigned)f < (unsigned)nf && tx_face(faces, f, nv, idx)) {
    double o[3], d[3];
    view_ray(rays, i, pose8, o, d);
    const ViewShear s = view_shear(d);      // only pixels with a hit face come here; castability is not asked again
    double x[3], y[3];
#pragma unroll
    for (int v = 0; v < 3; v++) {
      const double q0 = (double)vert[3 * (size_t)idx[v]] - o[0];
      const double q1 = (double)vert[3 * (size_t)idx[v] + 1] - o[1];
      const double q2 = (double)vert[3 * (size_t)idx[v] + 2] - o[2];
      const double qz = rc_pick<-1>(q0, q1, q2, s.kz);
      x[v] = rc_pick<-1>(q0, q1, q2, s.kx) - s.sx * qz;
      y[v] = rc_pick<-1>(q0, q1, q2, s.ky) - s.sy * qz;
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
        int x0c, y0c, half = f & 1;
        bool cell_ok = true;
        if (face_cell) {                  // sized: the face's own cell, which must lie inside the atlas
          const int32_t* fc = face_cell + 4 * (size_t)f;
          x0c = fc[0], y0c = fc[1], R = fc[2], half = fc[3] ? 1 : 0;
          cell_ok = R >= 4 && x0c >= 0 && y0c >= 0 && (long long)x0c + R < aW && (long long)y0c + R <= aH;
        } else {
          x0c = ((f >> 1) % cols) * (R + 1), y0c = ((f >> 1) / cols) * R;
        }
        if (cell_ok) {
          tx_atlas_xy(half, beta, gamma, R, x0c, y0c, &ax, &ay);
          const double xf = floor(ax), yf = floor(ay);
          // the integer corners, clamped into the cell [x0c, x0c + R] x [y0c, y0c + R - 1] (a guard; the doubles
          // first, so that the conversion is defined for any beta, gamma)
          const int xi = (int)fmin(fmax(xf, (double)x0c - 1.0), (double)(x0c + R) + 1.0);
          const int yi = (int)fmin(fmax(yf, (double)y0c - 1.0), (double)(y0c + R - 1) + 1.0);
          const int xa = min(max(xi, x0c), x0c + R), xb = min(max(xi + 1, x0c), x0c + R);
          const int ya = min(max(yi, y0c), y0c + R - 1), yb = min(max(yi + 1, y0c), y0c + R - 1);
          const size_t Wd = (size_t)aW;
          tx_bilinear(atlas, ya * Wd + xa, ya * Wd + xb, yb * Wd + xa, yb * Wd + xb, ax - xf, ay - yf, col);
          out[0] = (float)col[0], out[1] = (float)col[1], out[2] = (float)col[2];
        }
      }
    }
  }
  rgb[3 * i] = out[0], rgb[3 * i + 1] = out[1], rgb[3 * i + 2] = out[2];
}

// ---- the sized atlas: classes, stable rank, layout ---------------------------------------------------------------------
constexpr int kTxClasses = 13;                 // R in {4, 6, 8, 12, ..., 192, 256}: each step is at most 1.5x
constexpr int kTxCols = kTxClasses + 1;        // a row of the count table: the 13 class counts and the clamped count
constexpr int kTxWaves = kTxBlock / kWave;

__host__ __device__ constexpr int tx_class_R(int c) { return ((c & 1) ? 6 : 4) << (c >> 1); }

// One thread per face: the class of R_f and whether the face needed more than the cap.  need = ceil(density L + 3.5),
// L the longest edge; the smallest class >= max(need, floor), capped.  A face with an index out of range or an edge
// that is not finite gets the floor class.
__global__ __launch_bounds__(kTxBlock) void tx_class_kernel(const float* __restrict__ vert,
                                                            const int32_t* __restrict__ faces, int nf, int nv,
                                                            double density, int lo, int cap, int32_t* __restrict__ cls,
                                                            int32_t* __restrict__ clamped) {
  const int f = blockIdx.x * kTxBlock + threadIdx.x;
  if (f >= nf) return;
  int idx[3], c = lo, over = 0;
  if (tx_face(faces, f, nv, idx)) {
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const size_t p = 3 * (size_t)idx[k], q = 3 * (size_t)idx[k == 2 ? 0 : k + 1];
      const double dx = (double)vert[q] - (double)vert[p], dy = (double)vert[q + 1] - (double)vert[p + 1];
      const double dz = (double)vert[q + 2] - (double)vert[p + 2];
      e[k] = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    if (e[0] < INFINITY && e[1] < INFINITY && e[2] < INFINITY) {          // false on a NaN
      const double L = fmax(fmax(e[0], e[1]), e[2]);
      const double need = ceil(density * L + 3.5);
      c = 0;
#pragma unroll
      for (int k = 0; k < kTxClasses; k++) c += (double)tx_class_R(k) < need ? 1 : 0;    // the first class >= need
      c = min(max(c, lo), cap);
      over = need > (double)tx_class_R(cap) ? 1 : 0;
    }
  }
  cls[f] = c, clamped[f] = over;
}

// THE STABLE RANK BY CLASS is a counting sort of the faces over 13 keys in three launches, in integers and without
// atomics, so that the rank depends on nothing but the classes.  Within a wave the faces of class k below a lane are the
// set bits below it of the ballot of `class == k`; the waves of a block add up through LDS; the blocks through the
// table i32[blocks + 1, 14], which the second launch turns into exclusive prefixes per column with the totals in the
// last row.
__global__ __launch_bounds__(kTxBlock) void tx_rank_count_kernel(const int32_t* __restrict__ cls,
                                                                 const int32_t* __restrict__ clamped, int nf,
                                                                 int32_t* __restrict__ table) {
  __shared__ int wc[kTxWaves][kTxCols];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int f = blockIdx.x * kTxBlock + tid;
  const int c = f < nf ? cls[f] : -1;
  const int over = f < nf ? (clamped[f] != 0) : 0;
#pragma unroll
  for (int k = 0; k < kTxClasses; k++) {
    const unsigned long long m = __ballot(c == k);
    if (lane == 0) wc[wave][k] = __popcll(m);
  }
  const unsigned long long m = __ballot(over);
  if (lane == 0) wc[wave][kTxClasses] = __popcll(m);
  __syncthreads();
  if (tid < kTxCols) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kTxWaves; w++) s += wc[w][tid];
    table[(size_t)blockIdx.x * kTxCols + tid] = s;
  }
}

// One block: wave w scans the columns w, w + 4, ... of the table over the blocks, 64 rows at a time.
__global__ __launch_bounds__(kTxBlock) void tx_rank_scan_kernel(int nblk, int32_t* __restrict__ table) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int col = wave; col < kTxCols; col += kTxWaves) {
    int carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += kWave) {
      const int b = b0 + lane;
      const int v = b < nblk ? table[(size_t)b * kTxCols + col] : 0;
      int s = v;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(s, off, kWave);
        if (lane >= off) s += t;
      }
      if (b < nblk) table[(size_t)b * kTxCols + col] = carry + (s - v);
      carry += __shfl(s, kWave - 1, kWave);
    }
    if (lane == 0) table[(size_t)nblk * kTxCols + col] = carry;
  }
}

// rank[f], order[base of the class + rank] = f, and the 14 totals.  One ballot per class in use.
__global__ __launch_bounds__(kTxBlock) void tx_rank_write_kernel(const int32_t* __restrict__ cls, int nf, int nblk,
                                                                 const int32_t* __restrict__ table,
                                                                 int32_t* __restrict__ rank, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ counts) {
  __shared__ int wc[kTxWaves][kTxClasses];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int f = blockIdx.x * kTxBlock + tid;
  const int c = f < nf ? cls[f] : -1;
  const int32_t* total = table + (size_t)nblk * kTxCols;
  int below = 0, base = 0;
#pragma unroll
  for (int k = kTxClasses - 1; k >= 0; k--) {
    const int tk = total[k];                                            // the same for every thread of the grid
    if (tk == 0) continue;
    const unsigned long long m = __ballot(c == k);
    if (lane == 0) wc[wave][k] = __popcll(m);
    if (c == k) below = __popcll(m & ((1ull << lane) - 1ull));
    if (c < k) base += tk;                                              // the classes of a larger R come first
  }
  __syncthreads();
  if (f < nf) {
    int r = -1;
    if ((unsigned)c < (unsigned)kTxClasses) {
      r = table[(size_t)blockIdx.x * kTxCols + c] + below;
      for (int w = 0; w < wave; w++) r += wc[w][c];
      order[base + r] = f;
    }
    rank[f] = r;
  }
  if (blockIdx.x == 0 && tid < kTxCols) counts[tid] = total[tid];
}

// The band table, by value: per class (R is tx_class_R) the cells per row, the rows, the first texel row, the first
// position in `order` and the faces.
struct TxBands {
  int cols[kTxClasses], rows[kTxClasses], y0[kTxClasses], base[kTxClasses], count[kTxClasses];
};

// owner of texel i: the band from the row, the cell and the half inside it, the face from `order`.  The loop is
// unrolled so that the table stays in scalar registers.
__global__ __launch_bounds__(kTxBlock) void tx_layout_sized_kernel(TxBands bd, int n, int W,
                                                                   const int32_t* __restrict__ order,
                                                                   int32_t* __restrict__ owner) {
  const int i = blockIdx.x * kTxBlock + threadIdx.x;
  if (i >= n) return;
  const int x = i % W, y = i / W;
  long long at = -1;
#pragma unroll
  for (int c = 0; c < kTxClasses; c++) {
    const int R = tx_class_R(c), yy = y - bd.y0[c];
    if (bd.count[c] > 0 && yy >= 0 && yy < bd.rows[c] * R) {
      const int cx = x / (R + 1), cy = yy / R;
      const int ii = x - cx * (R + 1), jj = yy - cy * R;
      const long long k = 2 * ((long long)cy * bd.cols[c] + cx) + (ii + jj > R - 1 ? 1 : 0);
      if (cx < bd.cols[c] && k < bd.count[c]) at = bd.base[c] + k;
    }
  }
  owner[i] = at >= 0 ? order[at] : -1;
}

// face_cell[f] = (x0, y0, R_f, half) from the face's class and rank.
__global__ __launch_bounds__(kTxBlock) void tx_face_cell_kernel(TxBands bd, int nf, const int32_t* __restrict__ cls,
                                                                const int32_t* __restrict__ rank,
                                                                int32_t* __restrict__ cell) {
  const int f = blockIdx.x * kTxBlock + threadIdx.x;
  if (f >= nf) return;
  const int c = cls[f], k = rank[f];
  int R = 4, cols = 0, y0 = 0, count = 0;
#pragma unroll
  for (int j = 0; j < kTxClasses; j++)
    if (c == j) R = tx_class_R(j), cols = bd.cols[j], y0 = bd.y0[j], count = bd.count[j];
  int out[4] = {0, 0, R, 0};
  if (k >= 0 && k < count) {                     // cols >= 1 where count > 0 (tx_bands_arg)
    const int q = k >> 1;
    out[0] = (q % cols) * (R + 1), out[1] = y0 + (q / cols) * R, out[3] = k & 1;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) cell[4 * (size_t)f + j] = out[j];
}

// The checked band table of a sized atlas of H x W texels for num_faces faces: rows of (R, cols, rows, y0, base, count)
// on the host, largest class first in y and in `order`; false with the error set.
static bool tx_bands_arg(const char* what, const int32_t* bands, int num_faces, int H, int W, TxBands* bd, int* n) {
  if (!bands || num_faces < 0 || H < 0 || W < 0) {
    set_error("%s: null band table or negative size", what);
    return false;
  }
  if ((int64_t)H * W >= (1ll << 31) || 3 * (int64_t)num_faces >= (1ll << 31)) {
    set_error("%s: %lld texels / %d faces are outside the int32 index range", what, (long long)H * W, num_faces);
    return false;
  }
  int64_t y = 0, base = 0;
  for (int c = kTxClasses - 1; c >= 0; c--) {
    const int32_t* b = bands + 6 * c;
    const int64_t R = tx_class_R(c), cells = ((int64_t)b[5] + 1) >> 1;
    const bool ok = b[0] == R && b[1] >= 0 && b[2] >= 0 && b[5] >= 0 && b[3] == y && b[4] == base &&
                    (int64_t)b[1] * (R + 1) <= W && (int64_t)b[1] * b[2] >= cells && (b[5] > 0 || b[2] == 0);
    if (!ok) {
      set_error("%s: row %d of the band table (R %d, cols %d, rows %d, y0 %d, base %d, count %d) does not fit an atlas "
                "%d wide at row %lld, position %lld", what, c, b[0], b[1], b[2], b[3], b[4], b[5], W, (long long)y,
                (long long)base);
      return false;
    }
    bd->cols[c] = b[1], bd->rows[c] = b[2], bd->y0[c] = b[3], bd->base[c] = b[4], bd->count[c] = b[5];
    y += (int64_t)b[2] * R, base += b[5];
    if (y > H || base > num_faces) break;
  }
  if (y != H || base != num_faces) {
    set_error("%s: the bands hold %lld rows and %lld faces, the atlas %d rows and %d faces", what, (long long)y,
              (long long)base, H, num_faces);
    return false;
  }
  *n = H * W;
  return true;
}

// The checked sized atlas (owner, face_cell, H, W) -> at, n; false with the error set.
static bool tx_sized_arg(const char* what, const int32_t* owner, const int32_t* face_cell, int num_faces, int H, int W,
                         TxSized* at, int* n) {
  if (num_faces < 0 || H < 0 || W < 0 || (int64_t)H * W >= (1ll << 31) || 3 * (int64_t)num_faces >= (1ll << 31)) {
    set_error("%s: an atlas of %d x %d texels / %d faces is negative or outside the int32 index range", what, H, W,
              num_faces);
    return false;
  }
  *n = H * W;
  if (*n && (!owner || (num_faces && !face_cell))) {
    set_error("%s: null pointer", what);
    return false;
  }
  *at = TxSized{owner, face_cell, num_faces, W};
  return true;
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
  if (int rc = view_check("mesh_texture_rays", 1, h, w, nullptr, near, far, false)) return rc;
  MSLAM_REQUIRE(cos_min == cos_min, "mesh_texture_rays: cos_min must not be NaN");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && pose8 && dir && r && cos && uv && (vertices || num_vertices == 0),
                "mesh_texture_rays: null pointer");
  hipLaunchKernelGGL(tx_rays_kernel<TxAtlas>, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at, n,
                     vertices, faces, num_vertices, pose8, fx, fy, cx, cy, h, w, near, far, cos_min, dir, r, cos, uv);
  MSLAM_LAUNCH_CHECK("mesh_texture_rays");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_accumulate(const double* t64, const double* r, const double* cos, const double* uv,
                                             const float* image, int h, int w, const float* pose8, double tol, int n,
                                             double* sums, int32_t* views, void* stream) {
  MSLAM_REQUIRE(n >= 0, "mesh_texture_accumulate: negative size");
  MSLAM_REQUIRE(h >= 2 && w >= 2, "mesh_texture_accumulate: an image must be at least 2x2, got %dx%d", h, w);
  if (int rc = view_check("mesh_texture_accumulate", 1, h, w, nullptr, 0.0, 0.0, false)) return rc;
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
  hipLaunchKernelGGL(tx_resolve_kernel<TxAtlas>, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at, n,
                     faces, num_vertices, sums, colors, default_color, atlas);
  MSLAM_LAUNCH_CHECK("mesh_texture_resolve");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_shade(const int32_t* face, const float* rays, int h, int w, const float* pose8,
                                const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                const float* colors, const float* atlas, int texels, int cols, int rows, float* rgb,
                                void* stream) {
  if (int rc = view_check("mesh_shade", 1, h, w, nullptr, 0.0, 0.0, false)) return rc;
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
  hipLaunchKernelGGL(tx_shade_kernel, view_grid(h, w), dim3(kMdBlock), 0, (hipStream_t)stream, face, rays, h, w, pose8,
                     vertices, faces, num_faces, num_vertices, colors, atlas, texels, cols, (const int32_t*)nullptr, 0,
                     atlas ? cols * (texels + 1) : 0, rgb);
  MSLAM_LAUNCH_CHECK("mesh_shade");
  return MSLAM_OK;
}

// ---- the sized atlas ---------------------------------------------------------------------------------------------------
extern "C" int mslam_mesh_texture_classes(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                          double density, int floor_class, int cap_class, int32_t* cls,
                                          int32_t* clamped, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0 && 3 * (int64_t)num_faces < (1ll << 31),
                "mesh_texture_classes: negative size or faces outside the int32 index range");
  MSLAM_REQUIRE(density > 0.0 && density < INFINITY, "mesh_texture_classes: density must be a positive number");
  MSLAM_REQUIRE(0 <= floor_class && floor_class <= cap_class && cap_class < kTxClasses,
                "mesh_texture_classes: classes %d..%d are not within 0..%d in order", floor_class, cap_class,
                kTxClasses - 1);
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && cls && clamped && (vertices || num_vertices == 0), "mesh_texture_classes: null pointer");
  hipLaunchKernelGGL(tx_class_kernel, dim3(blocks_for(num_faces, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream,
                     vertices, faces, num_faces, num_vertices, density, floor_class, cap_class, cls, clamped);
  MSLAM_LAUNCH_CHECK("mesh_texture_classes");
  return MSLAM_OK;
}

extern "C" size_t mslam_mesh_texture_rank_table_ints(int num_faces) {
  return num_faces < 0 ? 0 : ((size_t)blocks_for(num_faces, kTxBlock) + 1) * kTxCols;
}

extern "C" int mslam_mesh_texture_rank(const int32_t* cls, const int32_t* clamped, int num_faces, int32_t* table,
                                       size_t table_ints, int32_t* rank, int32_t* order, int32_t* counts,
                                       void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && 3 * (int64_t)num_faces < (1ll << 31),
                "mesh_texture_rank: negative size or faces outside the int32 index range");
  MSLAM_REQUIRE(counts && table, "mesh_texture_rank: null pointer");
  MSLAM_REQUIRE(table_ints >= mslam_mesh_texture_rank_table_ints(num_faces),
                "mesh_texture_rank: the table holds %zu ints, %d faces need %zu", table_ints, num_faces,
                mslam_mesh_texture_rank_table_ints(num_faces));
  MSLAM_REQUIRE(num_faces == 0 || (cls && clamped && rank && order), "mesh_texture_rank: null pointer");
  const int nblk = (int)blocks_for(num_faces, kTxBlock);
  hipStream_t st = (hipStream_t)stream;
  if (nblk) {
    hipLaunchKernelGGL(tx_rank_count_kernel, dim3(nblk), dim3(kTxBlock), 0, st, cls, clamped, num_faces, table);
    MSLAM_LAUNCH_CHECK("mesh_texture_rank count");
  }
  hipLaunchKernelGGL(tx_rank_scan_kernel, dim3(1), dim3(kTxBlock), 0, st, nblk, table);
  MSLAM_LAUNCH_CHECK("mesh_texture_rank scan");
  // at least one block, so that the counts of a mesh without faces are written too
  hipLaunchKernelGGL(tx_rank_write_kernel, dim3(nblk ? nblk : 1), dim3(kTxBlock), 0, st, cls, num_faces, nblk, table,
                     rank, order, counts);
  MSLAM_LAUNCH_CHECK("mesh_texture_rank write");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_layout_sized(const int32_t* bands, int num_faces, int H, int W, const int32_t* cls,
                                               const int32_t* rank, const int32_t* order, int32_t* owner,
                                               int32_t* face_cell, void* stream) {
  TxBands bd;
  int n;
  if (!tx_bands_arg("mesh_texture_layout_sized", bands, num_faces, H, W, &bd, &n)) return MSLAM_EINVAL;
  if (num_faces == 0) return MSLAM_OK;           // then H = 0
  MSLAM_REQUIRE(cls && rank && order && owner && face_cell, "mesh_texture_layout_sized: null pointer");
  hipLaunchKernelGGL(tx_layout_sized_kernel, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, bd,
                     n, W, order, owner);
  MSLAM_LAUNCH_CHECK("mesh_texture_layout_sized owner");
  hipLaunchKernelGGL(tx_face_cell_kernel, dim3(blocks_for(num_faces, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream,
                     bd, num_faces, cls, rank, face_cell);
  MSLAM_LAUNCH_CHECK("mesh_texture_layout_sized face_cell");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_rays_sized(const float* vertices, const int32_t* faces, int num_faces,
                                             int num_vertices, const int32_t* owner, const int32_t* face_cell, int H,
                                             int W, const float* pose8, double fx, double fy, double cx, double cy,
                                             int h, int w, double near, double far, double cos_min, float* dir,
                                             double* r, double* cos, double* uv, void* stream) {
  TxSized at;
  int n;
  if (!tx_sized_arg("mesh_texture_rays_sized", owner, face_cell, num_faces, H, W, &at, &n)) return MSLAM_EINVAL;
  MSLAM_REQUIRE(num_vertices >= 0, "mesh_texture_rays_sized: negative size");
  MSLAM_REQUIRE(h >= 2 && w >= 2, "mesh_texture_rays_sized: an image must be at least 2x2, got %dx%d", h, w);
  if (int rc = view_check("mesh_texture_rays_sized", 1, h, w, nullptr, near, far, false)) return rc;
  MSLAM_REQUIRE(cos_min == cos_min, "mesh_texture_rays_sized: cos_min must not be NaN");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && pose8 && dir && r && cos && uv && (vertices || num_vertices == 0),
                "mesh_texture_rays_sized: null pointer");
  hipLaunchKernelGGL(tx_rays_kernel<TxSized>, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream, at,
                     n, vertices, faces, num_vertices, pose8, fx, fy, cx, cy, h, w, near, far, cos_min, dir, r, cos, uv);
  MSLAM_LAUNCH_CHECK("mesh_texture_rays_sized");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_texture_resolve_sized(const int32_t* faces, int num_faces, int num_vertices,
                                                const int32_t* owner, const int32_t* face_cell, int H, int W,
                                                const double* sums, const float* colors, double default_color,
                                                float* atlas, void* stream) {
  TxSized at;
  int n;
  if (!tx_sized_arg("mesh_texture_resolve_sized", owner, face_cell, num_faces, H, W, &at, &n)) return MSLAM_EINVAL;
  MSLAM_REQUIRE(num_vertices >= 0, "mesh_texture_resolve_sized: negative size");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && sums && atlas, "mesh_texture_resolve_sized: null pointer");
  hipLaunchKernelGGL(tx_resolve_kernel<TxSized>, dim3(blocks_for(n, kTxBlock)), dim3(kTxBlock), 0, (hipStream_t)stream,
                     at, n, faces, num_vertices, sums, colors, default_color, atlas);
  MSLAM_LAUNCH_CHECK("mesh_texture_resolve_sized");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_shade_sized(const int32_t* face, const float* rays, int h, int w, const float* pose8,
                                      const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                      const float* atlas, const int32_t* face_cell, int H, int W, float* rgb,
                                      void* stream) {
  if (int rc = view_check("mesh_shade_sized", 1, h, w, nullptr, 0.0, 0.0, false)) return rc;
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_shade_sized: negative size");
  MSLAM_REQUIRE(H >= 0 && W >= 0 && (int64_t)H * W < (1ll << 31), "mesh_shade_sized: bad atlas size %d x %d", H, W);
  MSLAM_REQUIRE(num_faces == 0 || (atlas && face_cell), "mesh_shade_sized: null atlas or face_cell");
  if (h == 0 || w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(face && rays && pose8 && rgb, "mesh_shade_sized: null pointer");
  MSLAM_REQUIRE(num_faces == 0 || (faces && (vertices || num_vertices == 0)), "mesh_shade_sized: null pointer");
  hipLaunchKernelGGL(tx_shade_kernel, view_grid(h, w), dim3(kMdBlock), 0, (hipStream_t)stream, face, rays, h, w, pose8,
                     vertices, faces, num_faces, num_vertices, (const float*)nullptr, atlas, 0, 0, face_cell, H, W, rgb);
  MSLAM_LAUNCH_CHECK("mesh_shade_sized");
  return MSLAM_OK;
}
