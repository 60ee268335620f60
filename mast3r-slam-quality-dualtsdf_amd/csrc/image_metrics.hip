// Render quality: PSNR and SSIM (Wang et al. 2004: 11-tap Gaussian window, sigma 1.5, K1 0.01, K2 0.03, data range 1)
// of image pairs f32[n,h,w,c] under an optional pixel mask, in one pass over the images.  The definition is
// tests/imgmetrics_numpy.py; DESIGN.md "Render quality" states the design.
//
// One 256-thread workgroup owns a kTH x kTW tile of window centres of one image (grid.z).  Per channel it stages the
// tile plus a 5-pixel halo of a and b (f32) in LDS, the row pass leaves the five window moments (a, b, aa, bb, ab) of
// every halo row in LDS as f64, the column pass turns them into S at the tile's centres.  The mask is staged once, as
// 0 outside the image, and a centre is valid when the separable AND of its 11x11 mask pixels holds: a window that
// leaves the image or touches a masked-out pixel is invalid, so halo loads are clamped into the image (no load leaves
// the allocation) and what they fetch reaches invalid centres only.  The squared error of the tile's own masked-in
// pixels is taken from the staged values in the same pass.
//
// Reduction: wave64 shuffle tree, the four waves in order through LDS, one partial per workgroup and quantity into the
// workspace, and a second launch that adds an image's partials in block order.  No atomics; counts are integers.
#include "common.h"

namespace {

using namespace mslam;

constexpr int kTH = MSLAM_IMAGE_METRICS_TILE_H;
constexpr int kTW = MSLAM_IMAGE_METRICS_TILE_W;
constexpr int kR = 5;                   // window radius
constexpr int kTaps = 2 * kR + 1;
constexpr int kHH = kTH + 2 * kR;       // halo tile
constexpr int kHW = kTW + 2 * kR;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPer = kTH * kTW / kThreads;   // centres per thread
constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;
static_assert(kTH * kTW % kThreads == 0, "a whole number of centres per thread");

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// part_sums f64[n, tiles, 2], part_counts i64[n, tiles, 2]; tiles = gridDim.x * gridDim.y, tile = by * gridDim.x + bx
__global__ __launch_bounds__(kThreads) void image_metrics_tile_kernel(
    const float* __restrict__ a, const float* __restrict__ b, const uint8_t* __restrict__ mask, int h, int w, int c,
    const double* __restrict__ window, double* __restrict__ part_sums, long long* __restrict__ part_counts,
    float* __restrict__ ssim_map) {
  __shared__ double s_mom[5][kHH][kTW];       // row-pass moments of the halo rows
  __shared__ float s_a[kHH][kHW], s_b[kHH][kHW];
  __shared__ uint8_t s_m[kHH][kHW];           // mask, 0 outside the image
  __shared__ uint8_t s_rowok[kHH][kTW];       // AND of the 11 mask pixels to the right of (row, col)
  __shared__ double s_red[2][kWaves];
  __shared__ long long s_cnt[2][kWaves];

  const int t = threadIdx.x;
  const int img = blockIdx.z;
  const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
  const int64_t plane = (int64_t)img * h * w;

  double g[kTaps];
#pragma unroll
  for (int k = 0; k < kTaps; ++k) g[k] = window[k];

  double s_sum[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) s_sum[j] = 0.0;
  bool valid[kPer] = {};
  double se = 0.0;
  long long n_pix = 0;

  for (int ch = 0; ch < c; ++ch) {
    for (int i = t; i < kHH * kHW; i += kThreads) {
      const int ry = i / kHW, rx = i % kHW;
      const int gy = y0 - kR + ry, gx = x0 - kR + rx;
      const bool inside = gy >= 0 && gy < h && gx >= 0 && gx < w;
      const int cy = min(max(gy, 0), h - 1), cx = min(max(gx, 0), w - 1);
      const int64_t pix = plane + (int64_t)cy * w + cx;
      s_a[ry][rx] = a[pix * c + ch];
      s_b[ry][rx] = b[pix * c + ch];
      if (ch == 0) s_m[ry][rx] = (inside && (mask == nullptr || mask[pix] != 0)) ? 1 : 0;
    }
    __syncthreads();
    for (int i = t; i < kHH * kTW; i += kThreads) {
      const int r = i / kTW, col = i % kTW;
      double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
      unsigned ok = 1;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const double x = (double)s_a[r][col + k], y = (double)s_b[r][col + k];
        ma += g[k] * x;
        mb += g[k] * y;
        maa += g[k] * (x * x);
        mbb += g[k] * (y * y);
        mab += g[k] * (x * y);
        ok &= s_m[r][col + k];
      }
      s_mom[0][r][col] = ma;
      s_mom[1][r][col] = mb;
      s_mom[2][r][col] = maa;
      s_mom[3][r][col] = mbb;
      s_mom[4][r][col] = mab;
      if (ch == 0) s_rowok[r][col] = (uint8_t)ok;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {           // the squared error of the tile's own pixels
      const int p = t + j * kThreads, r = p / kTW + kR, col = p % kTW + kR;
      if (s_m[r][col]) {
        const double d = (double)s_a[r][col] - (double)s_b[r][col];
        se += d * d;
        if (ch == 0) ++n_pix;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int p = t + j * kThreads, r = p / kTW, col = p % kTW;
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      unsigned ok = 1;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += g[k] * s_mom[q][r + k][col];
        ok &= s_rowok[r + k][col];
      }
      if (ch == 0) valid[j] = ok != 0;
      const double mu_ab = m[0] * m[1], mu_aa = m[0] * m[0], mu_bb = m[1] * m[1];
      const double va = m[2] - mu_aa, vb = m[3] - mu_bb, cab = m[4] - mu_ab;
      const double num = (2.0 * mu_ab + kC1) * (2.0 * cab + kC2);
      const double den = (mu_aa + mu_bb + kC1) * (va + vb + kC2);
      s_sum[j] += num / den;
    }
    __syncthreads();                           // the next channel restages s_a / s_b / s_mom
  }

  double s_tot = 0.0;
  long long n_win = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int p = t + j * kThreads;
    const int y = y0 + p / kTW, x = x0 + p % kTW;
    if (valid[j]) {
      s_tot += s_sum[j];
      ++n_win;
    }
    if (ssim_map != nullptr && y < h && x < w)
      ssim_map[plane + (int64_t)y * w + x] = valid[j] ? (float)(s_sum[j] / (double)c) : __builtin_nanf("");
  }

  se = wave_sum(se);
  s_tot = wave_sum(s_tot);
  n_pix = wave_sum_i64(n_pix);
  n_win = wave_sum_i64(n_win);
  const int wave = t / kWave;
  if (t % kWave == 0) {
    s_red[0][wave] = se;
    s_red[1][wave] = s_tot;
    s_cnt[0][wave] = n_pix;
    s_cnt[1][wave] = n_win;
  }
  __syncthreads();
  if (t == 0) {
    double r0 = s_red[0][0], r1 = s_red[1][0];
    long long c0 = s_cnt[0][0], c1 = s_cnt[1][0];
    for (int k = 1; k < kWaves; ++k) {
      r0 += s_red[0][k];
      r1 += s_red[1][k];
      c0 += s_cnt[0][k];
      c1 += s_cnt[1][k];
    }
    const int64_t tiles = (int64_t)gridDim.x * gridDim.y;
    const int64_t slot = ((int64_t)img * tiles + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    part_sums[slot] = r0;
    part_sums[slot + 1] = r1;
    part_counts[slot] = c0;
    part_counts[slot + 1] = c1;
  }
}

// One workgroup per image; threads 0..3 each add one quantity's partials in block order.
__global__ __launch_bounds__(kWave) void image_metrics_sum_kernel(const double* __restrict__ part_sums,
                                                                  const long long* __restrict__ part_counts,
                                                                  int64_t tiles, double* __restrict__ sums,
                                                                  long long* __restrict__ counts) {
  const int img = blockIdx.x, q = threadIdx.x;
  if (q < 2) {
    const double* p = part_sums + (int64_t)img * tiles * 2 + q;
    double acc = 0.0;
    for (int64_t i = 0; i < tiles; ++i) acc += p[2 * i];
    sums[2 * img + q] = acc;
  } else if (q < 4) {
    const long long* p = part_counts + (int64_t)img * tiles * 2 + (q - 2);
    long long acc = 0;
    for (int64_t i = 0; i < tiles; ++i) acc += p[2 * i];
    counts[2 * img + (q - 2)] = acc;
  }
}

// tiles per image, or 0 for a shape the entry points refuse
int64_t image_metrics_tiles(int n, int h, int w, int c, unsigned* tx, unsigned* ty) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || c < 1 || c > 4) return 0;
  const int64_t x = ((int64_t)w + kTW - 1) / kTW, y = ((int64_t)h + kTH - 1) / kTH;
  if (y > 65535) return 0;
  if (tx) *tx = (unsigned)x;
  if (ty) *ty = (unsigned)y;
  return x * y;
}

}  // namespace

extern "C" size_t mslam_image_metrics_workspace_bytes(int n, int h, int w, int c) {
  const int64_t tiles = image_metrics_tiles(n, h, w, c, nullptr, nullptr);
  return (size_t)n * (size_t)tiles * 2 * (sizeof(double) + sizeof(long long));
}

extern "C" int mslam_image_metrics(const float* a, const float* b, const uint8_t* mask, int n, int h, int w, int c,
                                   const double* window, double* sums, int64_t* counts, float* ssim_map, void* workspace,
                                   void* stream) {
  MSLAM_REQUIRE(n >= 1, "image_metrics: n must be at least 1, got %d", n);
  MSLAM_REQUIRE(h >= 1 && w >= 1, "image_metrics: h and w must be at least 1, got %d x %d", h, w);
  MSLAM_REQUIRE(c >= 1 && c <= 4, "image_metrics: c must be in 1..4, got %d", c);
  MSLAM_REQUIRE(a && b && window && sums && counts && workspace, "image_metrics: null pointer");
  unsigned tx = 0, ty = 0;
  const int64_t tiles = image_metrics_tiles(n, h, w, c, &tx, &ty);
  MSLAM_REQUIRE(tiles > 0, "image_metrics: %d images of %d rows exceed the grid", n, h);
  double* part_sums = (double*)workspace;
  long long* part_counts = (long long*)(part_sums + (int64_t)n * tiles * 2);
  hipLaunchKernelGGL(image_metrics_tile_kernel, dim3(tx, ty, (unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, a, b,
                     mask, h, w, c, window, part_sums, part_counts, ssim_map);
  MSLAM_LAUNCH_CHECK("image_metrics");
  hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream,
                     (const double*)part_sums, (const long long*)part_counts, tiles, sums, (long long*)counts);
  MSLAM_LAUNCH_CHECK("image_metrics");
  return MSLAM_OK;
}
