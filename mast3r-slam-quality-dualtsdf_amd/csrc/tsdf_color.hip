// Colour of the global sparse TSDF: a second caller-owned buffer beside the voxel hash, addressed by the SLOT INDEX of
// the table (csrc/tsdf_table.h, untouched), four 64-bit words per slot: sum_w, sum_wr, sum_wg, sum_wb.  A voxel has
// colour only if it is in the table, so the owner rule of a sharded table, overflow handling and kMaxProbe carry over
// with no second hash.  Semantics in DESIGN.md "Colour"; tests/color_numpy.py states the same in numpy.
//
//   fuse      one thread per (band position, point): the point's ray walk is restated from tsdf_emit_kernel
//             (csrc/tsdf_global.hip, same f32 operations in the same order: this TU is built with -ffp-contract=off too),
//             thread j looks at sample k0 + j only.  In-band samples find their voxel (read only) and add
//             wq = rint(w * 2^20) and wq * c8 (c8 = rint(255 c), 8 bit) to the voxel's four words.
//   The sums are INTEGERS: the result does not depend on the order of arrival, so colour is bit-identical for any
//   schedule, capacity and shard count without the TSDF's sort-and-replay pass.  A word overflows after
//   2^64 / (255 * 2^20) = 6.9e10 units of summed weight in one voxel (a keyframe adds a few hundred at most).
//   There is no weight cap: a voxel's colour is the weighted mean of everything ever fused into it.
//   Launch shape: consecutive lanes are consecutive points at the same band position (coalesced point loads, 3 750
//   workgroups for 40 000 points x 24 positions: every CU is busy, no counter on a single address).  The four words of a
//   sample are added by four neighbouring lanes after a quad exchange, so one wave instruction carries 16 segments of
//   32 contiguous bytes instead of 64 single words in 64 rows; the adds are non-returning device-scope
//   global_atomic_add_x2.
//   sample    one thread per point: trilinear colour on the mesh's and the view's lattice (g = p / vs - 0.5), corners
//             without colour contribute the default colour.  Serves mesh vertices, view pixels and sample_color().
#include "common.h"
#include "tsdf_table.h"

namespace mslam {

constexpr double kColorWeightScale = 1048576.0;   // 2^20 units per unit of weight
constexpr int kColorWords = 4;

// One sample of one point, exactly as tsdf_emit_kernel sees it: returns the weight in fixed point (0: nothing to add)
// and the slot of its voxel.
__device__ __forceinline__ unsigned long long color_sample(const TsdfTable& t, float o0, float o1, float o2, float d0,
                                                           float d1, float d2, float L, float maxd, float lstep, int num,
                                                           int k, double cf, float vs, float truncf, uint64_t& slot) {
  float dist;
  if (num == 1) dist = 0.0f;
  else if (k == num - 1) dist = maxd;
  else dist = (float)k * lstep;
  const float sdf = L - dist;
  if (fabsf(sdf) > truncf) return 0ull;
  const float s0 = o0 + dist * d0, s1 = o1 + dist * d1, s2 = o2 + dist * d2;
  const float e = -fabsf(sdf) / truncf;
  const double w = cf * exp((double)e);
  if (!(w > 0.0)) return 0ull;
  uint64_t key;
  if (!world_to_key(s0, s1, s2, vs, key)) return 0ull;   // tsdf_table.h: the key function of the emit pass
  const int64_t s = table_find(t, key);     // not in this table (another shard owns it, or the insert overflowed)
  if (s < 0) return 0ull;
  slot = (uint64_t)s;
  // weights beyond 2^53 units are not confidences any more; the bound only keeps the conversion defined
  return (unsigned long long)rint(fmin(w * kColorWeightScale, 9007199254740992.0));
}

__global__ __launch_bounds__(256) void color_fuse_kernel(void* base, uint64_t cap, unsigned long long* __restrict__ color,
                                                         const float* __restrict__ points,
                                                         const double* __restrict__ conf,
                                                         const float* __restrict__ rgb,
                                                         const float* __restrict__ origin, int n, int band, float vs,
                                                         float stepf, float truncf) {
  const TsdfTable t = table_carve(base, cap);
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int j = (int)(tid / n);             // band position; the grid covers band * n threads, rounded up to a wave
  const int i = (int)(tid - (long long)j * n);
  unsigned long long wq = 0ull;             // this lane's sample: weight units, slot, packed 8-bit colour
  uint64_t slot = 0;
  uint32_t c8 = 0;
  if (j < band) {
    const float o0 = origin[0], o1 = origin[1], o2 = origin[2];
    const float r0 = points[3 * (size_t)i] - o0, r1 = points[3 * (size_t)i + 1] - o1, r2 = points[3 * (size_t)i + 2] - o2;
    const float sq = (float)(((double)(r0 * r0) + (double)(r1 * r1)) + (double)(r2 * r2));
    const float L = sqrtf(sq);
    const float maxd = L + truncf;
    if (isfinite(L) && !(L < 1.0e-4f) && maxd / stepf < 1048576.0f) {
      const float d0 = r0 / L, d1 = r1 / L, d2 = r2 / L;
      int num = (int)(maxd / stepf);
      if (num < 1) num = 1;
      const float lstep = num > 1 ? maxd / (float)(num - 1) : 0.0f;
      int k0 = num > 1 ? (int)((L - truncf) / lstep) - 2 : 0;
      if (k0 < 0) k0 = 0;
      const double cf = conf[i];
      const float cr = rgb[3 * (size_t)i], cg = rgb[3 * (size_t)i + 1], cb = rgb[3 * (size_t)i + 2];
      auto q8 = [](float c) { return (uint32_t)rintf(255.0f * fminf(fmaxf(c, 0.0f), 1.0f)); };   // NaN -> 0
      c8 = q8(cr) | (q8(cg) << 8) | (q8(cb) << 16);
      const int k = k0 + j;
      if (k < num) wq = color_sample(t, o0, o1, o2, d0, d1, d2, L, maxd, lstep, num, k, cf, vs, truncf, slot);
      if (j == band - 1) {
        // Samples past the last band position.  The in-band samples are a contiguous run that starts at most three
        // positions after k0 and is shorter than 2 trunc / step + 2, so usually none is left; the exact end point
        // (dist = maxd, k = num - 1) is the one that can lie further out.  Whatever is left is added here, one by one.
        for (int kk = k + 1; kk < num; kk++) {
          if (kk < num - 1 && L - (float)kk * lstep < -truncf) kk = num - 1;   // past the band: only the end point is left
          uint64_t s2 = 0;
          const unsigned long long w2 = color_sample(t, o0, o1, o2, d0, d1, d2, L, maxd, lstep, num, kk, cf, vs, truncf, s2);
          if (w2 == 0ull) continue;
          unsigned long long* dst = color + s2 * kColorWords;
          atomicAdd(dst, w2);
          atomicAdd(dst + 1, w2 * (unsigned long long)(c8 & 255u));
          atomicAdd(dst + 2, w2 * (unsigned long long)((c8 >> 8) & 255u));
          atomicAdd(dst + 3, w2 * (unsigned long long)(c8 >> 16));
        }
      }
    }
  }
  // quad exchange: in round r the four lanes of a quad add the four words of the sample held by the quad's lane r
  const int lane = threadIdx.x & 63, word = lane & 3, quad = lane & ~3;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const unsigned long long w = __shfl(wq, quad + r, 64);
    const unsigned long long s = __shfl((unsigned long long)slot, quad + r, 64);
    const uint32_t c = __shfl(c8, quad + r, 64);
    if (w == 0ull) continue;
    const unsigned long long f = word == 0 ? 1ull : (unsigned long long)((c >> (8 * (word - 1))) & 255u);
    if (f == 0ull) continue;                 // a zero channel adds nothing
    atomicAdd(color + s * kColorWords + word, w * f);
  }
}

__global__ __launch_bounds__(256) void color_rehash_kernel(void* old_base, uint64_t old_cap,
                                                           const unsigned long long* __restrict__ old_color,
                                                           void* new_base, uint64_t new_cap,
                                                           unsigned long long* __restrict__ new_color) {
  const TsdfTable a = table_carve(old_base, old_cap), b = table_carve(new_base, new_cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= old_cap) return;
  const uint64_t key = a.keys[i];
  if (key == kEmptyKey) return;
  const int64_t s = table_find(b, key);
  if (s < 0) return;                         // the table rehash overflowed and said so in its header
#pragma unroll
  for (int c = 0; c < kColorWords; c++) new_color[(uint64_t)s * kColorWords + c] = old_color[i * kColorWords + c];
}

// keyed read / write of the sums: one thread per key
__global__ __launch_bounds__(256) void color_dump_kernel(void* base, uint64_t cap,
                                                         const unsigned long long* __restrict__ color,
                                                         const int64_t* __restrict__ keys, int n,
                                                         unsigned long long* __restrict__ sums) {
  const TsdfTable t = table_carve(base, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t key;
  int64_t s = -1;
  if (pack_key(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2], key)) s = table_find(t, key);
#pragma unroll
  for (int c = 0; c < kColorWords; c++) sums[(size_t)i * kColorWords + c] = s >= 0 ? color[(uint64_t)s * kColorWords + c] : 0ull;
}

__global__ __launch_bounds__(256) void color_load_kernel(void* base, uint64_t cap, unsigned long long* __restrict__ color,
                                                         const int64_t* __restrict__ keys,
                                                         const unsigned long long* __restrict__ sums, int n) {
  const TsdfTable t = table_carve(base, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t key;
  if (!pack_key(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2], key)) return;
  const int64_t s = table_find(t, key);
  if (s < 0) return;
#pragma unroll
  for (int c = 0; c < kColorWords; c++) color[(uint64_t)s * kColorWords + c] = sums[(size_t)i * kColorWords + c];
}

__device__ __forceinline__ double color_lerp(double a, double b, double f) { return a + f * (b - a); }

__global__ __launch_bounds__(256) void color_sample_kernel(void* base, uint64_t cap,
                                                           const unsigned long long* __restrict__ color,
                                                           const float* __restrict__ pts, int n, int image_w, double vs,
                                                           double dr, double dg, double db, float* __restrict__ out_rgb,
                                                           uint8_t* __restrict__ out_count) {
  const TsdfTable t = table_carve(base, cap);
  size_t i;
  if (image_w > 0) {     // the points are the pixels of an image with rows of image_w: 16x16 per block, 8x8 per wave
    const int h = n / image_w;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (px >= image_w || py >= h) return;
    i = (size_t)py * image_w + px;
  } else {
    i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
  }
  const double dflt[3] = {dr, dg, db};
  double b[3], f[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double g = (double)pts[3 * i + a] / vs - 0.5;
    b[a] = floor(g);
    f[a] = g - b[a];
    ok = ok && fabs(b[a]) < (double)kKeyBias;    // false for a non-finite point too
  }
  double v[8][3];
  int count = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int64_t s = -1;
    uint64_t key;
    if (ok && pack_key((long long)b[0] + (c & 1), (long long)b[1] + ((c >> 1) & 1), (long long)b[2] + ((c >> 2) & 1), key))
      s = table_find(t, key);
    const unsigned long long sw = s >= 0 ? color[(uint64_t)s * kColorWords] : 0ull;
    if (sw > 0ull) {
      const double den = 255.0 * (double)sw;
#pragma unroll
      for (int a = 0; a < 3; a++) v[c][a] = (double)color[(uint64_t)s * kColorWords + 1 + a] / den;
      count++;
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) v[c][a] = dflt[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double r = dflt[a];
    if (ok) {
      const double c00 = color_lerp(v[0][a], v[1][a], f[0]), c10 = color_lerp(v[2][a], v[3][a], f[0]);
      const double c01 = color_lerp(v[4][a], v[5][a], f[0]), c11 = color_lerp(v[6][a], v[7][a], f[0]);
      r = color_lerp(color_lerp(c00, c10, f[1]), color_lerp(c01, c11, f[1]), f[2]);
    }
    out_rgb[3 * i + a] = (float)r;
  }
  out_count[i] = (uint8_t)count;
}

static bool color_cap_ok(uint64_t capacity) {
  return capacity >= 1024 && (capacity & (capacity - 1)) == 0 && capacity <= (1ull << 32);
}

// band positions per point: tsdf_global.hip max_band_for (the most samples a point can have in band) plus the up to
// three out-of-band samples the walk starts early with, plus one
static int color_band_for(double voxel_size, double trunc, double step_scale) {
  double step = voxel_size * step_scale;
  if (step < 1.0e-4) step = 1.0e-4;
  return (int)(2.0 * trunc / step) + 8;
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_tsdf_color_bytes(uint64_t capacity) {
  if (!color_cap_ok(capacity)) return 0;
  return (size_t)capacity * kColorWords * sizeof(unsigned long long);
}

extern "C" int mslam_tsdf_color_init(void* color, size_t color_bytes, uint64_t capacity, void* stream) {
  MSLAM_REQUIRE(color, "tsdf_color_init: null buffer");
  MSLAM_REQUIRE(color_cap_ok(capacity), "tsdf_color_init: capacity must be a power of two in [2^10, 2^32]");
  MSLAM_REQUIRE(color_bytes >= mslam_tsdf_color_bytes(capacity), "tsdf_color_init: buffer too small for %llu slots",
                (unsigned long long)capacity);
  return check_hip(hipMemsetAsync(color, 0, mslam_tsdf_color_bytes(capacity), (hipStream_t)stream), "tsdf_color_init");
}

extern "C" int mslam_tsdf_integrate_color(void* table, uint64_t capacity, void* color, const float* points_world,
                                          const double* conf, const float* rgb, const float* cam_origin, int n_points,
                                          double voxel_size, double trunc, double step_scale, void* stream) {
  MSLAM_REQUIRE(n_points >= 0, "tsdf_integrate_color: negative point count");
  if (n_points == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && color && points_world && conf && rgb && cam_origin, "tsdf_integrate_color: null pointer");
  MSLAM_REQUIRE(color_cap_ok(capacity), "tsdf_integrate_color: bad capacity");
  MSLAM_REQUIRE(voxel_size > 0 && trunc > 0, "tsdf_integrate_color: voxel_size and trunc must be positive");
  double step = voxel_size * step_scale;
  if (step < 1.0e-4) step = 1.0e-4;
  const int band = color_band_for(voxel_size, trunc, step_scale);
  const long long threads = (long long)band * n_points;
  const long long blocks = (threads + 255) / 256;
  MSLAM_REQUIRE(blocks < (1ll << 31), "tsdf_integrate_color: %lld x %d samples exceed the grid", (long long)n_points, band);
  hipLaunchKernelGGL(color_fuse_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, capacity,
                     (unsigned long long*)color, points_world, conf, rgb, cam_origin, n_points, band, (float)voxel_size,
                     (float)step, (float)trunc);
  MSLAM_LAUNCH_CHECK("tsdf_integrate_color");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_rehash(void* old_table, uint64_t old_capacity, const void* old_color, void* new_table,
                                       uint64_t new_capacity, void* new_color, void* stream) {
  MSLAM_REQUIRE(old_table && new_table && old_color && new_color && old_table != new_table && old_color != new_color,
                "tsdf_color_rehash: bad buffers");
  MSLAM_REQUIRE(color_cap_ok(old_capacity) && color_cap_ok(new_capacity) && new_capacity >= old_capacity,
                "tsdf_color_rehash: capacities must be powers of two, new >= old");
  hipLaunchKernelGGL(color_rehash_kernel, dim3((unsigned)((old_capacity + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, old_table, old_capacity, (const unsigned long long*)old_color, new_table,
                     new_capacity, (unsigned long long*)new_color);
  MSLAM_LAUNCH_CHECK("tsdf_color_rehash");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_dump(void* table, uint64_t capacity, const void* color, const int64_t* keys, int n,
                                     uint64_t* sums, void* stream) {
  MSLAM_REQUIRE(n >= 0, "tsdf_color_dump: negative count");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && color && keys && sums, "tsdf_color_dump: null pointer");
  MSLAM_REQUIRE(color_cap_ok(capacity), "tsdf_color_dump: bad capacity");
  hipLaunchKernelGGL(color_dump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table,
                     capacity, (const unsigned long long*)color, keys, n, (unsigned long long*)sums);
  MSLAM_LAUNCH_CHECK("tsdf_color_dump");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_load(void* table, uint64_t capacity, void* color, const int64_t* keys,
                                     const uint64_t* sums, int n, void* stream) {
  MSLAM_REQUIRE(n >= 0, "tsdf_color_load: negative count");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && color && keys && sums, "tsdf_color_load: null pointer");
  MSLAM_REQUIRE(color_cap_ok(capacity), "tsdf_color_load: bad capacity");
  hipLaunchKernelGGL(color_load_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table,
                     capacity, (unsigned long long*)color, keys, (const unsigned long long*)sums, n);
  MSLAM_LAUNCH_CHECK("tsdf_color_load");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_sample(void* table, uint64_t capacity, const void* color, const float* points, int n,
                                       int image_w, double voxel_size, double default_r, double default_g,
                                       double default_b, float* out_rgb, uint8_t* out_count, void* stream) {
  MSLAM_REQUIRE(n >= 0, "tsdf_color_sample: negative count");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && color && points && out_rgb && out_count, "tsdf_color_sample: null pointer");
  MSLAM_REQUIRE(color_cap_ok(capacity), "tsdf_color_sample: bad capacity");
  MSLAM_REQUIRE(voxel_size > 0.0, "tsdf_color_sample: voxel_size must be positive");
  MSLAM_REQUIRE(image_w >= 0 && (image_w == 0 || n % image_w == 0), "tsdf_color_sample: %d points are not rows of %d",
                n, image_w);
  const dim3 grid = image_w > 0 ? dim3((unsigned)((image_w + 15) / 16), (unsigned)((n / image_w + 15) / 16))
                                : dim3((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(color_sample_kernel, grid, dim3(256), 0, (hipStream_t)stream, table, capacity,
                     (const unsigned long long*)color, points, n, image_w, voxel_size, default_r, default_g, default_b,
                     out_rgb, out_count);
  MSLAM_LAUNCH_CHECK("tsdf_color_sample");
  return MSLAM_OK;
}
