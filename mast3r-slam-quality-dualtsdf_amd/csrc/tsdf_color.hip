// Colour of the global sparse TSDF: a second caller-owned buffer beside the voxel hash, addressed by the SLOT INDEX of
// the table (csrc/tsdf_table.h, untouched), four 64-bit words per slot: sum_w, sum_wr, sum_wg, sum_wb.  A voxel has
// colour only if it is in the table, so the owner rule of a sharded table, overflow handling and kMaxProbe carry over
// with no second hash.  Semantics in DESIGN.md "Colour"; tests/color_numpy.py states the same in numpy.
//
//   fuse      one thread per (band position, point): the point's ray walk is shared with tsdf_emit_kernel
//             (csrc/tsdf_walk.h: one statement of the f32 operations; this TU is built with -ffp-contract=off too),
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
//   sample    one thread per point: trilinear colour on the mesh's and the view's lattice (tsdf_table.h lattice_cell),
//             corners without colour contribute the default colour.  Serves mesh vertices, view pixels and
//             sample_color().
#include "common.h"
#include "tsdf_walk.h"
#include "view.h"

namespace mslam {

constexpr double kColorWeightScale = 1048576.0;   // 2^20 units per unit of weight
constexpr int kColorWords = 4;

// Sample k of a point's walk: its weight in fixed point (0: nothing to add) and the slot of its voxel.  `step` tells a
// sample behind the band from the rest.
__device__ __forceinline__ unsigned long long color_sample(const TsdfTable& t, const RayWalk& ray, int k, double cf,
                                                           float vs, float truncf, uint64_t& slot, WalkStep& step) {
  WalkSample smp;
  step = walk_sample(ray, k, cf, vs, truncf, smp);
  if (step != kSampleOk) return 0ull;
  const int64_t s = table_find(t, smp.key);   // not in this table (another shard owns it, or the insert overflowed)
  if (s < 0) return 0ull;
  slot = (uint64_t)s;
  // weights beyond 2^53 units are not confidences any more; the bound only keeps the conversion defined
  return (unsigned long long)rint(fmin(smp.w * kColorWeightScale, 9007199254740992.0));
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
    RayWalk ray;
    if (walk_begin(points, (size_t)i, origin, stepf, truncf, ray) == kWalkOk) {   // no ray, or one the emit pass dropped
      const double cf = conf[i];
      const float cr = rgb[3 * (size_t)i], cg = rgb[3 * (size_t)i + 1], cb = rgb[3 * (size_t)i + 2];
      auto q8 = [](float c) { return (uint32_t)rintf(255.0f * fminf(fmaxf(c, 0.0f), 1.0f)); };   // NaN -> 0
      c8 = q8(cr) | (q8(cg) << 8) | (q8(cb) << 16);
      const int k = ray.k0 + j;
      WalkStep step;
      if (k < ray.num) wq = color_sample(t, ray, k, cf, vs, truncf, slot, step);
      if (j == band - 1) {
        // Samples past the last band position.  The in-band samples are a contiguous run that starts at most three
        // positions after k0 and is shorter than 2 trunc / step + 2, so usually none is left; the exact end point
        // (dist = maxd, k = num - 1) is the one that can lie further out.  Whatever is left is added here, one by one.
        for (int kk = k + 1; kk < ray.num; kk++) {
          uint64_t s2 = 0;
          const unsigned long long w2 = color_sample(t, ray, kk, cf, vs, truncf, s2, step);
          if (step == kSampleBehind && kk < ray.num - 1) kk = ray.num - 2;   // past the band: only the end point is left
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

__global__ __launch_bounds__(256) void color_sample_kernel(void* base, uint64_t cap,
                                                           const unsigned long long* __restrict__ color,
                                                           const float* __restrict__ pts, int n, int image_w, double vs,
                                                           double dr, double dg, double db, float* __restrict__ out_rgb,
                                                           uint8_t* __restrict__ out_count) {
  const TsdfTable t = table_carve(base, cap);
  size_t i;
  if (image_w > 0) {     // the points are the pixels of an image with rows of image_w
    int px, py;
    view_pixel(px, py);
    if (px >= image_w || py >= n / image_w) return;
    i = (size_t)py * image_w + px;
  } else {
    i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
  }
  const double dflt[3] = {dr, dg, db};
  const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
  double b[3], f[3];
  const bool ok = lattice_cell(p, vs, b, f);    // false for a non-finite point too
  double v[3][8];   // channel, corner
  int count = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int64_t s = -1;
    uint64_t key;
    if (ok && pack_key((long long)b[0] + corner_offset(c, 0), (long long)b[1] + corner_offset(c, 1),
                       (long long)b[2] + corner_offset(c, 2), key))
      s = table_find(t, key);
    // a corner has colour when its voxel is in the table and something was fused into it: not the valid-voxel rule
    const unsigned long long sw = s >= 0 ? color[(uint64_t)s * kColorWords] : 0ull;
    if (sw > 0ull) {
      const double den = 255.0 * (double)sw;
#pragma unroll
      for (int a = 0; a < 3; a++) v[a][c] = (double)color[(uint64_t)s * kColorWords + 1 + a] / den;
      count++;
    } else {
#pragma unroll
      for (int a = 0; a < 3; a++) v[a][c] = dflt[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) out_rgb[3 * i + a] = (float)(ok ? trilerp(v[a], f) : dflt[a]);
  out_count[i] = (uint8_t)count;
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_tsdf_color_bytes(uint64_t capacity) {
  if (!table_cap_ok(capacity)) return 0;
  return (size_t)capacity * kColorWords * sizeof(unsigned long long);
}

extern "C" int mslam_tsdf_color_init(void* color, size_t color_bytes, uint64_t capacity, void* stream) {
  MSLAM_REQUIRE(color, "tsdf_color_init: null buffer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_color_init: capacity must be a power of two in [2^10, 2^32]");
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
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_integrate_color: bad capacity");
  MSLAM_REQUIRE(voxel_size > 0 && trunc > 0, "tsdf_integrate_color: voxel_size and trunc must be positive");
  // band positions per point: the most samples a point can have in band, plus the up to three out-of-band samples the
  // walk starts early with, plus one
  const int band = max_band_for(voxel_size, trunc, step_scale) + 4;
  const long long threads = (long long)band * n_points;
  MSLAM_REQUIRE(threads <= 256ll * 0x7FFFFFFF, "tsdf_integrate_color: %lld x %d samples exceed the grid",
                (long long)n_points, band);
  hipLaunchKernelGGL(color_fuse_kernel, dim3(blocks_for(threads, 256)), dim3(256), 0, (hipStream_t)stream, table,
                     capacity, (unsigned long long*)color, points_world, conf, rgb, cam_origin, n_points, band,
                     (float)voxel_size, (float)integrate_step(voxel_size, step_scale), (float)trunc);
  MSLAM_LAUNCH_CHECK("tsdf_integrate_color");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_rehash(void* old_table, uint64_t old_capacity, const void* old_color, void* new_table,
                                       uint64_t new_capacity, void* new_color, void* stream) {
  MSLAM_REQUIRE(old_table && new_table && old_color && new_color && old_table != new_table && old_color != new_color,
                "tsdf_color_rehash: bad buffers");
  MSLAM_REQUIRE(table_cap_ok(old_capacity) && table_cap_ok(new_capacity) && new_capacity >= old_capacity,
                "tsdf_color_rehash: capacities must be powers of two, new >= old");
  hipLaunchKernelGGL(color_rehash_kernel, dim3(blocks_for(old_capacity, 256)), dim3(256), 0,
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
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_color_dump: bad capacity");
  hipLaunchKernelGGL(color_dump_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, table,
                     capacity, (const unsigned long long*)color, keys, n, (unsigned long long*)sums);
  MSLAM_LAUNCH_CHECK("tsdf_color_dump");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_color_load(void* table, uint64_t capacity, void* color, const int64_t* keys,
                                     const uint64_t* sums, int n, void* stream) {
  MSLAM_REQUIRE(n >= 0, "tsdf_color_load: negative count");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && color && keys && sums, "tsdf_color_load: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_color_load: bad capacity");
  hipLaunchKernelGGL(color_load_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, table,
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
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_color_sample: bad capacity");
  MSLAM_REQUIRE(voxel_size > 0.0, "tsdf_color_sample: voxel_size must be positive");
  MSLAM_REQUIRE(image_w >= 0 && (image_w == 0 || n % image_w == 0), "tsdf_color_sample: %d points are not rows of %d",
                n, image_w);
  const dim3 grid = image_w > 0 ? view_tile_grid(n / image_w, image_w)
                                : dim3(blocks_for(n, 256));
  hipLaunchKernelGGL(color_sample_kernel, grid, dim3(256), 0, (hipStream_t)stream, table, capacity,
                     (const unsigned long long*)color, points, n, image_w, voxel_size, default_r, default_g, default_b,
                     out_rgb, out_count);
  MSLAM_LAUNCH_CHECK("tsdf_color_sample");
  return MSLAM_OK;
}
