// Depth / normal view of the global sparse TSDF by ray casting the live voxel hash.  Semantics in DESIGN.md "View
// rendering"; tests/render_numpy.py states the same march in numpy.
//
//   blocks    one thread per slot: every valid voxel (present, fused, weight >= min_weight) inserts the key of its
//             8^3-voxel block into a hash set in the workspace (64-bit CAS on the block's own slot; no counter on one
//             address).  A set that cannot take a block raises a flag word and the march then skips nothing.
//   render    one thread per ray, 8x8 pixels per wave (2x2 waves per 256-thread block) so a wave's rays probe
//             neighbouring voxels.  Samples k = 0, 1, ... at t_k = near + k * step; the 8 corner values of the current
//             cell stay in registers and are probed again only when the cell changes; the first valid pair of samples
//             that goes from >= level to < level is the hit.
// Empty-space skipping.  A sample at p reads the corners base + {0,1}^3, base = floor(p / vs - 0.5), and is valid only
// if all 8 are: in particular `base` itself.  Blocks are therefore taken on the SAMPLE lattice - the block of a sample is
// base >> 3, the cube p / vs - 0.5 in [8B, 8B + 8) - and a sample that could be valid lies in a marked block with no
// dilation at all.  In an unmarked block the march jumps to the last sample index that is still in that block.  Every
// coordinate of base(k) is a monotone function of k in floating point (rounding keeps order), so when base(k) and
// base(j) lie in one block every index between them does too: the jump target is estimated from the block's exit
// distance and then CHECKED by evaluating base(j); only samples that are invalid anyway are left out, and the output
// equals the brute-force march bit for bit.  k stays the integer sample index; t is never accumulated.
// Nothing here writes the table.
#include "common.h"
#include "tsdf_table.h"
#include "view.h"

namespace mslam {

constexpr int kBlockShift = 3;              // blocks of 8^3 voxels
constexpr int kBlockBias = kKeyBias >> kBlockShift;
constexpr uint64_t kMaxSamples = 1u << 30;  // per ray

struct RenderHeader {
  uint32_t overflow;  // != 0: the block set is full, the march must not skip
};

struct BlockSet {
  RenderHeader* hdr;
  uint64_t* keys;  // [cap] packed block keys, kEmptyKey elsewhere
  uint64_t cap;    // power of two
  size_t bytes;
};

// a quarter of the table's slots: a fused surface band puts tens of voxels into every block it meets
__host__ __device__ inline BlockSet blocks_carve(void* base, uint64_t table_cap) {
  BlockSet b;
  b.cap = table_cap / 4 < 1024 ? 1024 : table_cap / 4;
  b.hdr = (RenderHeader*)base;
  b.keys = (uint64_t*)((char*)base + 256);
  b.bytes = 256 + (b.cap * 8 + 255) / 256 * 256;
  return b;
}

// block coordinates are voxel coordinates >> 3, in [-2^17, 2^17): 3 x 18 bits
__device__ __forceinline__ uint64_t pack_block(long long bx, long long by, long long bz) {
  return ((uint64_t)(bx + kBlockBias) << 36) | ((uint64_t)(by + kBlockBias) << 18) | (uint64_t)(bz + kBlockBias);
}

__global__ __launch_bounds__(256) void render_blocks_kernel(void* base, uint64_t cap, double min_weight, BlockSet B) {
  const TsdfTable t = table_carve(base, cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const uint64_t k = t.keys[i];
  if (k == kEmptyKey || !voxel_valid(t, (int64_t)i, min_weight)) return;
  long long x, y, z;
  unpack_key(k, x, y, z);
  const uint64_t bk = pack_block(x >> kBlockShift, y >> kBlockShift, z >> kBlockShift);
  bool inserted;
  // most voxels find their block already there: read first, no atomic
  if (probe_insert<kInsertReadFirst>(B.keys, B.cap, bk, inserted) < 0) B.hdr->overflow = 1u;
}

// a miss after kMaxProbe slots is not reached when the set did not overflow (an insert that probed this far raised the flag)
__device__ __forceinline__ bool block_marked(const BlockSet& B, uint64_t bk) { return probe_find(B.keys, B.cap, bk) >= 0; }

struct Ray {
  double o[3], d[3];
  double near, step, vs;
};

// sample k: its cell on the sample lattice (tsdf_table.h lattice_cell); false when the position is not finite or outside
// the key range (such a sample is invalid)
__device__ __forceinline__ bool sample_cell(const Ray& r, int k, double (&b)[3], double (&f)[3]) {
  const double tk = r.near + (double)k * r.step;
  const double p[3] = {r.o[0] + tk * r.d[0], r.o[1] + tk * r.d[1], r.o[2] + tk * r.d[2]};
  return lattice_cell(p, r.vs, b, f);
}

struct Cell {
  int x, y, z;
  double v[8];   // corner c = dx + 2 dy + 4 dz
  bool loaded, valid;
};

__device__ __forceinline__ void cell_load(const TsdfTable& t, double min_weight, int x, int y, int z,
                                          Cell& c) {
  if (c.loaded && c.x == x && c.y == y && c.z == z) return;
  c.x = x; c.y = y; c.z = z; c.loaded = true; c.valid = true;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (!c.valid) break;                     // one missing corner settles it: the sample is invalid
    // base is inside the key range; base + 1 may step out of it at the upper end
    const int64_t s = find_valid(t, x + corner_offset(i, 0), y + corner_offset(i, 1), z + corner_offset(i, 2), min_weight);
    if (s >= 0) c.v[i] = t.tsdf[s];
    else c.valid = false;
  }
}

__device__ __forceinline__ double cell_value(const Cell& c, const double (&f)[3]) { return trilerp(c.v, f); }

// analytic gradient of the trilinear interpolant
__device__ __forceinline__ void cell_gradient(const Cell& c, const double (&f)[3], double vs, double (&g)[3]) {
  const double c00 = lerp(c.v[0], c.v[1], f[0]), c10 = lerp(c.v[2], c.v[3], f[0]);
  const double c01 = lerp(c.v[4], c.v[5], f[0]), c11 = lerp(c.v[6], c.v[7], f[0]);
  const double c0 = lerp(c00, c10, f[1]), c1 = lerp(c01, c11, f[1]);
  g[0] = lerp(lerp(c.v[1] - c.v[0], c.v[3] - c.v[2], f[1]), lerp(c.v[5] - c.v[4], c.v[7] - c.v[6], f[1]), f[2]) / vs;
  g[1] = lerp(c10 - c00, c11 - c01, f[2]) / vs;
  g[2] = (c1 - c0) / vs;
}

// last sample index j in (k, kmax] that still lies in block (bx, by, bz) of sample k, or k: estimated from the distance
// at which the ray leaves the block, kept only when base(j) confirms it (see the note on monotonicity above)
__device__ __forceinline__ int block_last_sample(const Ray& r, int k, int kmax, int bx,
                                                       int by, int bz) {
  const int bb[3] = {bx, by, bz};
  double t_exit = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (r.d[a] == 0.0) continue;
    const double face = ((double)((bb[a] + (r.d[a] > 0.0 ? 1 : 0)) * (1 << kBlockShift)) + 0.5) * r.vs;
    const double te = (face - r.o[a]) / r.d[a];
    t_exit = te < t_exit ? te : t_exit;
  }
  const double x = floor((t_exit - r.near) / r.step);
  if (!(x > (double)k)) return k;
  int j = x >= (double)kmax ? kmax : (int)x;
  for (int attempt = 0; attempt < 2 && j > k; attempt++, j--) {
    double b[3], f[3];
    if (sample_cell(r, j, b, f) && ((int)b[0] >> kBlockShift) == bx && ((int)b[1] >> kBlockShift) == by &&
        ((int)b[2] >> kBlockShift) == bz)
      return j;
  }
  return k;
}

__global__ __launch_bounds__(256) void render_kernel(void* base, uint64_t cap, const float* __restrict__ rays, int h,
                                                     int w, const float* __restrict__ pose8, double vs,
                                                     double min_weight, double level, double near, double far,
                                                     double step, int skip, BlockSet B, float* __restrict__ range,
                                                     float* __restrict__ normal, uint8_t* __restrict__ hit) {
  const TsdfTable t = table_carve(base, cap);
  int px, py;
  view_pixel(px, py);
  if (px >= w || py >= h) return;
  const size_t i = (size_t)py * w + px;

  Ray r;
  r.near = near; r.step = step; r.vs = vs;
  const double scale = (double)pose8[7];
  view_ray(rays, i, pose8, r.o, r.d);

  // kmax: the last k with near + k * step <= far (the host bounds (far - near) / step by kMaxSamples)
  int kmax = (int)floor((far - near) / step);
  while (near + (double)(kmax + 1) * step <= far) kmax++;
  while (kmax >= 0 && !(near + (double)kmax * step <= far)) kmax--;

  const bool skipping = skip != 0 && B.hdr->overflow == 0;
  Cell cell;
  cell.loaded = false; cell.valid = false; cell.x = cell.y = cell.z = 0;
  uint64_t seen_block = kEmptyKey;    // the last block looked up and its answer
  bool seen_marked = false;
  bool prev_valid = false;
  double prev_f = 0.0;
  float out_range = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f};
  uint8_t out_hit = 0;

  for (int k = 0; k <= kmax; k++) {
    double b[3], f[3];
    if (!sample_cell(r, k, b, f)) { prev_valid = false; continue; }
    const int x = (int)b[0], y = (int)b[1], z = (int)b[2];
    if (skipping) {
      const int bx = x >> kBlockShift, by = y >> kBlockShift, bz = z >> kBlockShift;
      const uint64_t bk = pack_block(bx, by, bz);
      if (bk != seen_block) { seen_block = bk; seen_marked = block_marked(B, bk); }
      if (!seen_marked) {                 // no valid voxel in this block: this sample and the block's later ones are invalid
        prev_valid = false;
        k = block_last_sample(r, k, kmax, bx, by, bz);
        continue;
      }
    }
    cell_load(t, min_weight, x, y, z, cell);
    if (!cell.valid) { prev_valid = false; continue; }
    const double cur_f = cell_value(cell, f);
    if (prev_valid && prev_f >= level && cur_f < level) {
      const double fr = (prev_f - level) / (prev_f - cur_f);
      const double ts = (near + (double)(k - 1) * step) + step * fr;
      double g1[3], g0[3], b0[3], f0[3];
      cell_gradient(cell, f, vs, g1);
      sample_cell(r, k - 1, b0, f0);      // sample k - 1 was valid: its cell loads again (usually it is this cell)
      cell_load(t, min_weight, (int)b0[0], (int)b0[1], (int)b0[2], cell);
      cell_gradient(cell, f0, vs, g0);
      double g[3];
#pragma unroll
      for (int a = 0; a < 3; a++) g[a] = g0[a] + fr * (g1[a] - g0[a]);
      const double ln = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
      for (int a = 0; a < 3; a++) out_n[a] = ln > 0.0 ? (float)(g[a] / ln) : 0.0f;
      out_range = (float)(ts / scale);
      out_hit = 1;
      break;
    }
    prev_valid = true;
    prev_f = cur_f;
  }
  range[i] = out_range;
  normal[3 * i] = out_n[0]; normal[3 * i + 1] = out_n[1]; normal[3 * i + 2] = out_n[2];
  hit[i] = out_hit;
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_tsdf_render_workspace_bytes(uint64_t capacity) {
  if (!table_cap_ok(capacity)) return 0;
  return blocks_carve(nullptr, capacity).bytes;
}

extern "C" int mslam_tsdf_render_blocks(void* table, uint64_t capacity, double min_weight, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  MSLAM_REQUIRE(table && workspace, "tsdf_render_blocks: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_render_blocks: bad capacity");
  const BlockSet B = blocks_carve(workspace, capacity);
  MSLAM_REQUIRE(workspace_bytes >= B.bytes, "tsdf_render_blocks: workspace needs %zu bytes", B.bytes);
  hipStream_t s = (hipStream_t)stream;
  int rc = check_hip(hipMemsetAsync(workspace, 0, 256, s), "tsdf_render_blocks memset");
  if (rc) return rc;
  rc = check_hip(hipMemsetAsync(B.keys, 0xFF, B.cap * 8, s), "tsdf_render_blocks memset");
  if (rc) return rc;
  hipLaunchKernelGGL(render_blocks_kernel, dim3(blocks_for(capacity, 256)), dim3(256), 0, s, table, capacity,
                     min_weight, B);
  MSLAM_LAUNCH_CHECK("tsdf_render_blocks");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_render(void* table, uint64_t capacity, const float* rays, int h, int w, const float* pose8,
                                 double voxel_size, double min_weight, double level, double near, double far,
                                 double step, int skip, const void* workspace, size_t workspace_bytes, float* range,
                                 float* normal, uint8_t* hit, void* stream) {
  if (int rc = view_check("tsdf_render", 1, h, w, nullptr, near, far, true)) return rc;   // the march divides by the span
  if (h == 0 || w == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && rays && pose8 && workspace && range && normal && hit, "tsdf_render: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_render: bad capacity");
  MSLAM_REQUIRE(voxel_size > 0.0 && step > 0.0, "tsdf_render: bad march");
  MSLAM_REQUIRE((far - near) / step < (double)kMaxSamples, "tsdf_render: more than 2^30 samples per ray");
  const BlockSet B = blocks_carve(const_cast<void*>(workspace), capacity);
  MSLAM_REQUIRE(workspace_bytes >= B.bytes, "tsdf_render: workspace needs %zu bytes", B.bytes);
  hipLaunchKernelGGL(render_kernel, view_tile_grid(h, w), dim3(kViewBlock), 0,
                     (hipStream_t)stream, table, capacity, rays, h, w, pose8, voxel_size, min_weight, level, near, far,
                     step, skip, B, range, normal, hit);
  MSLAM_LAUNCH_CHECK("tsdf_render");
  return MSLAM_OK;
}
