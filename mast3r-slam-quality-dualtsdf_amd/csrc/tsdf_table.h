// The global-TSDF voxel hash and every rule of reading it, each stated once: layout and capacity rule, keys, the bounded
// probe, what a valid voxel is, and the sample lattice with its corner order and trilinear blend.  Used by csrc/tsdf_global.hip (integrate / query / pose), tsdf_color.hip (colour fuse and
// sample), tsdf_render.hip (ray cast), tsdf_mesh.hip (mesh extraction, loading), tsdf_walk.h (the ray walk of a fused
// point) and cloud.hip (world_to_key).
#pragma once
#include "common.h"

namespace mslam {

constexpr uint64_t kEmptyKey = ~0ull;
constexpr int kKeyBias = 1 << 20;  // coordinates in [-2^20, 2^20)

// Every table is made by mslam_tsdf_table_init, which refuses any other capacity: an entry point that checks this
// refuses nothing that worked before, and no kernel masks with cap - 1 on a number that is not a power of two.
static inline bool table_cap_ok(uint64_t capacity) {
  return capacity >= 1024 && (capacity & (capacity - 1)) == 0 && capacity <= (1ull << 32);
}

struct TsdfHeader {
  uint64_t capacity;     // slots (power of two)
  uint32_t count;        // occupied slots
  uint32_t overflow;     // != 0: table full or coordinate out of range (samples were dropped)
  uint32_t n_records;    // scratch: records emitted by the running integrate
  uint32_t n_touched;    // scratch: voxels touched by the running integrate
  uint32_t seg_cursor;   // scratch
  uint32_t fused;        // points fused by the last integrate (return value of the reference)
  uint32_t dump_cursor;
  uint32_t n_big;        // scratch: voxels with more samples than a thread sorts itself (replayed by a wave each)
};

struct TsdfTable {
  TsdfHeader* hdr;
  uint64_t* keys;
  double* tsdf;
  double* weight;
  uint32_t* cnt;
  uint32_t* off;
  uint32_t* fill;
  uint8_t* state;  // 0 absent, 1 touched once (value is still the float32 sample), 2 averaged
  uint64_t cap;
};

static inline size_t al(size_t x) { return (x + 255) / 256 * 256; }

__host__ __device__ inline TsdfTable table_carve(void* base, uint64_t cap) {
  TsdfTable t;
  char* p = (char*)base;
  size_t o = 0;
  t.hdr = (TsdfHeader*)(p + o); o += 256;
  t.keys = (uint64_t*)(p + o); o += (cap * 8 + 255) / 256 * 256;
  t.tsdf = (double*)(p + o); o += (cap * 8 + 255) / 256 * 256;
  t.weight = (double*)(p + o); o += (cap * 8 + 255) / 256 * 256;
  t.cnt = (uint32_t*)(p + o); o += (cap * 4 + 255) / 256 * 256;
  t.off = (uint32_t*)(p + o); o += (cap * 4 + 255) / 256 * 256;
  t.fill = (uint32_t*)(p + o); o += (cap * 4 + 255) / 256 * 256;
  t.state = (uint8_t*)(p + o); o += (cap + 255) / 256 * 256;
  t.cap = cap;
  return t;
}

static size_t table_bytes(uint64_t cap) {
  return 256 + 3 * al(cap * 8) + 3 * al(cap * 4) + al(cap);
}

__device__ __forceinline__ uint64_t mix64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

__device__ __forceinline__ bool pack_key(long long x, long long y, long long z, uint64_t& key) {
  const long long bx = x + kKeyBias, by = y + kKeyBias, bz = z + kKeyBias;
  if ((unsigned long long)bx >= 2ull * kKeyBias || (unsigned long long)by >= 2ull * kKeyBias ||
      (unsigned long long)bz >= 2ull * kKeyBias)
    return false;
  key = ((uint64_t)bx << 42) | ((uint64_t)by << 21) | (uint64_t)bz;
  return true;
}

__device__ __forceinline__ void unpack_key(uint64_t key, long long& x, long long& y, long long& z) {
  x = (long long)((key >> 42) & 0x1FFFFF) - kKeyBias;
  y = (long long)((key >> 21) & 0x1FFFFF) - kKeyBias;
  z = (long long)(key & 0x1FFFFF) - kKeyBias;
}

// Integer voxel index of a world point, floor(float32 / float32(voxel_size)) per axis (global_volume.py:133-134 under
// NumPy-2 promotion), for every kernel that turns a position into a key.  A quotient that is NaN, +-inf or beyond
// +-2^21 has no voxel: the reference's np.floor(..).astype(int) gives INT64_MIN there, which no dict entry has, while
// the C++ cast of such a float is undefined (gfx950 turns NaN into 0, a voxel that exists).  It is decided on the
// float, before any cast; every other value casts exactly (|q| < 2^21 is an integer in float32) and its neighbours
// k +- 1 are out of the key range whenever q itself was refused.
__device__ __forceinline__ bool world_to_index(float px, float py, float pz, float vs, long long (&k)[3]) {
  const float q[3] = {floorf(px / vs), floorf(py / vs), floorf(pz / vs)};
  const float lim = 2.0f * (float)kKeyBias;
  if (!(fabsf(q[0]) < lim) || !(fabsf(q[1]) < lim) || !(fabsf(q[2]) < lim)) return false;
  k[0] = (long long)q[0]; k[1] = (long long)q[1]; k[2] = (long long)q[2];
  return true;
}

__device__ __forceinline__ bool world_to_key(float px, float py, float pz, float vs, uint64_t& key) {
  long long k[3];
  return world_to_index(px, py, pz, vs, k) && pack_key(k[0], k[1], k[2], key);
}

// Probe sequences are bounded: the host keeps the load factor <= 1/2 (TSDFVolume.maintain grows and rehashes), where a
// linear-probe cluster of kMaxProbe slots does not occur; an insert that would need more reports overflow instead of
// scanning a multi-million-slot table.
constexpr uint64_t kMaxProbe = 1024;

// The probe over a raw key array of `cap` slots (a power of two): the slot that holds `key`, or -1.  kFind only reads
// and stops at the first empty slot.  kInsert claims the first empty slot with a 64-bit CAS.  kInsertReadFirst reads
// the slot and goes to the CAS only when it saw it empty: for a set whose inserts mostly find their key already there
// (the block set of the ray cast) most probes then cost no atomic.
enum ProbeMode { kFind, kInsert, kInsertReadFirst };

template <ProbeMode kMode>
__device__ __forceinline__ int64_t probe_slot(uint64_t* keys, uint64_t cap, uint64_t key, bool& inserted) {
  uint64_t s = mix64(key) & (cap - 1);
  const uint64_t limit = cap < kMaxProbe ? cap : kMaxProbe;
  for (uint64_t probe = 0; probe < limit; probe++) {
    uint64_t k = kMode == kInsert ? kEmptyKey : keys[s];
    if (kMode != kFind && k == kEmptyKey) {
      k = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (k == kEmptyKey) { inserted = true; return (int64_t)s; }
    }
    if (k == key) return (int64_t)s;
    if (kMode == kFind && k == kEmptyKey) return -1;
    s = (s + 1) & (cap - 1);
  }
  return -1;
}

__device__ __forceinline__ int64_t probe_find(uint64_t* keys, uint64_t cap, uint64_t key) {
  bool inserted;
  return probe_slot<kFind>(keys, cap, key, inserted);
}

// `inserted` is set when this call claimed the slot and left alone otherwise
template <ProbeMode kMode = kInsert>
__device__ __forceinline__ int64_t probe_insert(uint64_t* keys, uint64_t cap, uint64_t key, bool& inserted) {
  static_assert(kMode != kFind, "probe_insert inserts");
  return probe_slot<kMode>(keys, cap, key, inserted);
}

__device__ __forceinline__ int64_t table_find(const TsdfTable& t, uint64_t key) { return probe_find(t.keys, t.cap, key); }

__device__ __forceinline__ int64_t table_insert(const TsdfTable& t, uint64_t key) {
  bool inserted = false;
  const int64_t s = probe_insert(t.keys, t.cap, key, inserted);
  if (inserted) atomicAdd(&t.hdr->count, 1u);
  return s;
}

// A voxel that the mesh, the view and the block set count: present, fused, and heavy enough.
__device__ __forceinline__ bool voxel_valid(const TsdfTable& t, int64_t slot, double min_weight) {
  return slot >= 0 && t.state[slot] != 0 && t.weight[slot] >= min_weight;
}

// slot of the valid voxel at (x, y, z), or -1 (absent, unfused, light, or outside the key range)
__device__ __forceinline__ int64_t find_valid(const TsdfTable& t, long long x, long long y, long long z, double min_weight) {
  uint64_t key;
  if (!pack_key(x, y, z, key)) return -1;
  const int64_t s = table_find(t, key);
  return voxel_valid(t, s, min_weight) ? s : -1;
}

// The sample lattice of the mesh, the view and the colour: voxel values sit at the voxel centres, so a point p lies in
// the cell whose base corner is b = floor(p / vs - 0.5) (integral, as doubles) at the fractions f = p / vs - 0.5 - b.
// False when the point is not finite or the base is outside the key range; b + 1 may still step out of it.
__device__ __forceinline__ bool lattice_cell(const double (&p)[3], double vs, double (&b)[3], double (&f)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double g = p[a] / vs - 0.5;
    b[a] = floor(g);
    f[a] = g - b[a];
    ok = ok && fabs(b[a]) < (double)kKeyBias;
  }
  return ok;
}

// corner c = dx + 2 dy + 4 dz of a cell or a cube: its offset from the base along `axis`
__device__ __forceinline__ int corner_offset(int c, int axis) { return (c >> axis) & 1; }

__device__ __forceinline__ double lerp(double a, double b, double f) { return a + f * (b - a); }

__device__ __forceinline__ double trilerp(const double (&v)[8], const double (&f)[3]) {
  const double c00 = lerp(v[0], v[1], f[0]), c10 = lerp(v[2], v[3], f[0]);
  const double c01 = lerp(v[4], v[5], f[0]), c11 = lerp(v[6], v[7], f[0]);
  return lerp(lerp(c00, c10, f[1]), lerp(c01, c11, f[1]), f[2]);
}

}  // namespace mslam
