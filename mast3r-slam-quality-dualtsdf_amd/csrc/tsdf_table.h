// Layout of the global-TSDF voxel hash and its probe helpers, shared by csrc/tsdf_global.hip (integrate / query /
// pose) and csrc/tsdf_mesh.hip (mesh extraction, loading).
#pragma once
#include "common.h"

namespace mslam {

constexpr uint64_t kEmptyKey = ~0ull;
constexpr int kKeyBias = 1 << 20;  // coordinates in [-2^20, 2^20)

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

__device__ __forceinline__ int64_t table_find(const TsdfTable& t, uint64_t key) {
  uint64_t s = mix64(key) & (t.cap - 1);
  const uint64_t limit = t.cap < kMaxProbe ? t.cap : kMaxProbe;
  for (uint64_t probe = 0; probe < limit; probe++) {
    const uint64_t k = t.keys[s];
    if (k == key) return (int64_t)s;
    if (k == kEmptyKey) return -1;
    s = (s + 1) & (t.cap - 1);
  }
  return -1;
}

__device__ __forceinline__ int64_t table_insert(const TsdfTable& t, uint64_t key) {
  uint64_t s = mix64(key) & (t.cap - 1);
  const uint64_t limit = t.cap < kMaxProbe ? t.cap : kMaxProbe;
  for (uint64_t probe = 0; probe < limit; probe++) {
    const uint64_t prev = atomicCAS((unsigned long long*)&t.keys[s], (unsigned long long)kEmptyKey,
                                    (unsigned long long)key);
    if (prev == kEmptyKey) { atomicAdd(&t.hdr->count, 1u); return (int64_t)s; }
    if (prev == key) return (int64_t)s;
    s = (s + 1) & (t.cap - 1);
  }
  return -1;
}

}  // namespace mslam
