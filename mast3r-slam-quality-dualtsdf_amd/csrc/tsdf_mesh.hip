// Triangle mesh of the global sparse TSDF (marching cubes over the live voxel hash), and bulk loading of voxels into a
// table.  Semantics in DESIGN.md "Mesh extraction"; tests/mc_numpy.py states the same algorithm in numpy.
//
//   keys      one thread per slot: the packed key of every valid voxel (present, fused, weight >= min_weight), else
//             INT64_MAX.  The caller sorts these once (torch.sort): the packed-key order is lexicographic on the
//             biased coordinates, so sorted position i is the voxel's canonical index, whatever the capacity.
//   rank      one thread per sorted position: rank[slot] = position; clears the position's flags.
//   classify  one thread per valid voxel: probes its 7 +x/+y/+z/+xy/+xz/+yz/+xyz neighbours (bounded, kMaxProbe),
//             forms the cube case when all 8 corners are valid, writes the cube's triangle count and flags every edge
//             its triangles use at the edge's owner (the lower endpoint; plain byte stores of 1 - idempotent).
//   vcount    one thread per position: number of flagged edges = vertices the voxel owns.
//   (caller)  exclusive scans of the vertex / face counts (torch.cumsum), one host read of (V, F).
//   vertices  one thread per position with flagged edges: interpolated position and normal per flagged edge.
//   faces     one thread per position with triangles: re-probes its 7 neighbours and writes the vertex ids of each
//             triangle, found through the owner voxel's scanned base.
// No counter lives at a single address: every output offset comes from the scans, so the output is canonical and
// bit-identical across capacities, rehashes and repeated calls.  Nothing here writes the table.
#include "common.h"
#include "mc_tables.h"
#include "tsdf_table.h"

namespace mslam {

constexpr int64_t kNoKey = 0x7FFFFFFFFFFFFFFFll;

// byte 0..2: edge along axis a owned by this voxel carries a referenced vertex; byte 3: cube case (0 = no triangles)
struct MeshScratch {
  uint32_t* rank;   // [cap] slot -> sorted position (valid voxels only)
  uint8_t* flags;   // [cap][4]
  size_t bytes;
};

static MeshScratch mesh_carve(void* base, uint64_t cap) {
  MeshScratch s;
  char* p = (char*)base;
  s.rank = (uint32_t*)p;
  s.flags = (uint8_t*)(p + al(cap * 4));
  s.bytes = al(cap * 4) + al(cap * 4);
  return s;
}

__global__ __launch_bounds__(256) void mesh_keys_kernel(void* base, uint64_t cap, double min_weight,
                                                        int64_t* __restrict__ sort_keys) {
  const TsdfTable t = table_carve(base, cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const uint64_t k = t.keys[i];
  sort_keys[i] = (k != kEmptyKey && voxel_valid(t, (int64_t)i, min_weight)) ? (int64_t)k : kNoKey;
}

__global__ __launch_bounds__(256) void mesh_rank_kernel(uint64_t cap, const int64_t* __restrict__ sorted,
                                                        const int64_t* __restrict__ order, MeshScratch S) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  reinterpret_cast<uint32_t*>(S.flags)[i] = 0u;
  if (sorted[i] != kNoKey) S.rank[order[i]] = (uint32_t)i;
}

// the 8 cube corners of key (x, y, z) in the lattice's corner order (tsdf_table.h corner_offset): slot of corner c, -1
// when absent / invalid
__device__ __forceinline__ bool cube_slots(const TsdfTable& t, int64_t own_slot, long long x, long long y, long long z,
                                           double min_weight, int64_t (&cs)[8]) {
  cs[0] = own_slot;
  bool full = true;
#pragma unroll
  for (int c = 1; c < 8; c++) {
    cs[c] = find_valid(t, x + corner_offset(c, 0), y + corner_offset(c, 1), z + corner_offset(c, 2), min_weight);
    full = full && cs[c] >= 0;
  }
  return full;
}

__global__ __launch_bounds__(256) void mesh_classify_kernel(void* base, uint64_t cap, double min_weight, double level,
                                                            const int64_t* __restrict__ sorted,
                                                            const int64_t* __restrict__ order, MeshScratch S,
                                                            int32_t* __restrict__ fcount) {
  const TsdfTable t = table_carve(base, cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const int64_t key = sorted[i];
  if (key == kNoKey) { fcount[i] = 0; return; }
  long long x, y, z;
  unpack_key((uint64_t)key, x, y, z);
  int64_t cs[8];
  int ntri = 0;
  if (cube_slots(t, order[i], x, y, z, min_weight, cs)) {
    int cube = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) cube |= (t.tsdf[cs[c]] < level ? 1 : 0) << c;
    ntri = kMcTriCount[cube];
    if (ntri) {
      S.flags[4 * i + 3] = (uint8_t)cube;
      for (int j = 0; j < 3 * ntri; j++) {
        const int e = kMcTriTable[cube][j];
        const int c = kMcEdgeCorner[e];
        const uint32_t owner = c == 0 ? (uint32_t)i : S.rank[cs[c]];
        S.flags[4 * (uint64_t)owner + kMcEdgeAxis[e]] = 1;
      }
    }
  }
  fcount[i] = ntri;
}

__global__ __launch_bounds__(256) void mesh_vcount_kernel(uint64_t cap, MeshScratch S, int32_t* __restrict__ vcount) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const uint8_t* f = S.flags + 4 * i;
  vcount[i] = (int32_t)f[0] + (int32_t)f[1] + (int32_t)f[2];
}

// TSDF gradient at voxel (x, y, z) of value v: central differences over valid neighbours, one-sided with one, 0 with none
__device__ __forceinline__ void voxel_gradient(const TsdfTable& t, long long x, long long y, long long z, double v,
                                               double vs, double min_weight, double (&g)[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const long long dx = d == 0, dy = d == 1, dz = d == 2;
    const int64_t sp = find_valid(t, x + dx, y + dy, z + dz, min_weight);
    const int64_t sm = find_valid(t, x - dx, y - dy, z - dz, min_weight);
    if (sp >= 0 && sm >= 0) g[d] = (t.tsdf[sp] - t.tsdf[sm]) / (2.0 * vs);
    else if (sp >= 0) g[d] = (t.tsdf[sp] - v) / vs;
    else if (sm >= 0) g[d] = (v - t.tsdf[sm]) / vs;
    else g[d] = 0.0;
  }
}

__global__ __launch_bounds__(256) void mesh_vertices_kernel(void* base, uint64_t cap, double vs, double min_weight,
                                                            double level, const int64_t* __restrict__ sorted,
                                                            const int64_t* __restrict__ order, MeshScratch S,
                                                            const int64_t* __restrict__ vbase, int64_t nv,
                                                            float* __restrict__ vert, float* __restrict__ nrm) {
  const TsdfTable t = table_carve(base, cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const uint8_t* f = S.flags + 4 * i;
  if (!(f[0] | f[1] | f[2])) return;
  long long x, y, z;
  unpack_key((uint64_t)sorted[i], x, y, z);
  const int64_t sa = order[i];
  const double va = t.tsdf[sa];
  double ga[3];
  voxel_gradient(t, x, y, z, va, vs, min_weight, ga);
  int64_t id = vbase[i];
  for (int a = 0; a < 3; a++) {
    if (!f[a]) continue;
    const long long bx = x + (a == 0), by = y + (a == 1), bz = z + (a == 2);
    const int64_t sb = find_valid(t, bx, by, bz, min_weight);   // flagged => valid (a cube with all 8 corners used it)
    if (sb < 0 || id >= nv) return;
    const double vb = t.tsdf[sb];
    double gb[3];
    voxel_gradient(t, bx, by, bz, vb, vs, min_weight, gb);
    const double tt = (level - va) / (vb - va);
    const double pa[3] = {((double)x + 0.5) * vs, ((double)y + 0.5) * vs, ((double)z + 0.5) * vs};
    const double pb[3] = {((double)bx + 0.5) * vs, ((double)by + 0.5) * vs, ((double)bz + 0.5) * vs};
    double g[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      vert[3 * id + d] = (float)(pa[d] + tt * (pb[d] - pa[d]));
      g[d] = ga[d] + tt * (gb[d] - ga[d]);
    }
    const double ln = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
    for (int d = 0; d < 3; d++) nrm[3 * id + d] = ln > 0.0 ? (float)(g[d] / ln) : 0.0f;
    id++;
  }
}

__global__ __launch_bounds__(256) void mesh_faces_kernel(void* base, uint64_t cap, double min_weight,
                                                         const int64_t* __restrict__ sorted,
                                                         const int64_t* __restrict__ order, MeshScratch S,
                                                         const int64_t* __restrict__ vbase,
                                                         const int64_t* __restrict__ fbase, int64_t nf,
                                                         int32_t* __restrict__ faces) {
  const TsdfTable t = table_carve(base, cap);
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const int cube = S.flags[4 * i + 3];
  if (cube == 0) return;
  long long x, y, z;
  unpack_key((uint64_t)sorted[i], x, y, z);
  int64_t cs[8];
  if (!cube_slots(t, order[i], x, y, z, min_weight, cs)) return;
  const int ntri = kMcTriCount[cube];
  const int64_t f0 = fbase[i];
  if (f0 + ntri > nf) return;
  for (int j = 0; j < 3 * ntri; j++) {
    const int e = kMcTriTable[cube][j];
    const int c = kMcEdgeCorner[e], a = kMcEdgeAxis[e];
    const uint64_t owner = c == 0 ? i : (uint64_t)S.rank[cs[c]];
    const uint8_t* of = S.flags + 4 * owner;
    int32_t before = 0;
    for (int b = 0; b < a; b++) before += of[b];
    faces[3 * f0 + j] = (int32_t)(vbase[owner] + before);
  }
}

// bulk insert of averaged voxels (state 2): keys i64[n,3] must be distinct
__global__ __launch_bounds__(256) void tsdf_load_kernel(void* base, uint64_t cap, const int64_t* __restrict__ keys,
                                                        const double* __restrict__ tsdf,
                                                        const double* __restrict__ weight, int n) {
  const TsdfTable t = table_carve(base, cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t key;
  if (!pack_key(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2], key)) { t.hdr->overflow = 1; return; }
  const int64_t slot = table_insert(t, key);
  if (slot < 0) { t.hdr->overflow = 1; return; }
  t.tsdf[slot] = tsdf[i]; t.weight[slot] = weight[i]; t.state[slot] = 2;
}

}  // namespace mslam

using namespace mslam;

extern "C" size_t mslam_tsdf_mesh_workspace_bytes(uint64_t capacity) {
  if (!table_cap_ok(capacity)) return 0;
  return mesh_carve(nullptr, capacity).bytes;
}

extern "C" int mslam_tsdf_mesh_keys(void* table, uint64_t capacity, double min_weight, int64_t* sort_keys,
                                    void* stream) {
  MSLAM_REQUIRE(table && sort_keys, "tsdf_mesh_keys: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_mesh_keys: bad capacity");
  hipLaunchKernelGGL(mesh_keys_kernel, dim3(blocks_for(capacity, 256)), dim3(256), 0, (hipStream_t)stream, table, capacity,
                     min_weight, sort_keys);
  MSLAM_LAUNCH_CHECK("tsdf_mesh_keys");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_mesh_count(void* table, uint64_t capacity, double min_weight, double level,
                                     const int64_t* sorted_keys, const int64_t* order, int32_t* counts,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  MSLAM_REQUIRE(table && sorted_keys && order && counts && workspace, "tsdf_mesh_count: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_mesh_count: bad capacity");
  const MeshScratch S = mesh_carve(workspace, capacity);
  MSLAM_REQUIRE(workspace_bytes >= S.bytes, "tsdf_mesh_count: workspace needs %zu bytes", S.bytes);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = blocks_for(capacity, 256);
  hipLaunchKernelGGL(mesh_rank_kernel, dim3(nb), dim3(256), 0, s, capacity, sorted_keys, order, S);
  hipLaunchKernelGGL(mesh_classify_kernel, dim3(nb), dim3(256), 0, s, table, capacity, min_weight, level, sorted_keys,
                     order, S, counts + capacity);
  hipLaunchKernelGGL(mesh_vcount_kernel, dim3(nb), dim3(256), 0, s, capacity, S, counts);
  MSLAM_LAUNCH_CHECK("tsdf_mesh_count");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_mesh_emit(void* table, uint64_t capacity, double voxel_size, double min_weight, double level,
                                    const int64_t* sorted_keys, const int64_t* order, const int64_t* vbase,
                                    const int64_t* fbase, void* workspace, size_t workspace_bytes, float* vertices,
                                    float* normals, int32_t* faces, int64_t n_vertices, int64_t n_faces,
                                    void* stream) {
  MSLAM_REQUIRE(n_vertices >= 0 && n_faces >= 0 && n_vertices < (1ll << 31), "tsdf_mesh_emit: bad output sizes");
  if (n_vertices == 0 && n_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && sorted_keys && order && vbase && fbase && workspace && vertices && normals && faces,
                "tsdf_mesh_emit: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_mesh_emit: bad capacity");
  const MeshScratch S = mesh_carve(workspace, capacity);
  MSLAM_REQUIRE(workspace_bytes >= S.bytes, "tsdf_mesh_emit: workspace needs %zu bytes", S.bytes);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = blocks_for(capacity, 256);
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3(nb), dim3(256), 0, s, table, capacity, voxel_size, min_weight, level,
                     sorted_keys, order, S, vbase, n_vertices, vertices, normals);
  hipLaunchKernelGGL(mesh_faces_kernel, dim3(nb), dim3(256), 0, s, table, capacity, min_weight, sorted_keys, order, S,
                     vbase, fbase, n_faces, faces);
  MSLAM_LAUNCH_CHECK("tsdf_mesh_emit");
  return MSLAM_OK;
}

extern "C" int mslam_tsdf_load(void* table, uint64_t capacity, const int64_t* keys, const double* tsdf,
                               const double* weight, int n, void* stream) {
  MSLAM_REQUIRE(n >= 0, "tsdf_load: negative count");
  if (n == 0) return MSLAM_OK;
  MSLAM_REQUIRE(table && keys && tsdf && weight, "tsdf_load: null pointer");
  MSLAM_REQUIRE(table_cap_ok(capacity), "tsdf_load: bad capacity");
  hipLaunchKernelGGL(tsdf_load_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, table,
                     capacity, keys, tsdf, weight, n);
  MSLAM_LAUNCH_CHECK("tsdf_load");
  return MSLAM_OK;
}
