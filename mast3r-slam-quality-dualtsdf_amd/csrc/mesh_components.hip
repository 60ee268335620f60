// Connected components of a welded triangle mesh (faces i32[F,3] with indices in [0, V)), and the filter that drops
// whole components.  Semantics in DESIGN.md "Mesh components"; tests/cc_numpy.py states the same definitions in numpy.
//
//   label   init: root[v] = v.  hook: one thread per face unites (a, b) and (a, c) in a lock-free union-find whose
//           parent array is `root` itself.  flatten: root[v] = find(v).  On return root[v] is the smallest vertex index
//           of v's component, exactly, whatever order the atomics landed in.
//   count   faces_at_root[r] / verts_at_root[r] = faces (by their first vertex) / vertices of the component whose root
//           is r, zero at every other index.  Integer adds: the same value in any order.
//   select  keep_vertex[v] = keep_root[root[v]], keep_face[f] = keep_root[root[first vertex of f]] as 0/1 i32.
//   (caller)  exclusive scans of the flags (torch.cumsum), one host read of the output sizes.
//   emit    kept vertices / normals / colours gathered in their original order, kept faces written with remapped ids.
// No output offset comes from a counter at a single address: a filtered canonical mesh stays canonical.
//
// THE INVARIANT of the union-find.  Every write to the parent array is an atomicMin (or, in flatten, a store of the
// final root, which is <= every value the entry has held), so a parent is only ever replaced by a smaller value, and
// since it starts as parent[v] = v, parent[v] <= v ALWAYS holds.  From that alone:
//   - every find strictly descends (each step moves to a strictly smaller index or stops), so it ends after at most v
//     steps whatever other threads do, also when a load returns a value that has since been lowered: every value an
//     entry has ever held is <= its index;
//   - a union retries only onto a pair whose larger member is strictly smaller than before, so it ends too;
//   - there is no lock, spin-wait or flag that another thread must set: no thread ever waits for another.
// Nothing is lost on the way.  Every value written to parent[x] lies in x's component.  When atomicMin(&parent[hi], lo)
// returns old != hi, the entry now holds min(old, lo); whichever of the two it dropped is re-united by continuing from
// the pair (old, lo), both below hi.  Path halving writes a grandparent gp of v read through p = parent[v]; p and gp
// stay connected through parent entries of indices below v (by induction over the index), so v keeps its connection to
// everything parent[v] has ever held.  When the hook kernel has ended, no pair is pending, the parent links alone span
// each component, every tree's root is its smallest index, and flatten reads it.
#include "mesh_topo.h"
#include "union_find.h"

namespace mslam {

// cc_find, cc_unite and CC_RELAXED: union_find.h, shared with cloud_cluster.hip

__global__ __launch_bounds__(256) void cc_init_kernel(int nv, int32_t* __restrict__ root) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < nv) root[v] = v;
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                      int32_t* parent) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  if (!tp_in_range(a, b, c, nv)) return;     // the caller validates; never index outside the array
  cc_unite(parent, a, b);
  cc_unite(parent, a, c);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int nv, int32_t* parent) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  __hip_atomic_store(parent + v, cc_find(parent, v), CC_RELAXED);
}

// dst[r] += 1 for every lane with r >= 0.  aggregate: a run of neighbouring lanes with the same r adds once, its
// length (faces and vertices that are neighbours in canonical order almost always share a root).  Every lane of the
// wave must call this (r = -1 for a lane without work): the shuffle and the ballot read all 64.
__device__ __forceinline__ void cc_wave_add(int32_t* dst, int r, bool aggregate) {
  if (!aggregate) {
    if (r >= 0) atomicAdd(dst + r, 1);
    return;
  }
  const int lane = threadIdx.x & (kWave - 1);
  const int prev = __shfl_up(r, 1, kWave);
  const bool head = lane == 0 || prev != r;
  const unsigned long long heads = __ballot(head);
  if (head && r >= 0) {
    const unsigned long long later = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    atomicAdd(dst + r, later ? __ffsll(later) : kWave - lane);      // lanes up to the next run's head
  }
}

__global__ __launch_bounds__(256) void cc_zero_kernel(int nv, int32_t* __restrict__ a, int32_t* __restrict__ b) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  if (a) a[v] = 0;
  if (b) b[v] = 0;
}

__global__ __launch_bounds__(256) void cc_count_faces_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                             const int32_t* __restrict__ root,
                                                             int32_t* faces_at_root, int aggregate) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  if (f < nf) {
    const int a = faces[3 * (size_t)f];
    if ((unsigned)a < (unsigned)nv) r = root[a];
    if ((unsigned)r >= (unsigned)nv) r = -1;
  }
  cc_wave_add(faces_at_root, r, aggregate != 0);
}

__global__ __launch_bounds__(256) void cc_count_verts_kernel(int nv, const int32_t* __restrict__ root,
                                                             int32_t* verts_at_root, int aggregate) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  int r = v < nv ? root[v] : -1;
  if ((unsigned)r >= (unsigned)nv) r = -1;
  cc_wave_add(verts_at_root, r, aggregate != 0);
}

__global__ __launch_bounds__(256) void cc_select_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                        const int32_t* __restrict__ root,
                                                        const uint8_t* __restrict__ keep_root,
                                                        int32_t* __restrict__ keep_vertex,
                                                        int32_t* __restrict__ keep_face) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    const int r = root[i];
    keep_vertex[i] = (unsigned)r < (unsigned)nv && keep_root[r] ? 1 : 0;
  }
  if (i < nf) {
    const int a = faces[3 * (size_t)i];
    const int r = (unsigned)a < (unsigned)nv ? root[a] : -1;
    keep_face[i] = (unsigned)r < (unsigned)nv && keep_root[r] ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void cc_emit_kernel(const float* __restrict__ vert, const float* __restrict__ nrm,
                                                      const float* __restrict__ col,
                                                      const int32_t* __restrict__ faces, int nf, int nv,
                                                      const int32_t* __restrict__ keep_vertex,
                                                      const int32_t* __restrict__ keep_face,
                                                      const int64_t* __restrict__ vbase,
                                                      const int64_t* __restrict__ fbase, float* __restrict__ out_vert,
                                                      float* __restrict__ out_nrm, float* __restrict__ out_col,
                                                      int32_t* __restrict__ out_faces, int64_t nv_out,
                                                      int64_t nf_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nv && keep_vertex[i]) {
    const int64_t o = vbase[i];
    if (o >= 0 && o < nv_out) {
#pragma unroll
      for (int d = 0; d < 3; d++) {
        out_vert[3 * o + d] = vert[3 * (size_t)i + d];
        out_nrm[3 * o + d] = nrm[3 * (size_t)i + d];
        if (col) out_col[3 * o + d] = col[3 * (size_t)i + d];
      }
    }
  }
  if (i < nf && keep_face[i]) {
    const int64_t o = fbase[i];
    const int a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    if (o >= 0 && o < nf_out && tp_in_range(a, b, c, nv)) {
      out_faces[3 * o] = (int32_t)vbase[a];       // a kept face's vertices are kept: they share its root
      out_faces[3 * o + 1] = (int32_t)vbase[b];
      out_faces[3 * o + 2] = (int32_t)vbase[c];
    }
  }
}

}  // namespace mslam

using namespace mslam;

extern "C" int mslam_mesh_cc_label(const int32_t* faces, int num_faces, int num_vertices, int32_t* root,
                                   void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_cc_label: negative size");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(root && (faces || num_faces == 0), "mesh_cc_label: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, s, num_vertices, root);
  if (num_faces > 0) {
    hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, s, faces, num_faces,
                       num_vertices, root);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, s, num_vertices, root);
  }
  MSLAM_LAUNCH_CHECK("mesh_cc_label");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_cc_count(const int32_t* faces, int num_faces, int num_vertices, const int32_t* root,
                                   int32_t* faces_at_root, int32_t* verts_at_root, int aggregate, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_cc_count: negative size");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(root && (faces || num_faces == 0), "mesh_cc_count: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_zero_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, s, num_vertices, faces_at_root,
                     verts_at_root);
  if (faces_at_root && num_faces > 0)
    hipLaunchKernelGGL(cc_count_faces_kernel, dim3(blocks_for(num_faces, 256)), dim3(256), 0, s, faces, num_faces,
                       num_vertices, root, faces_at_root, aggregate);
  if (verts_at_root)
    hipLaunchKernelGGL(cc_count_verts_kernel, dim3(blocks_for(num_vertices, 256)), dim3(256), 0, s, num_vertices, root,
                       verts_at_root, aggregate);
  MSLAM_LAUNCH_CHECK("mesh_cc_count");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_cc_select(const int32_t* faces, int num_faces, int num_vertices, const int32_t* root,
                                    const uint8_t* keep_root, int32_t* keep_vertex, int32_t* keep_face, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_cc_select: negative size");
  if (num_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(root && keep_root && keep_vertex && ((faces && keep_face) || num_faces == 0),
                "mesh_cc_select: null pointer");
  const int n = num_vertices > num_faces ? num_vertices : num_faces;
  hipLaunchKernelGGL(cc_select_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, faces, num_faces,
                     num_vertices, root, keep_root, keep_vertex, keep_face);
  MSLAM_LAUNCH_CHECK("mesh_cc_select");
  return MSLAM_OK;
}

extern "C" int mslam_mesh_cc_emit(const float* vertices, const float* normals, const float* colors,
                                  const int32_t* faces, int num_faces, int num_vertices, const int32_t* keep_vertex,
                                  const int32_t* keep_face, const int64_t* vbase, const int64_t* fbase,
                                  float* out_vertices, float* out_normals, float* out_colors, int32_t* out_faces,
                                  int64_t n_out_vertices, int64_t n_out_faces, void* stream) {
  MSLAM_REQUIRE(num_faces >= 0 && num_vertices >= 0, "mesh_cc_emit: negative size");
  MSLAM_REQUIRE(n_out_vertices >= 0 && n_out_vertices <= num_vertices && n_out_faces >= 0 &&
                n_out_faces <= num_faces, "mesh_cc_emit: bad output sizes");
  if (n_out_vertices == 0 && n_out_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && normals && keep_vertex && vbase && out_vertices && out_normals,
                "mesh_cc_emit: null pointer");
  MSLAM_REQUIRE((colors == nullptr) == (out_colors == nullptr), "mesh_cc_emit: colours need an input and an output");
  MSLAM_REQUIRE(num_faces == 0 || (faces && keep_face && fbase && (out_faces || n_out_faces == 0)),
                "mesh_cc_emit: null pointer");
  const int n = num_vertices > num_faces ? num_vertices : num_faces;
  hipLaunchKernelGGL(cc_emit_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, vertices, normals,
                     colors, faces, num_faces, num_vertices, keep_vertex, keep_face, vbase, fbase, out_vertices,
                     out_normals, out_colors, out_faces, n_out_vertices, n_out_faces);
  MSLAM_LAUNCH_CHECK("mesh_cc_emit");
  return MSLAM_OK;
}
