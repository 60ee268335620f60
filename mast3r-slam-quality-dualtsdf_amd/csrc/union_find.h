// The lock-free union-find that mesh_components.hip (components of a mesh) and cloud_cluster.hip (clusters of a cloud)
// share: parent[v] <= v always, every write an atomicMin, no thread ever waits for another.  The invariant and why
// nothing is lost on the way are written out at the head of mesh_components.hip.
#pragma once
#include "common.h"

namespace mslam {

#define CC_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// Root of v as far as this thread can see; halves the path on the way.  v strictly decreases in every round.
__device__ __forceinline__ int cc_find(int32_t* parent, int v) {
  int p = __hip_atomic_load(parent + v, CC_RELAXED);
  while (p < v) {
    const int gp = __hip_atomic_load(parent + p, CC_RELAXED);
    if (gp >= p) return p;
    atomicMin(parent + v, gp);
    v = gp;
    p = __hip_atomic_load(parent + v, CC_RELAXED);
  }
  return v;
}

// Links the larger root below the smaller.  max(a, b) strictly decreases in every round.
__device__ __forceinline__ void cc_unite(int32_t* parent, int a, int b) {
  a = cc_find(parent, a);
  b = cc_find(parent, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(parent + hi, lo);
    if (old == hi) return;            // hi was a root and now hangs below lo
    a = cc_find(parent, old);         // old < hi: hi was no root any more; (old, lo) still has to be united
    b = cc_find(parent, lo);
  }
}

}  // namespace mslam
