// Boundary loops of a welded triangle mesh, and the closing of the small, well-behaved ones with a centroid fan.
// Semantics in DESIGN.md "Mesh holes"; tests/holes_numpy.py states the same definitions, operation by operation, in
// numpy.  All arithmetic is f64 on the f32 inputs, the build has -ffp-contract=off, every sum runs in walk order.
//
//   keys     one thread per face: the three undirected edge keys min V + max of a counting face (indices in [0, V),
//            pairwise different) in dart order (slot 3 f + c: the edge from corner c to corner c + 1), INT64_MAX in all
//            three slots of any other face.
//   (caller)   sorts the keys, stable, with the permutation: sorted slot i came from dart order[i].
//   mark     one thread per sorted slot: a run of length 1 below INT64_MAX is a boundary dart; flag[order[i]] says so.
//   (caller)   compacts the flagged darts in ascending dart id (B of them, one host read).
//   darts    one thread per boundary dart: its tail and head from the face.
//   (caller)   sorts the tails (with the permutation) and the heads.
//   link     one thread per boundary dart: its head is simple when it occurs exactly once among the tails and once among
//            the heads (two binary searches); then next = the dart with that tail, else none.  state = (next, tail).
//   double   one round of pointer doubling, Jacobi style from state_in to state_out: (ptr, lab)[d] becomes
//            (ptr[ptr[d]], min(lab[d], lab[ptr[d]])), and stays when ptr[d] is none.  After r rounds ptr is the 2^r-th
//            successor, or none if the chain ends before it, and lab the smallest tail on the way: with 2^r >= B a dart
//            whose ptr is not none lies on a cycle and lab is the loop id.
//   loop_labels  one thread per boundary dart: the sort key lab, or INT32_MAX for an open dart, and one more INT32_MAX.
//   (caller)   sorts them; unique_consecutive with counts gives the loop ids, ascending, and their lengths (one host read);
//            the last run, less one, counts the open darts.
//   loop_assign  one thread per boundary dart: the number of its loop (binary search of lab in the loop ids) or -1, and
//            the loop's first dart: the one whose own label (here its tail) is the loop id.
//   measure  one thread per loop: walks it from its first dart and writes the perimeter, the centre and whether the loop
//            is fillable.  Loops longer than max_edges are walked only when all perimeters are asked for.
//   (caller)   exclusive scans of the fillable flags and lengths give the bases (one host read: the new sizes).
//   emit     one thread per fillable loop: the new vertex, its normal and colour, and the n fan faces.
// No atomics, and no thread reads what another writes within a launch.  Every index read from memory is checked against
// its array before it is followed; a walk that meets a bad one stops and its loop is not fillable.
#include <math.h>

#include "mesh_topo.h"

namespace mslam {

constexpr int64_t kMhNoKey = INT64_MAX;
constexpr int32_t kMhNoLabel = INT32_MAX;

__global__ __launch_bounds__(256) void mh_keys_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                      int64_t* __restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const bool ok = tp_counts(a, b, c, nv);
  int64_t* k = keys + 3 * (size_t)f;
  k[0] = ok ? (int64_t)min(a, b) * nv + max(a, b) : kMhNoKey;
  k[1] = ok ? (int64_t)min(b, c) * nv + max(b, c) : kMhNoKey;
  k[2] = ok ? (int64_t)min(c, a) * nv + max(c, a) : kMhNoKey;
}

__global__ __launch_bounds__(256) void mh_mark_kernel(const int64_t* __restrict__ sorted_keys,
                                                      const int64_t* __restrict__ order, int64_t n,
                                                      uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t k = sorted_keys[i];
  const bool single = k != kMhNoKey && (i == 0 || sorted_keys[i - 1] != k) && (i + 1 == n || sorted_keys[i + 1] != k);
  const int64_t d = order[i];
  if ((uint64_t)d < (uint64_t)n) flag[d] = single ? 1 : 0;
}

__global__ __launch_bounds__(256) void mh_darts_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                       const int32_t* __restrict__ dart, int nb,
                                                       int32_t* __restrict__ tail, int32_t* __restrict__ head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int d = dart[i];
  int t = -1, h = -1;
  if ((unsigned)d < 3u * (unsigned)nf) {
    const int f = d / 3, c = d - 3 * f;
    const int a = faces[3 * (size_t)f + c], b = faces[3 * (size_t)f + (c == 2 ? 0 : c + 1)];
    if ((unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv) t = a, h = b;
  }
  tail[i] = t;
  head[i] = h;
}

__global__ __launch_bounds__(256) void mh_link_kernel(const int32_t* __restrict__ tail,
                                                      const int32_t* __restrict__ head,
                                                      const int32_t* __restrict__ sorted_tail,
                                                      const int64_t* __restrict__ tail_order,
                                                      const int32_t* __restrict__ sorted_head, int nb, int nv,
                                                      int2* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int h = head[i];
  int nxt = -1;
  if ((unsigned)h < (unsigned)nv) {
    const int p = tp_once(sorted_tail, nb, h);
    if (p >= 0 && tp_once(sorted_head, nb, h) >= 0) {
      const int64_t j = tail_order[p];
      if ((uint64_t)j < (uint64_t)nb) nxt = (int)j;
    }
  }
  state[i] = make_int2(nxt, tail[i]);
}

// The combine step of a pointer doubling: what a dart's second entry becomes when its pointer jumps over `over`.
struct MhMinLabel {                                      // the smallest label on the way
  static __device__ __forceinline__ int join(int own, int over, int) { return min(own, over); }
};
struct MhSumSteps {                                      // the number of steps, saturating at B + 1
  static __device__ __forceinline__ int join(int own, int over, int nb) {
    return (int)min((int64_t)own + (int64_t)over, (int64_t)nb + 1);
  }
};

template <class Join>
__global__ __launch_bounds__(256) void mh_double_kernel(const int2* __restrict__ state_in, int2* __restrict__ state_out,
                                                        int nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  int2 s = state_in[i];
  if ((unsigned)s.x < (unsigned)nb) {
    const int2 t = state_in[s.x];
    s.x = (unsigned)t.x < (unsigned)nb ? t.x : -1;
    s.y = Join::join(s.y, t.y, nb);
  } else {
    s.x = -1;
  }
  state_out[i] = s;
}

// Is the dart with the doubled state s on a loop?  It lies on a cycle, and `flag` (null: no cycle is excluded) does not
// exclude the cycle's label.  Only a flag makes the label an index, so only then is it held against [0, B): in plain mode
// a label is a vertex and may well be >= B.
__device__ __forceinline__ bool mh_on_loop(int2 s, const uint8_t* __restrict__ flag, int nb) {
  return s.x >= 0 && (!flag || ((unsigned)s.y < (unsigned)nb && !flag[s.y]));
}

__global__ __launch_bounds__(256) void mh_loop_labels_kernel(const int2* __restrict__ labelled,
                                                             const uint8_t* __restrict__ flag, int nb,
                                                             int32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > nb) return;
  int32_t k = kMhNoLabel;
  if (i < nb) {
    const int2 s = labelled[i];
    if (mh_on_loop(s, flag, nb)) k = s.y;
  }
  keys[i] = k;
}

// `own`: the state before the doubling, whose second entry is the dart's own label (its tail, or its name in bow-tie
// mode).  Labels on a cycle are distinct (a loop id is a simple vertex; names are distinct), so one dart writes start[l].
__global__ __launch_bounds__(256) void mh_loop_assign_kernel(
    const int2* __restrict__ labelled, const int2* __restrict__ own, const uint8_t* __restrict__ flag,
    const int32_t* __restrict__ tail, const int32_t* __restrict__ head, int nb, const int32_t* __restrict__ loop_name,
    int nl, int32_t* __restrict__ dart_loop, int32_t* __restrict__ start, int32_t* __restrict__ loop_id,
    int32_t* __restrict__ loop_head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int2 s = labelled[i];
  int l = -1;
  if (mh_on_loop(s, flag, nb)) {
    const int p = tp_lower(loop_name, nl, s.y);
    if (p < nl && loop_name[p] == s.y) l = p;
  }
  dart_loop[i] = l;
  if (l >= 0 && own[i].y == s.y) {
    start[l] = i;
    if (loop_id) loop_id[l] = tail[i];
    if (loop_head) loop_head[l] = head[i];
  }
}

// tail and head of boundary dart d, both in [0, V); false for a dart outside [0, B) or a vertex outside [0, V)
__device__ __forceinline__ bool mh_ends(const int32_t* __restrict__ tail, const int32_t* __restrict__ head, int d, int nb,
                                        int nv, int& a, int& b) {
  if ((unsigned)d >= (unsigned)nb) return false;
  a = tail[d], b = head[d];
  return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv;
}

__global__ __launch_bounds__(256) void mh_measure_kernel(
    const float* __restrict__ vert, const int32_t* __restrict__ faces, int nf, int nv, const int32_t* __restrict__ dart,
    const int32_t* __restrict__ tail, const int32_t* __restrict__ head, const int2* __restrict__ state, int nb,
    const int32_t* __restrict__ start, const int32_t* __restrict__ length, int nl, int max_edges, int all_perimeters,
    double* __restrict__ perimeter, double* __restrict__ centre, uint8_t* __restrict__ fillable) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nl) return;
  const int n = length[l], d0 = start[l];
  const bool small = n >= 3 && n <= max_edges;
  const bool walk = n >= 1 && n <= nb && (small || all_perimeters);
  double per = 0.0, s[3] = {0.0, 0.0, 0.0};
  bool ok = walk;
  int d = d0;
  for (int i = 0; ok && i < n; i++) {
    int a, b;
    ok = mh_ends(tail, head, d, nb, nv, a, b);
    if (!ok) break;
    double pa[3], pb[3], e[3];
    tp_point(vert, a, pa);
    tp_point(vert, b, pb);
    tp_sub(pb, pa, e);
    per = per + sqrt(tp_dot(e, e));
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = s[k] + pa[k];
    d = state[d].x;
  }
  ok = ok && d == d0;                                    // n steps close the loop
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = s[k] / (double)n;
  bool fill = ok && small;
  d = d0;
  for (int i = 0; fill && i < n; i++) {
    int a, b;
    if (!mh_ends(tail, head, d, nb, nv, a, b)) { fill = false; break; }
    const int f = dart[d] / 3;
    if ((unsigned)f >= (unsigned)nf) { fill = false; break; }
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if (!tp_counts(i0, i1, i2, nv)) { fill = false; break; }
    double pa[3], pb[3], q0[3], q1[3], q2[3], u[3], w[3], e1[3], e2[3], fan[3], own[3];
    tp_point(vert, a, pa);
    tp_point(vert, b, pb);
    tp_point(vert, i0, q0);
    tp_point(vert, i1, q1);
    tp_point(vert, i2, q2);
    tp_sub(pa, pb, u);
    tp_sub(c, pb, w);
    tp_cross(u, w, fan);
    tp_sub(q1, q0, e1);
    tp_sub(q2, q0, e2);
    tp_cross(e1, e2, own);
    fill = tp_dot(fan, own) > 0.0;                       // false for zero and for NaN
    d = state[d].x;
  }
  perimeter[l] = ok ? per : (double)NAN;
#pragma unroll
  for (int k = 0; k < 3; k++) centre[3 * (size_t)l + k] = ok ? c[k] : 0.0;
  fillable[l] = fill ? 1 : 0;
}

__global__ __launch_bounds__(256) void mh_emit_kernel(
    const float* __restrict__ vert, const float* __restrict__ colors, const int32_t* __restrict__ tail,
    const int32_t* __restrict__ head, const int2* __restrict__ state, int nb, const int32_t* __restrict__ start,
    const int32_t* __restrict__ length, const uint8_t* __restrict__ fillable, const int64_t* __restrict__ vbase,
    const int64_t* __restrict__ fbase, int nl, int nv, int nf, int new_v, int new_f, const double* __restrict__ centre,
    float* __restrict__ out_vert, float* __restrict__ out_nrm, float* __restrict__ out_col,
    int32_t* __restrict__ out_faces) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= nl || !fillable[l]) return;
  const int n = length[l];
  const int64_t kv = vbase[l], kf = fbase[l];
  if (n < 3 || (uint64_t)kv >= (uint64_t)new_v || kf < 0 || kf + n > new_f) return;
  float c32[3];
  double c[3], s[3] = {0.0, 0.0, 0.0}, col[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c32[k] = (float)centre[3 * (size_t)l + k];
    c[k] = (double)c32[k];
  }
  const int vnew = nv + (int)kv;
  int d = start[l];
  for (int i = 0; i < n; i++) {
    int a = -1, b = -1;
    const bool ok = mh_ends(tail, head, d, nb, nv, a, b);
    int32_t* face = out_faces + 3 * ((size_t)nf + kf + i);
    face[0] = ok ? b : 0, face[1] = ok ? a : 0, face[2] = ok ? vnew : 0;      // measure has walked this loop: ok
    if (!ok) continue;
    double x[3], y[3], e1[3], e2[3], nrm[3];
    tp_point(vert, b, x);
    tp_point(vert, a, y);
    tp_sub(y, x, e1);
    tp_sub(c, x, e2);
    tp_cross(e1, e2, nrm);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      s[k] = s[k] + nrm[k];
      if (colors) col[k] = col[k] + (double)colors[3 * (size_t)a + k];
    }
    d = state[d].x;
  }
  const double ln = sqrt(tp_dot(s, s));
  const bool unit = ln > 0.0 && ln < (double)INFINITY;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const size_t o = 3 * (size_t)vnew + k;
    out_vert[o] = c32[k];
    out_nrm[o] = unit ? (float)(s[k] / ln) : 0.0f;
    if (out_col) out_col[o] = (float)(col[k] / (double)n);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Bow-tie mode (DESIGN.md "Mesh holes", tests/bowtie_numpy.py): boundary darts are paired across the hole they bound, so
// the rims of holes that meet in a vertex close.  Between keys .. darts above and measure, emit above:
//   dkeys    one thread per face: the directed edge keys tail V + head of a counting face in dart order, INT64_MAX else.
//   (caller)   sorts them, stable, with the permutation; gathers the keys of the boundary darts and sorts those too.
//   fan      one thread per boundary dart u -> v: rotates about v, from the dart's face across interior edges, until the
//            edge after the one it came in by is a boundary dart: fan(d).  An edge is crossed only when it and its reverse
//            occur exactly once among the sorted keys; at most as many steps as keys have the tail v.
//   (caller)   sorts the successors.
//   claim    one thread per boundary dart: state = (fan(d) when nobody else claims it, else none; name), name = the
//            position of the dart's key among the sorted keys of the boundary darts.
//   double   as above: ptr >= 0 exactly on the closed walks of fan, lab = the walk's smallest name.
//   rank_init, rank_double   the same doubling kernel over (successor, steps), adding steps where double takes the
//            minimum, cut in front of the walk's first dart: steps becomes the distance to that dart along fan, n for the
//            first dart itself, so n - steps is the rank.
//   walk_keys  label B + (B - steps): the order by (walk, rank).  (caller) sorts with the permutation.
//   pair_keys  in that order, head B + label.  (caller) sorts, stable: runs of one (head, walk) by ascending rank.
//   repair   one thread per sorted slot: the ends of its run by binary search, next(d_m) = fan(d_(m-1 mod k)).
//   double   on (next, name): the cycles of next and their smallest names.
//   tail_keys, tail_flag   label V + tail, sorted by the caller; a repeated key stores 1 to the flag of that label (many
//            lanes may store the same byte; nobody reads it in that launch).
//   loop_labels, loop_assign   as above, with the flag: without the flagged cycles; a label is a name, so the first dart
//            is found by its name, and its tail and head are the loop's id and head.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mh_dkeys_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                       int64_t* __restrict__ keys) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  const bool ok = tp_counts(a, b, c, nv);
  int64_t* k = keys + 3 * (size_t)f;
  k[0] = ok ? (int64_t)a * nv + b : kMhNoKey;
  k[1] = ok ? (int64_t)b * nv + c : kMhNoKey;
  k[2] = ok ? (int64_t)c * nv + a : kMhNoKey;
}

__global__ __launch_bounds__(256) void mh_fan_kernel(const int32_t* __restrict__ faces, int nf, int nv,
                                                     const int32_t* __restrict__ dart,
                                                     const int32_t* __restrict__ head, int nb,
                                                     const int64_t* __restrict__ sorted_keys,
                                                     const int64_t* __restrict__ key_order, int32_t* __restrict__ fan) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int64_t n = 3 * (int64_t)nf;
  const int v = head[i];
  int64_t s = dart[i];
  int out = -1;
  if ((uint64_t)s < (uint64_t)n && (unsigned)v < (unsigned)nv) {
    const int64_t row = (int64_t)v * nv;
    const int64_t bound = tp_lower(sorted_keys, n, row + nv) - tp_lower(sorted_keys, n, row);
    for (int64_t step = 0; step < bound; step++) {
      const int64_t f = s / 3;
      const int c = (int)(s - 3 * f), c1 = c == 2 ? 0 : c + 1, c2 = c1 == 2 ? 0 : c1 + 1;
      const int w = faces[3 * f + c2];
      if (faces[3 * f + c1] != v || (unsigned)w >= (unsigned)nv) break;    // the edge after s in its face is v -> w
      const int p = tp_once(dart, nb, (int)(3 * f + c1));
      if (p >= 0) { out = p; break; }
      const int64_t q = tp_once(sorted_keys, n, (int64_t)w * nv + v);
      if (q < 0 || tp_once(sorted_keys, n, row + w) < 0) break;
      s = key_order[q];
      if ((uint64_t)s >= (uint64_t)n) break;
    }
  }
  fan[i] = out;
}

__global__ __launch_bounds__(256) void mh_claim_kernel(const int32_t* __restrict__ fan,
                                                       const int32_t* __restrict__ sorted_fan,
                                                       const int64_t* __restrict__ dart_key,
                                                       const int64_t* __restrict__ sorted_dart_key, int nb,
                                                       int2* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int s = fan[i];
  const bool mine = (unsigned)s < (unsigned)nb && tp_once(sorted_fan, nb, s) >= 0;
  state[i] = make_int2(mine ? s : -1, (int)tp_lower(sorted_dart_key, (int64_t)nb, dart_key[i]));
}

__global__ __launch_bounds__(256) void mh_rank_init_kernel(const int2* __restrict__ state,
                                                           const int2* __restrict__ labelled, int nb,
                                                           int2* __restrict__ rank) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  int2 r = make_int2(-1, 0);
  const int s = state[i].x;
  if (labelled[i].x >= 0 && (unsigned)s < (unsigned)nb) {
    r.y = 1;
    if (state[s].y != labelled[i].y) r.x = s;             // the walk's first dart carries the label as its name
  }
  rank[i] = r;
}

__global__ __launch_bounds__(256) void mh_walk_keys_kernel(const int2* __restrict__ labelled,
                                                           const int2* __restrict__ rank, int nb,
                                                           int64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int2 l = labelled[i];
  const int steps = rank[i].y;
  const bool ok = l.x >= 0 && (unsigned)l.y < (unsigned)nb && steps >= 1 && steps <= nb;
  keys[i] = ok ? (int64_t)l.y * nb + (nb - steps) : kMhNoKey;
}

__global__ __launch_bounds__(256) void mh_pair_keys_kernel(const int2* __restrict__ labelled,
                                                           const int32_t* __restrict__ head,
                                                           const int64_t* __restrict__ sorted_walk_keys,
                                                           const int64_t* __restrict__ walk_order, int nb, int nv,
                                                           int64_t* __restrict__ keys) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  const int64_t d = walk_order[j];
  int64_t k = kMhNoKey;
  if (sorted_walk_keys[j] != kMhNoKey && (uint64_t)d < (uint64_t)nb) {
    const int h = head[d], l = labelled[d].y;
    if ((unsigned)h < (unsigned)nv && (unsigned)l < (unsigned)nb) k = (int64_t)h * nb + l;
  }
  keys[j] = k;
}

// the dart in slot j of the order by (head, walk, rank), or -1
__device__ __forceinline__ int mh_slot_dart(const int64_t* __restrict__ pair_order,
                                            const int64_t* __restrict__ walk_order, int64_t j, int nb) {
  const int64_t a = pair_order[j];
  if ((uint64_t)a >= (uint64_t)nb) return -1;
  const int64_t d = walk_order[a];
  return (uint64_t)d < (uint64_t)nb ? (int)d : -1;
}

__global__ __launch_bounds__(256) void mh_repair_kernel(const int64_t* __restrict__ sorted_pair_keys,
                                                        const int64_t* __restrict__ pair_order,
                                                        const int64_t* __restrict__ walk_order,
                                                        const int2* __restrict__ state, int nb,
                                                        int2* __restrict__ paired) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  const int d = mh_slot_dart(pair_order, walk_order, j, nb);
  if (d < 0) return;
  const int64_t k = sorted_pair_keys[j];
  int nxt = -1;
  if (k != kMhNoKey) {
    const int64_t n = nb, lo = tp_lower(sorted_pair_keys, n, k), hi = tp_lower(sorted_pair_keys, n, k + 1);
    const int64_t prev = j == lo ? hi - 1 : (int64_t)j - 1;
    const int dp = prev >= 0 && prev < nb ? mh_slot_dart(pair_order, walk_order, prev, nb) : -1;
    if (dp >= 0) {
      const int s = state[dp].x;
      if ((unsigned)s < (unsigned)nb) nxt = s;
    }
  }
  paired[d] = make_int2(nxt, state[d].y);
}

__global__ __launch_bounds__(256) void mh_tail_keys_kernel(const int2* __restrict__ labelled,
                                                           const int32_t* __restrict__ tail, int nb, int nv,
                                                           int64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nb) return;
  const int2 l = labelled[i];
  const int t = tail[i];
  const bool ok = l.x >= 0 && (unsigned)l.y < (unsigned)nb && (unsigned)t < (unsigned)nv;
  keys[i] = ok ? (int64_t)l.y * nv + t : kMhNoKey;
}

__global__ __launch_bounds__(256) void mh_tail_flag_kernel(const int64_t* __restrict__ sorted_keys, int nb, int nv,
                                                           uint8_t* __restrict__ flag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nb || j == 0) return;
  const int64_t k = sorted_keys[j];
  if (k == kMhNoKey || sorted_keys[j - 1] != k) return;
  const int64_t l = k / nv;
  if ((uint64_t)l < (uint64_t)nb) flag[l] = 1;
}

}  // namespace mslam

using namespace mslam;

// What the entry points repeat, spelled once.  A state is i32[B,2], read and written as int2, hence 8-byte aligned.
#define MH_STATE(p) reinterpret_cast<const int2*>(p)
#define MH_STATE_OUT(p) reinterpret_cast<int2*>(p)
#define MH_ALIGNED(p) ((uintptr_t)(p) % 8 == 0)
#define MH_SIZES(name, ok) MSLAM_REQUIRE(ok, name ": negative size")
#define MH_FACES(name, nf) MSLAM_REQUIRE((int64_t)(nf) * 3 < ((int64_t)1 << 31), name ": too many faces")
// one thread per element in blocks of 256, the launch check, and the entry point's return
#define MH_RUN(name, kernel, count, ...)                                                                     \
  hipLaunchKernelGGL(kernel, dim3(blocks_for(count, 256)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
  MSLAM_LAUNCH_CHECK(name);                                                                                  \
  return MSLAM_OK

extern "C" int mslam_mesh_holes_keys(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys,
                                     void* stream) {
  MH_SIZES("mesh_holes_keys", num_faces >= 0 && num_vertices >= 0);
  MH_FACES("mesh_holes_keys", num_faces);
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && keys, "mesh_holes_keys: null pointer");
  MH_RUN("mesh_holes_keys", mh_keys_kernel, num_faces, faces, num_faces, num_vertices, keys);
}

extern "C" int mslam_mesh_holes_mark(const int64_t* sorted_keys, const int64_t* order, int64_t num_keys, uint8_t* flag,
                                     void* stream) {
  MSLAM_REQUIRE(num_keys >= 0 && num_keys < ((int64_t)1 << 31), "mesh_holes_mark: size outside [0, 2^31)");
  if (num_keys == 0) return MSLAM_OK;
  MSLAM_REQUIRE(sorted_keys && order && flag, "mesh_holes_mark: null pointer");
  MH_RUN("mesh_holes_mark", mh_mark_kernel, num_keys, sorted_keys, order, num_keys, flag);
}

extern "C" int mslam_mesh_holes_darts(const int32_t* faces, int num_faces, int num_vertices, const int32_t* dart,
                                      int num_darts, int32_t* tail, int32_t* head, void* stream) {
  MH_SIZES("mesh_holes_darts", num_faces >= 0 && num_vertices >= 0 && num_darts >= 0);
  MH_FACES("mesh_holes_darts", num_faces);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(dart && tail && head && (faces || num_faces == 0), "mesh_holes_darts: null pointer");
  MH_RUN("mesh_holes_darts", mh_darts_kernel, num_darts, faces, num_faces, num_vertices, dart, num_darts, tail, head);
}

extern "C" int mslam_mesh_holes_link(const int32_t* tail, const int32_t* head, const int32_t* sorted_tail,
                                     const int64_t* tail_order, const int32_t* sorted_head, int num_darts,
                                     int num_vertices, int32_t* state, void* stream) {
  MH_SIZES("mesh_holes_link", num_darts >= 0 && num_vertices >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(tail && head && sorted_tail && tail_order && sorted_head && state, "mesh_holes_link: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(state), "mesh_holes_link: state must be 8-byte aligned");
  MH_RUN("mesh_holes_link", mh_link_kernel, num_darts, tail, head, sorted_tail, tail_order, sorted_head, num_darts,
         num_vertices, MH_STATE_OUT(state));
}

extern "C" int mslam_mesh_holes_double(const int32_t* state_in, int32_t* state_out, int num_darts, void* stream) {
  MH_SIZES("mesh_holes_double", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(state_in && state_out && state_in != state_out, "mesh_holes_double: null pointer or out == in");
  MSLAM_REQUIRE(MH_ALIGNED(state_in) && MH_ALIGNED(state_out), "mesh_holes_double: states must be 8-byte aligned");
  MH_RUN("mesh_holes_double", mh_double_kernel<MhMinLabel>, num_darts, MH_STATE(state_in), MH_STATE_OUT(state_out),
         num_darts);
}

extern "C" int mslam_mesh_holes_loop_labels(const int32_t* labelled, const uint8_t* flag, int num_darts, int32_t* keys,
                                            void* stream) {
  MSLAM_REQUIRE(num_darts >= 0 && num_darts < INT32_MAX, "mesh_holes_loop_labels: size outside [0, 2^31 - 1)");
  MSLAM_REQUIRE(keys && (labelled || num_darts == 0), "mesh_holes_loop_labels: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(labelled), "mesh_holes_loop_labels: state must be 8-byte aligned");
  MH_RUN("mesh_holes_loop_labels", mh_loop_labels_kernel, (int64_t)num_darts + 1, MH_STATE(labelled), flag, num_darts,
         keys);
}

extern "C" int mslam_mesh_holes_loop_assign(const int32_t* labelled, const int32_t* own, const uint8_t* flag,
                                            const int32_t* tail, const int32_t* head, int num_darts,
                                            const int32_t* loop_name, int num_loops, int32_t* dart_loop, int32_t* start,
                                            int32_t* loop_id, int32_t* loop_head, void* stream) {
  MH_SIZES("mesh_holes_loop_assign", num_darts >= 0 && num_loops >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(labelled && own && dart_loop && (num_loops == 0 || (loop_name && start)) && (tail || !loop_id) &&
                    (head || !loop_head),
                "mesh_holes_loop_assign: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(labelled) && MH_ALIGNED(own), "mesh_holes_loop_assign: states must be 8-byte aligned");
  MH_RUN("mesh_holes_loop_assign", mh_loop_assign_kernel, num_darts, MH_STATE(labelled), MH_STATE(own), flag, tail,
         head, num_darts, loop_name, num_loops, dart_loop, start, loop_id, loop_head);
}

extern "C" int mslam_mesh_holes_measure(const float* vertices, const int32_t* faces, int num_faces, int num_vertices,
                                        const int32_t* dart, const int32_t* tail, const int32_t* head,
                                        const int32_t* state, int num_darts, const int32_t* start,
                                        const int32_t* length, int num_loops, int max_edges, int all_perimeters,
                                        double* perimeter, double* centre, uint8_t* fillable, void* stream) {
  MH_SIZES("mesh_holes_measure", num_faces >= 0 && num_vertices >= 0 && num_darts >= 0 && num_loops >= 0);
  MH_FACES("mesh_holes_measure", num_faces);
  if (num_loops == 0) return MSLAM_OK;
  MSLAM_REQUIRE(start && length && perimeter && centre && fillable, "mesh_holes_measure: null pointer");
  MSLAM_REQUIRE(num_darts == 0 || (vertices && faces && dart && tail && head && state),
                "mesh_holes_measure: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(state), "mesh_holes_measure: state must be 8-byte aligned");
  MH_RUN("mesh_holes_measure", mh_measure_kernel, num_loops, vertices, faces, num_faces, num_vertices, dart, tail, head,
         MH_STATE(state), num_darts, start, length, num_loops, max_edges, all_perimeters, perimeter, centre, fillable);
}

extern "C" int mslam_mesh_holes_emit(const float* vertices, const float* colors, const int32_t* tail,
                                     const int32_t* head, const int32_t* state, int num_darts, const int32_t* start,
                                     const int32_t* length, const uint8_t* fillable, const int64_t* vertex_base,
                                     const int64_t* face_base, int num_loops, int num_vertices, int num_faces,
                                     int new_vertices, int new_faces, const double* centre, float* out_vertices,
                                     float* out_normals, float* out_colors, int32_t* out_faces, void* stream) {
  MH_SIZES("mesh_holes_emit", num_darts >= 0 && num_loops >= 0 && num_vertices >= 0 && num_faces >= 0 &&
                                  new_vertices >= 0 && new_faces >= 0);
  MSLAM_REQUIRE((int64_t)num_vertices + new_vertices < ((int64_t)1 << 31) &&
                    ((int64_t)num_faces + new_faces) * 3 < ((int64_t)1 << 31),
                "mesh_holes_emit: the output leaves the int32 index range");
  if (num_loops == 0 || new_vertices == 0) return MSLAM_OK;
  MSLAM_REQUIRE(vertices && tail && head && state && start && length && fillable && vertex_base && face_base &&
                    centre && out_vertices && out_normals && out_faces,
                "mesh_holes_emit: null pointer");
  MSLAM_REQUIRE((colors == nullptr) == (out_colors == nullptr), "mesh_holes_emit: colors and out_colors go together");
  MSLAM_REQUIRE(MH_ALIGNED(state), "mesh_holes_emit: state must be 8-byte aligned");
  MH_RUN("mesh_holes_emit", mh_emit_kernel, num_loops, vertices, colors, tail, head, MH_STATE(state), num_darts, start,
         length, fillable, vertex_base, face_base, num_loops, num_vertices, num_faces, new_vertices, new_faces, centre,
         out_vertices, out_normals, out_colors, out_faces);
}

// ---- bow-tie mode ----------------------------------------------------------------------------------------------------
extern "C" int mslam_mesh_holes_dkeys(const int32_t* faces, int num_faces, int num_vertices, int64_t* keys,
                                      void* stream) {
  MH_SIZES("mesh_holes_dkeys", num_faces >= 0 && num_vertices >= 0);
  MH_FACES("mesh_holes_dkeys", num_faces);
  if (num_faces == 0) return MSLAM_OK;
  MSLAM_REQUIRE(faces && keys, "mesh_holes_dkeys: null pointer");
  MH_RUN("mesh_holes_dkeys", mh_dkeys_kernel, num_faces, faces, num_faces, num_vertices, keys);
}

extern "C" int mslam_mesh_holes_fan(const int32_t* faces, int num_faces, int num_vertices, const int32_t* dart,
                                    const int32_t* head, int num_darts, const int64_t* sorted_keys,
                                    const int64_t* key_order, int32_t* fan, void* stream) {
  MH_SIZES("mesh_holes_fan", num_faces >= 0 && num_vertices >= 0 && num_darts >= 0);
  MH_FACES("mesh_holes_fan", num_faces);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(dart && head && fan && (num_faces == 0 || (faces && sorted_keys && key_order)),
                "mesh_holes_fan: null pointer");
  MH_RUN("mesh_holes_fan", mh_fan_kernel, num_darts, faces, num_faces, num_vertices, dart, head, num_darts, sorted_keys,
         key_order, fan);
}

extern "C" int mslam_mesh_holes_claim(const int32_t* fan, const int32_t* sorted_fan, const int64_t* dart_key,
                                      const int64_t* sorted_dart_key, int num_darts, int32_t* state, void* stream) {
  MH_SIZES("mesh_holes_claim", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(fan && sorted_fan && dart_key && sorted_dart_key && state, "mesh_holes_claim: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(state), "mesh_holes_claim: state must be 8-byte aligned");
  MH_RUN("mesh_holes_claim", mh_claim_kernel, num_darts, fan, sorted_fan, dart_key, sorted_dart_key, num_darts,
         MH_STATE_OUT(state));
}

extern "C" int mslam_mesh_holes_rank_init(const int32_t* state, const int32_t* labelled, int num_darts, int32_t* rank,
                                          void* stream) {
  MH_SIZES("mesh_holes_rank_init", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(state && labelled && rank, "mesh_holes_rank_init: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(state) && MH_ALIGNED(labelled) && MH_ALIGNED(rank),
                "mesh_holes_rank_init: states must be 8-byte aligned");
  MH_RUN("mesh_holes_rank_init", mh_rank_init_kernel, num_darts, MH_STATE(state), MH_STATE(labelled), num_darts,
         MH_STATE_OUT(rank));
}

extern "C" int mslam_mesh_holes_rank_double(const int32_t* rank_in, int32_t* rank_out, int num_darts, void* stream) {
  MH_SIZES("mesh_holes_rank_double", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(rank_in && rank_out && rank_in != rank_out, "mesh_holes_rank_double: null pointer or out == in");
  MSLAM_REQUIRE(MH_ALIGNED(rank_in) && MH_ALIGNED(rank_out), "mesh_holes_rank_double: states must be 8-byte aligned");
  MH_RUN("mesh_holes_rank_double", mh_double_kernel<MhSumSteps>, num_darts, MH_STATE(rank_in), MH_STATE_OUT(rank_out),
         num_darts);
}

extern "C" int mslam_mesh_holes_walk_keys(const int32_t* labelled, const int32_t* rank, int num_darts, int64_t* keys,
                                          void* stream) {
  MH_SIZES("mesh_holes_walk_keys", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(labelled && rank && keys, "mesh_holes_walk_keys: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(labelled) && MH_ALIGNED(rank), "mesh_holes_walk_keys: states must be 8-byte aligned");
  MH_RUN("mesh_holes_walk_keys", mh_walk_keys_kernel, num_darts, MH_STATE(labelled), MH_STATE(rank), num_darts, keys);
}

extern "C" int mslam_mesh_holes_pair_keys(const int32_t* labelled, const int32_t* head,
                                          const int64_t* sorted_walk_keys, const int64_t* walk_order, int num_darts,
                                          int num_vertices, int64_t* keys, void* stream) {
  MH_SIZES("mesh_holes_pair_keys", num_darts >= 0 && num_vertices >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(labelled && head && sorted_walk_keys && walk_order && keys, "mesh_holes_pair_keys: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(labelled), "mesh_holes_pair_keys: state must be 8-byte aligned");
  MH_RUN("mesh_holes_pair_keys", mh_pair_keys_kernel, num_darts, MH_STATE(labelled), head, sorted_walk_keys, walk_order,
         num_darts, num_vertices, keys);
}

extern "C" int mslam_mesh_holes_repair(const int64_t* sorted_pair_keys, const int64_t* pair_order,
                                       const int64_t* walk_order, const int32_t* state, int num_darts, int32_t* paired,
                                       void* stream) {
  MH_SIZES("mesh_holes_repair", num_darts >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(sorted_pair_keys && pair_order && walk_order && state && paired && state != paired,
                "mesh_holes_repair: null pointer or out == in");
  MSLAM_REQUIRE(MH_ALIGNED(state) && MH_ALIGNED(paired), "mesh_holes_repair: states must be 8-byte aligned");
  MH_RUN("mesh_holes_repair", mh_repair_kernel, num_darts, sorted_pair_keys, pair_order, walk_order, MH_STATE(state),
         num_darts, MH_STATE_OUT(paired));
}

extern "C" int mslam_mesh_holes_tail_keys(const int32_t* labelled, const int32_t* tail, int num_darts, int num_vertices,
                                          int64_t* keys, void* stream) {
  MH_SIZES("mesh_holes_tail_keys", num_darts >= 0 && num_vertices >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(labelled && tail && keys, "mesh_holes_tail_keys: null pointer");
  MSLAM_REQUIRE(MH_ALIGNED(labelled), "mesh_holes_tail_keys: state must be 8-byte aligned");
  MH_RUN("mesh_holes_tail_keys", mh_tail_keys_kernel, num_darts, MH_STATE(labelled), tail, num_darts, num_vertices,
         keys);
}

extern "C" int mslam_mesh_holes_tail_flag(const int64_t* sorted_keys, int num_darts, int num_vertices, uint8_t* flag,
                                          void* stream) {
  MH_SIZES("mesh_holes_tail_flag", num_darts >= 0 && num_vertices >= 0);
  if (num_darts == 0) return MSLAM_OK;
  MSLAM_REQUIRE(num_vertices > 0, "mesh_holes_tail_flag: darts without vertices");
  MSLAM_REQUIRE(sorted_keys && flag, "mesh_holes_tail_flag: null pointer");
  MH_RUN("mesh_holes_tail_flag", mh_tail_flag_kernel, num_darts, sorted_keys, num_darts, num_vertices, flag);
}
