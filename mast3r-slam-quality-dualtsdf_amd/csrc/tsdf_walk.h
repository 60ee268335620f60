// The ray walk of one fused point of the global TSDF (global_volume.py:51-71 of the reference), stated once for the two
// kernels that must visit the same voxels: tsdf_emit_kernel (csrc/tsdf_global.hip) creates a voxel for every sample it
// accepts, color_fuse_kernel (csrc/tsdf_color.hip) finds that voxel again by its key.  A rounding or a gate that
// differed between them would put colour into voxels the TSDF never made, with no error anywhere.  Every fp32 step that
// feeds the key is the reference's float32 operation in the same order; both TUs are built with -ffp-contract=off.
#pragma once
#include "tsdf_table.h"

namespace mslam {

// distance between two samples of a ray: `step = max(voxel_size * step_scale, 1e-4)`
static inline double integrate_step(double voxel_size, double step_scale) {
  const double step = voxel_size * step_scale;
  return step < 1.0e-4 ? 1.0e-4 : step;
}

// the most samples a point can have in band.  The walk starts up to three samples early, so the colour fuse, which
// gives every sample from k0 on a band position of its own, launches max_band_for(..) + 4 positions per point.
static inline int max_band_for(double voxel_size, double trunc, double step_scale) {
  return (int)(2.0 * trunc / integrate_step(voxel_size, step_scale)) + 4;
}

// np.linspace(0, maxd, num) along origin + dist * d; the in-band samples (|L - dist| <= trunc) are a contiguous index
// range that starts at k0 or up to three samples after it
struct RayWalk {
  float o[3], d[3];
  float L, maxd, lstep;
  int num, k0;
};

enum WalkBegin {
  kWalkNoRay,    // the length is not finite or below 1e-4: the reference skips the point
  kWalkTooLong,  // more than 2^20 samples: a fused point that is dropped and reported (only d and maxd are set)
  kWalkOk,
};

__device__ __forceinline__ WalkBegin walk_begin(const float* __restrict__ points, size_t i,
                                                const float* __restrict__ origin, float stepf, float truncf,
                                                RayWalk& r) {
  r.o[0] = origin[0]; r.o[1] = origin[1]; r.o[2] = origin[2];
  const float r0 = points[3 * i] - r.o[0], r1 = points[3 * i + 1] - r.o[1], r2 = points[3 * i + 2] - r.o[2];
  // np.linalg.norm: sqrt(sdot) with float products accumulated in double (OpenBLAS), rounded once
  const float sq = (float)(((double)(r0 * r0) + (double)(r1 * r1)) + (double)(r2 * r2));
  r.L = sqrtf(sq);
  if (!isfinite(r.L) || r.L < 1.0e-4f) return kWalkNoRay;
  r.d[0] = r0 / r.L; r.d[1] = r1 / r.L; r.d[2] = r2 / r.L;
  r.maxd = r.L + truncf;
  // A ray of more than 2^20 samples (15 km at the default 1.5 cm step) only occurs when a pose has diverged; the
  // reference would spend minutes in np.linspace there.
  if (!(r.maxd / stepf < 1048576.0f)) return kWalkTooLong;
  r.num = (int)(r.maxd / stepf);
  if (r.num < 1) r.num = 1;
  r.lstep = r.num > 1 ? r.maxd / (float)(r.num - 1) : 0.0f;
  r.k0 = r.num > 1 ? (int)((r.L - truncf) / r.lstep) - 2 : 0;
  if (r.k0 < 0) r.k0 = 0;
  return kWalkOk;
}

struct WalkSample {
  float tv;      // sdf / trunc, clamped to [-1, 1]
  double w;      // conf * exp(-|sdf| / trunc)
  uint64_t key;
};

enum WalkStep {
  kSampleBefore,    // out of band in front of the surface
  kSampleBehind,    // out of band behind the surface: of the later samples only the exact end point num - 1 can be in band
  kSampleNoWeight,  // `if weight <= 0.0: return` (NaN weights fall through in python; not fused here)
  kSampleNoKey,     // in band, but the position has no voxel (tsdf_table.h world_to_key)
  kSampleOk,
};

// sample k in [0, num) of the walk; `s` is complete only for kSampleOk
__device__ __forceinline__ WalkStep walk_sample(const RayWalk& r, int k, double cf, float vs, float truncf,
                                                WalkSample& s) {
  float dist;
  if (r.num == 1) dist = 0.0f;
  else if (k == r.num - 1) dist = r.maxd;
  else dist = (float)k * r.lstep;
  const float sdf = r.L - dist;
  if (fabsf(sdf) > truncf) return sdf < 0.0f ? kSampleBehind : kSampleBefore;
  const float s0 = r.o[0] + dist * r.d[0], s1 = r.o[1] + dist * r.d[1], s2 = r.o[2] + dist * r.d[2];
  s.tv = fminf(fmaxf(sdf / truncf, -1.0f), 1.0f);
  const float e = -fabsf(sdf) / truncf;
  s.w = cf * exp((double)e);
  if (!(s.w > 0.0)) return kSampleNoWeight;
  return world_to_key(s0, s1, s2, vs, s.key) ? kSampleOk : kSampleNoKey;
}

}  // namespace mslam
