// Cyclic Jacobi on a symmetric 3 x 3 matrix in f64 (ma_jacobi4 of mesh_align.hip restated for 3 x 3, unrolled with
// constant indices): what kn_normals_kernel of cloud_knn.hip takes a normal from and ip_solve_kernel of icp_plane.hip
// the spread of the normals.  tests/cloud_knn_numpy.py `jacobi3` is this, operation by operation.
#pragma once
#include <math.h>

#include "common.h"

namespace mslam {

// One rotation of the cyclic Jacobi sweep on the pair (P, Q): ma_jacobi4's, with constant indices
template <int P, int Q>
__device__ __forceinline__ void kn_rotate(double (&A)[3][3], double (&V)[3][3]) {
  if (A[P][Q] == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * A[P][Q]);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
  for (int r = 0; r < 3; r++) {                              // A <- A J
    const double akp = A[r][P], akq = A[r][Q];
    A[r][P] = cs * akp - sn * akq;
    A[r][Q] = sn * akp + cs * akq;
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {                              // A <- J^T A
    const double apk = A[P][r], aqk = A[Q][r];
    A[P][r] = cs * apk - sn * aqk;
    A[Q][r] = sn * apk + cs * aqk;
  }
#pragma unroll
  for (int r = 0; r < 3; r++) {                              // V <- V J
    const double vkp = V[r][P], vkq = V[r][Q];
    V[r][P] = cs * vkp - sn * vkq;
    V[r][Q] = sn * vkp + cs * vkq;
  }
}

// Up to 16 sweeps over (0, 1), (0, 2), (1, 2): A's diagonal becomes the eigenvalues, V (the identity on entry) gains
// the eigenvectors as columns.  Before each sweep the squares of the off-diagonal and of the diagonal entries are summed
// in row-major order, and the sweeps end unless off > 2^-104 diag.
__device__ __forceinline__ void kn_jacobi3(double (&A)[3][3], double (&V)[3][3]) {
  for (int sweep = 0; sweep < 16; sweep++) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
      for (int b = 0; b < 3; b++) {
        if (a == b) diag += A[a][b] * A[a][b];
        else off += A[a][b] * A[a][b];
      }
    }
    if (!(off > 0x1p-104 * diag)) break;                     // off-diagonal norm below 2^-52 of the diagonal's
    kn_rotate<0, 1>(A, V);
    kn_rotate<0, 2>(A, V);
    kn_rotate<1, 2>(A, V);
  }
}

}  // namespace mslam
