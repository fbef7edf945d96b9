// p2c_procrustes_dev.h -- the 3x3 orthogonal Procrustes problem of PA-MPJPE, solved per frame without a library (K22).
//
// Given H = X0^T Y0 (target^T prediction, both centred and scaled to unit Frobenius norm), metrics/extra_metrics.py:p_mpjpe
// takes H = U S V^T, R = V U^T, flips the smallest singular direction when det R < 0, and uses R and the signed sum of the
// singular values. That R is the proper rotation maximising tr(H R), and the signed sum is the maximum itself. Horn's
// closed form (J. Opt. Soc. Am. A 4, 1987) reaches both without an SVD and without a reflection case: the maximum is the
// largest eigenvalue of a symmetric 4x4 matrix built from H, and its eigenvector is the rotation as a unit quaternion. The
// eigenproblem is solved by cyclic Jacobi in fp64 with a FIXED number of sweeps and no data-dependent exit; NaN inputs run the
// same instructions and come out as NaN.
#pragma once

#if defined(__HIPCC__)
#define P2C_HD __host__ __device__ __forceinline__
#else
#define P2C_HD inline
#endif

namespace p2c_procrustes {

constexpr int SWEEPS = 8;        // cyclic Jacobi converges quadratically: random and graded 4x4 are at round-off after 5

// one Jacobi rotation in the (P, Q) plane of the symmetric A; the eigenvector matrix V accumulates the rotations
template <int P, int Q>
P2C_HD void rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q], d = A[Q][Q] - A[P][P];
  const double r = sqrt(d * d + 4.0 * apq * apq);
  const double den = d + copysign(r, d);                   // t = tan of the rotation angle, the smaller root
  const double t = (den != 0.0) ? 2.0 * apq / den : 0.0;    // den == 0 only when apq == 0 and d == 0; NaN stays NaN
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
  A[P][P] -= t * apq, A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k != P && k != Q) {
      const double akp = A[k][P], akq = A[k][Q];
      A[k][P] = A[P][k] = c * akp - s * akq;
      A[k][Q] = A[Q][k] = s * akp + c * akq;
    }
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// H[a][b] = sum_j X0[j][a] * Y0[j][b]. Out: R (row-vector convention, aligned = y R) and the signed singular-value sum.
P2C_HD void solve(const double (&H)[3][3], double (&R)[3][3], double &signed_sum) {
  // Horn's S_ab = sum (rotated cloud)_a (fixed cloud)_b = sum y_a x_b = H[b][a]
  const double Sxx = H[0][0], Sxy = H[1][0], Sxz = H[2][0];
  const double Syx = H[0][1], Syy = H[1][1], Syz = H[2][1];
  const double Szx = H[0][2], Szy = H[1][2], Szz = H[2][2];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    rotate<0, 1>(A, V), rotate<0, 2>(A, V), rotate<0, 3>(A, V);
    rotate<1, 2>(A, V), rotate<1, 3>(A, V), rotate<2, 3>(A, V);
  }
  // largest eigenvalue and its eigenvector, by selection (a NaN diagonal selects column 0, which is NaN too)
  double lam = A[0][0], q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = A[k][k] > lam;
    lam = up ? A[k][k] : lam;
    q0 = up ? V[0][k] : q0, qx = up ? V[1][k] : qx, qy = up ? V[2][k] : qy, qz = up ? V[3][k] : qz;
  }
  const double n = 1.0 / sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);    // the product of rotations is unit to round-off
  q0 *= n, qx *= n, qy *= n, qz *= n;
  // the quaternion's matrix Q takes the prediction onto the target as columns (x ~ Q y); as rows that is y R with R = Q^T
  R[0][0] = q0 * q0 + qx * qx - qy * qy - qz * qz, R[1][0] = 2.0 * (qx * qy - q0 * qz), R[2][0] = 2.0 * (qx * qz + q0 * qy);
  R[0][1] = 2.0 * (qy * qx + q0 * qz), R[1][1] = q0 * q0 - qx * qx + qy * qy - qz * qz, R[2][1] = 2.0 * (qy * qz - q0 * qx);
  R[0][2] = 2.0 * (qz * qx - q0 * qy), R[1][2] = 2.0 * (qz * qy + q0 * qx), R[2][2] = q0 * q0 - qx * qx - qy * qy + qz * qz;
  signed_sum = lam;
}

}  // namespace p2c_procrustes
