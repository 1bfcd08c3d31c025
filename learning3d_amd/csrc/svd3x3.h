// svd3x3.h -- the 3x3 rotation head shared by svd.hip (l3d_svd3x3_rotation, l3d_kabsch) and deepgmr.hip (l3d_gmm_register):
// one-sided (Hestenes) Jacobi SVD in fp64 registers with the reflection fix, for a single lane.
#pragma once
#include <hip/hip_runtime.h>

// R = V U^T from H = U S V^T, with det fix: if det(V U^T) < 0 negate the column of V that belongs
// to the SMALLEST singular value (the reference multiplies V by diag(1,1,-1) with LAPACK's
// descending order, utils/svd.py:41-45).
__device__ static void rotation_from_H(const double Hin[9], float Rout[9])
{
    // columns of W start as columns of H; V accumulates the right rotations:  H V = W
    double W[3][3], V[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { W[r][c] = Hin[r * 3 + c]; V[r][c] = (r == c) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 12; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; r++) {
                    alpha += W[r][p] * W[r][p];
                    beta += W[r][q] * W[r][q];
                    gamma += W[r][p] * W[r][q];
                }
                if (gamma == 0.0) continue;
                off = fmax(off, fabs(gamma) / sqrt(fmax(alpha * beta, 1e-300)));
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; r++) {
                    const double wp = W[r][p], wq = W[r][q];
                    W[r][p] = cs * wp - sn * wq;
                    W[r][q] = sn * wp + cs * wq;
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = cs * vp - sn * vq;
                    V[r][q] = sn * vp + cs * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double sig[3];
    for (int c = 0; c < 3; c++)
        sig[c] = sqrt(W[0][c] * W[0][c] + W[1][c] * W[1][c] + W[2][c] * W[2][c]);
    // order: i0 largest ... i2 smallest
    int i0 = 0, i1 = 1, i2 = 2;
    if (sig[i0] < sig[i1]) { int t = i0; i0 = i1; i1 = t; }
    if (sig[i1] < sig[i2]) { int t = i1; i1 = i2; i2 = t; }
    if (sig[i0] < sig[i1]) { int t = i0; i0 = i1; i1 = t; }
    double U[3][3];
    const double tiny = 1e-14 * fmax(sig[i0], 1e-300);
    // two leading left vectors (fall back to any orthonormal completion when degenerate)
    for (int r = 0; r < 3; r++) U[r][i0] = sig[i0] > 0 ? W[r][i0] / sig[i0] : (r == 0 ? 1.0 : 0.0);
    if (sig[i1] > tiny) {
        for (int r = 0; r < 3; r++) U[r][i1] = W[r][i1] / sig[i1];
    } else {
        // any unit vector orthogonal to U[:,i0]
        int m = fabs(U[0][i0]) < fabs(U[1][i0]) ? (fabs(U[0][i0]) < fabs(U[2][i0]) ? 0 : 2)
                                                : (fabs(U[1][i0]) < fabs(U[2][i0]) ? 1 : 2);
        double e[3] = {0, 0, 0}; e[m] = 1.0;
        double d = U[m][i0], nn = 0;
        for (int r = 0; r < 3; r++) { e[r] -= d * U[r][i0]; nn += e[r] * e[r]; }
        nn = sqrt(nn);
        for (int r = 0; r < 3; r++) U[r][i1] = e[r] / nn;
    }
    if (sig[i2] > tiny) {
        for (int r = 0; r < 3; r++) U[r][i2] = W[r][i2] / sig[i2];
    } else {
        U[0][i2] = U[1][i0] * U[2][i1] - U[2][i0] * U[1][i1];
        U[1][i2] = U[2][i0] * U[0][i1] - U[0][i0] * U[2][i1];
        U[2][i2] = U[0][i0] * U[1][i1] - U[1][i0] * U[0][i1];
    }
    double R[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            R[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + V[r][2] * U[c][2];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) -
                       R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0)
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[r][c] -= 2.0 * V[r][i2] * U[c][i2];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rout[r * 3 + c] = (float)R[r][c];
}
