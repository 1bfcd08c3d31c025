// se3_exp.h -- se3.exp (ops/se3.py:51-74) on the device, shared by the data feed (feed.hip) and the registration loop
// (registration.hip): R = I + sinc1(t) W + sinc2(t) W^2, p = (I + sinc2(t) W + sinc3(t) W^2) v, t = |w|, the sinc helpers of
// ops/sinc.py with their Taylor branch below 0.01.  fp64 throughout; every index is a compile-time constant (no private arrays).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void feed_se3_exp(const double w[3], const double v[3], double R[3][3], double p[3])
{
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], t = sqrt(t2);
    double s1, s2, s3;
    if (t < 0.01) {                                  // ops/sinc.py:14, :100, :129
        s1 = 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42));
        s2 = 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56)));
        s3 = 1.0 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72)));
    } else {
        s1 = sin(t) / t;
        s2 = (1 - cos(t)) / t2;
        s3 = (t - sin(t)) / (t2 * t);
    }
    const double W[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    double S[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) S[i][j] = W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j];
    for (int i = 0; i < 3; i++) {
        p[i] = 0;
        for (int j = 0; j < 3; j++) {
            R[i][j] = (i == j ? 1.0 : 0.0) + s1 * W[i][j] + s2 * S[i][j];
            p[i] += ((i == j ? 1.0 : 0.0) + s2 * W[i][j] + s3 * S[i][j]) * v[j];
        }
    }
}
