// registration.hip -- what lies BETWEEN two PointNet passes of the iterative registration models (models/pointnetlk.py:44-120,
// models/pcrnet.py:29-70), on the device, so that a whole forward is a fixed list of launches with no host read in it:
//
//   l3d_reg_pose_first_layer  cloud [B,N,3], transforms [B,T,4,4] (or the 6 finite-difference twists exp(-dt_k e_k) made in place)
//                             -> q = R p + t formed in fp32 in the reference's order (se3.transform, ops/se3.py:112-122), then
//                             y = act(scale W1 q + shift) as [B T, C1, N] -- the layout mlp.hip's kernels read; the posed cloud is
//                             written only when asked for.  The 6 perturbed templates / the per-iteration source never exist.
//   l3d_reg_jac_pinv          f0 [B,K], f [B,6,K], dt [6] -> J = (f0 - f) / dt, H = J^T J (21 sums over K in fp64), H^-1 by
//                             Gauss-Jordan with partial pivoting in fp64, pinv = H^-1 J^T as fp32 [B,6,K]  (approx_Jic +
//                             compute_inverse_jacobian, models/pointnetlk.py:109-152).  An exactly zero pivot sets singular[1 + b]
//                             and singular[0] instead of raising.
//   l3d_reg_iclk_step         one iteration of models/pointnetlk.py:70-88: r = f - f0, dx = -pinv r, the batch maximum of |dx|,
//                             and est_T <- exp(dx) est_T unless that maximum is below xtol.  The reference's `break` is a device
//                             word: once it is set every later launch only copies est_T into its slot of est_T_series.
//   l3d_reg_quat_update       iPCRNet's pose update (models/pcrnet.py:33-50): the head's 7-vector -> normalised quaternion,
//                             est_R <- R_q est_R, est_t <- R_q est_t + t_q, est_T.
#include "common.h"
#include "se3_exp.h"
#include "../../include/l3d_registration.h"

#define REG_THREADS 256

// ---------------------------------------------------------------------------------------------
// pose + first layer
// ---------------------------------------------------------------------------------------------
#define REG_CG 16            // output channels per workgroup (gridDim.z = C1 / REG_CG)

__global__ __launch_bounds__(REG_THREADS) void reg_pose_l1_kernel(const float *__restrict__ cloud, const float *__restrict__ T,
                                                                  const float *__restrict__ dt, int Tn, int N, int C1,
                                                                  const float *__restrict__ w1, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, int relu, float *__restrict__ y,
                                                                  float *__restrict__ posed)
{
    __shared__ float sT[12];
    const int bt = blockIdx.y, b = bt / Tn, k = bt - b * Tn;
    if (dt) {                                            // transform k of the Jacobian pass: exp(-dt[k] e_k)  (pointnetlk.py:122-126)
        if (threadIdx.x == 0) {
            const double d = -(double)dt[k];
            const double w[3] = {k == 0 ? d : 0.0, k == 1 ? d : 0.0, k == 2 ? d : 0.0};
            const double v[3] = {k == 3 ? d : 0.0, k == 4 ? d : 0.0, k == 5 ? d : 0.0};
            double R[3][3], p[3];
            feed_se3_exp(w, v, R, p);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) sT[i * 4 + j] = (float)R[i][j];
                sT[i * 4 + 3] = (float)p[i];
            }
        }
    } else if (threadIdx.x < 12) {
        sT[threadIdx.x] = T[(size_t)bt * 16 + threadIdx.x];
    }
    __syncthreads();
    const int n = blockIdx.x * REG_THREADS + threadIdx.x;
    if (n >= N) return;
    const float *q = cloud + ((size_t)b * N + n) * 3;
    const float x = q[0], yy = q[1], z = q[2];
    const float px = ((sT[0] * x + sT[1] * yy) + sT[2] * z) + sT[3];
    const float py = ((sT[4] * x + sT[5] * yy) + sT[6] * z) + sT[7];
    const float pz = ((sT[8] * x + sT[9] * yy) + sT[10] * z) + sT[11];
    if (posed && blockIdx.z == 0) {
        float *o = posed + ((size_t)bt * N + n) * 3;
        o[0] = px; o[1] = py; o[2] = pz;
    }
    if (!y) return;
    const int c0 = blockIdx.z * REG_CG;
#pragma unroll
    for (int c = 0; c < REG_CG; c++) {
        const int co = c0 + c;
        float a = (w1[co * 3] * px + w1[co * 3 + 1] * py) + w1[co * 3 + 2] * pz;
        if (scale) a *= scale[co];
        if (shift) a += shift[co];
        if (relu) a = fmaxf(a, 0.f);
        y[((size_t)bt * C1 + co) * N + n] = a;
    }
}

extern "C" int l3d_reg_pose_first_layer(const float *cloud, const float *T, const float *dt, int B, int Tn, int N, const float *w1,
                                        const float *scale, const float *shift, int C1, int relu, float *y, float *posed,
                                        l3d_stream_t stream)
{
    L3D_REQUIRE(cloud && B > 0 && Tn > 0 && N > 0 && (y || posed));
    L3D_REQUIRE((T != nullptr) != (dt != nullptr));                   // the transforms come from exactly one of the two
    L3D_REQUIRE(!y || (w1 && C1 > 0));
    if (dt && Tn != 6) return L3D_ERR_UNSUPPORTED;
    if ((long)B * Tn > 65535) return L3D_ERR_UNSUPPORTED;
    if (y && (C1 % REG_CG || C1 > 1024)) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(reg_pose_l1_kernel, dim3(l3d_divup(N, REG_THREADS), B * Tn, y ? C1 / REG_CG : 1), dim3(REG_THREADS), 0,
                       (hipStream_t)stream, cloud, T, dt, Tn, N, C1, w1, scale, shift, relu, y, posed);
    return l3d_check_launch();
}

// ---------------------------------------------------------------------------------------------
// Jacobian -> pseudo-inverse, one workgroup per cloud.  The 6 x 12 augmented matrix [H | I] lives in LDS; thread (r, c) of the
// first 72 owns one element, so no thread indexes a private array.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REG_THREADS) void reg_jac_pinv_kernel(const float *__restrict__ f0, const float *__restrict__ f,
                                                                   const float *__restrict__ dt, int K, float *__restrict__ pinv,
                                                                   int *singular)
{
    __shared__ double sH[REG_THREADS / 64][21];
    __shared__ double sA[6][12];
    __shared__ int sPiv, sSing;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *f0b = f0 + (size_t)b * K, *fb = f + (size_t)b * 6 * K;
    double rdt[6];
#pragma unroll
    for (int k = 0; k < 6; k++) rdt[k] = (double)dt[k];

    double h[21];
#pragma unroll
    for (int i = 0; i < 21; i++) h[i] = 0.0;
    for (int c = tid; c < K; c += REG_THREADS) {
        const double a = (double)f0b[c];
        double j[6];
#pragma unroll
        for (int k = 0; k < 6; k++) j[k] = (a - (double)fb[(size_t)k * K + c]) / rdt[k];
        int i = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++) h[i++] += j[p] * j[q];
    }
#pragma unroll
    for (int i = 0; i < 21; i++) {
        const double s = l3d_wave_sum(h[i]);
        if ((tid & 63) == 0) sH[tid >> 6][i] = s;
    }
    if (tid == 0) sSing = 0;
    __syncthreads();
    const int r = tid / 12, c = tid - r * 12;            // element (r, c) of [H | I] for tid < 72
    if (tid < 72) {
        double v;
        if (c < 6) {
            const int p = r < c ? r : c, q = r < c ? c : r;
            const int i = p * 6 - p * (p - 1) / 2 + (q - p);           // index of (p, q), p <= q, in the packed upper triangle
            v = ((sH[0][i] + sH[1][i]) + sH[2][i]) + sH[3][i];
        } else {
            v = (c - 6 == r) ? 1.0 : 0.0;
        }
        sA[r][c] = v;
    }
    __syncthreads();
    for (int p = 0; p < 6; p++) {
        if (tid == 0) {                                  // partial pivoting: the largest |a[i][p]|, i >= p (first one on ties)
            int best = p;
            double bv = fabs(sA[p][p]);
            for (int i = p + 1; i < 6; i++) {
                const double a = fabs(sA[i][p]);
                if (a > bv) { bv = a; best = i; }
            }
            sPiv = best;
            if (!(bv > 0.0) && !(bv != bv)) sSing = 1;   // exactly zero: H is singular (a NaN column is left to propagate)
        }
        __syncthreads();
        const int piv = sPiv;
        double up = 0.0, lo = 0.0, pv = 1.0;
        if (tid < 12) { up = sA[p][tid]; lo = sA[piv][tid]; pv = sA[piv][p]; }
        __syncthreads();
        if (tid < 12) {                                  // swap rows p and piv, the pivot row normalised on the way
            if (piv != p) sA[piv][tid] = up;
            sA[p][tid] = lo / pv;
        }
        __syncthreads();
        double fac = 0.0, prow = 0.0, cur = 0.0;
        if (tid < 72 && r != p) { fac = sA[r][p]; prow = sA[p][c]; cur = sA[r][c]; }
        __syncthreads();
        if (tid < 72 && r != p) sA[r][c] = cur - fac * prow;
        __syncthreads();
    }
    const int sing = sSing;
    if (tid == 0) {
        singular[1 + b] = sing;
        if (sing) atomicOr(&singular[0], 1);
    }
    double hi[6][6];
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int q = 0; q < 6; q++) hi[p][q] = sA[p][6 + q];
    for (int cc = tid; cc < K; cc += REG_THREADS) {
        const double a = (double)f0b[cc];
        double j[6];
#pragma unroll
        for (int k = 0; k < 6; k++) j[k] = (a - (double)fb[(size_t)k * K + cc]) / rdt[k];
#pragma unroll
        for (int p = 0; p < 6; p++) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) s += hi[p][q] * j[q];
            pinv[((size_t)b * 6 + p) * K + cc] = sing ? 0.f : (float)s;
        }
    }
}

extern "C" int l3d_reg_jac_pinv(const float *f0, const float *f, const float *dt, int B, int K, float *pinv, int32_t *singular,
                                l3d_stream_t stream)
{
    L3D_REQUIRE(f0 && f && dt && pinv && singular && B > 0 && K > 0);
    if (B > 65535 || K > (1 << 20)) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(reg_jac_pinv_kernel, dim3(B), dim3(REG_THREADS), 0, (hipStream_t)stream, f0, f, dt, K, pinv, singular);
    return l3d_check_launch();
}

// ---------------------------------------------------------------------------------------------
// ICLK step.  state = {done, itr, stopped at itr 0, ticket}; ws [B][8] = {dx[6], |dx|, -}.
// One workgroup per cloud forms dx; the workgroup that draws the last ticket takes the batch maximum and updates every cloud's
// est_T.  The hand-off is release/acquire at agent scope: the producers' ws stores are released before the ticket add, the last
// arriver acquires before it reads them, and it reads them with agent-scope atomic loads (never through the scalar cache).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void reg_compose(const float dx[6], const float E[12], float out[12])
{
    const double w[3] = {dx[0], dx[1], dx[2]}, v[3] = {dx[3], dx[4], dx[5]};
    double R[3][3], p[3];
    feed_se3_exp(w, v, R, p);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = (R[i][0] * (double)E[j] + R[i][1] * (double)E[4 + j]) + R[i][2] * (double)E[8 + j];
            if (j == 3) s += p[i];
            out[i * 4 + j] = (float)s;
        }
    }
}

__global__ __launch_bounds__(REG_THREADS) void reg_iclk_step_kernel(const float *__restrict__ f, const float *__restrict__ f0,
                                                                    const float *__restrict__ pinv, int B, int K, int step,
                                                                    float xtol, const int *__restrict__ singular, float *ws,
                                                                    int *state, float *est_T, float *__restrict__ series,
                                                                    float *__restrict__ r)
{
    __shared__ double sAcc[REG_THREADS / 64][6];
    __shared__ float sMax[REG_THREADS / 64];
    __shared__ int sNan[REG_THREADS / 64];
    __shared__ int sLast;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool first = step == 0;
    if (singular[0]) return;                             // the reference's early return: est_T, r and est_T_series stay as they are
    float *slot = series + (size_t)(step + 1) * B * 16;
    if (!first && state[0]) {                            // after the `break`: models/pointnetlk.py:90-91 fills the tail with est_T
        if (tid < 16) slot[b * 16 + tid] = est_T[b * 16 + tid];
        return;
    }
    double acc[6];
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = 0.0;
    for (int c = tid; c < K; c += REG_THREADS) {
        const float rv = f[(size_t)b * K + c] - f0[(size_t)b * K + c];
        r[(size_t)b * K + c] = rv;
#pragma unroll
        for (int k = 0; k < 6; k++) acc[k] += (double)pinv[((size_t)b * 6 + k) * K + c] * (double)rv;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double s = l3d_wave_sum(acc[k]);
        if ((tid & 63) == 0) sAcc[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float n2 = 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const float d = (float)(-(((sAcc[0][k] + sAcc[1][k]) + sAcc[2][k]) + sAcc[3][k]));
            __hip_atomic_store(&ws[b * 8 + k], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            n2 += d * d;
        }
        __hip_atomic_store(&ws[b * 8 + 6], sqrtf(n2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int ticket = __hip_atomic_fetch_add(&state[3], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == B - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        sLast = last;
    }
    __syncthreads();
    if (!sLast) return;

    // ---- the last arriver: batch maximum (NaN propagates, as torch.max does), then the update of every cloud
    float m = 0.f;
    int nan = 0;
    for (int i = tid; i < B; i += REG_THREADS) {
        const float v = __hip_atomic_load(&ws[i * 8 + 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nan |= (v != v);
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmaxf(m, __shfl_xor(m, o, 64));
        nan |= __shfl_xor(nan, o, 64);
    }
    if ((tid & 63) == 0) { sMax[tid >> 6] = m; sNan[tid >> 6] = nan; }
    __syncthreads();
    m = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
    nan = sNan[0] | sNan[1] | sNan[2] | sNan[3];
    const bool stop = !nan && m < xtol;                  // `float(check) < self.xtol` (pointnetlk.py:84): False for a NaN
    for (int i = tid; i < B; i += REG_THREADS) {
        float E[12], out[12];
#pragma unroll
        for (int e = 0; e < 12; e++) E[e] = first ? ((e == 0 || e == 5 || e == 10) ? 1.f : 0.f) : est_T[i * 16 + e];
        if (stop) {
#pragma unroll
            for (int e = 0; e < 12; e++) out[e] = E[e];
        } else {
            float dx[6];
#pragma unroll
            for (int k = 0; k < 6; k++) dx[k] = __hip_atomic_load(&ws[i * 8 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            reg_compose(dx, E, out);
        }
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float id = (e == 0 || e == 5 || e == 10 || e == 15) ? 1.f : 0.f;
            float v = id;                                // the last row: 0 0 0 1
#pragma unroll
            for (int q = 0; q < 12; q++) v = (q == e) ? out[q] : v;
            est_T[i * 16 + e] = v;
            slot[i * 16 + e] = v;
            if (first) series[i * 16 + e] = id;
        }
    }
    if (tid == 0) {
        state[0] = stop ? 1 : 0;
        state[1] = step + 1;
        if (first) state[2] = stop ? 1 : 0;
        __hip_atomic_store(&state[3], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

extern "C" int l3d_reg_iclk_step(const float *f, const float *f0, const float *pinv, int B, int K, int step, int maxiter, float xtol,
                                 const int32_t *singular, float *ws, int32_t *state, float *est_T, float *series, float *r,
                                 l3d_stream_t stream)
{
    L3D_REQUIRE(f && f0 && pinv && singular && ws && state && est_T && series && r && B > 0 && K > 0);
    L3D_REQUIRE(maxiter > 0 && step >= 0 && step < maxiter);
    if (B > 65535 || K > (1 << 20)) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(reg_iclk_step_kernel, dim3(B), dim3(REG_THREADS), 0, (hipStream_t)stream, f, f0, pinv, B, K, step, xtol,
                       singular, ws, state, est_T, series, r);
    return l3d_check_launch();
}

// ---------------------------------------------------------------------------------------------
// iPCRNet's pose update, one thread per cloud.  pose7 = (quaternion w x y z, translation) as the head emits it;
// q = pose7[:4] / max(|pose7[:4]|, 1e-12) (create_pose_7d), R_q from qrot(q, e_i) = e_i + 2 (q_w (u x e_i) + u x (u x e_i)),
// u = q_xyz (ops/quaternion.py:35-53).  `first` != 0: est_R = I, est_t = 0 are taken as the incoming pose (nothing is read).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REG_THREADS) void reg_quat_update_kernel(const float *__restrict__ pose7, int B, int first,
                                                                      float *est_R, float *est_t, float *__restrict__ est_T)
{
    const int b = blockIdx.x * REG_THREADS + threadIdx.x;
    if (b >= B) return;
    const float *ps = pose7 + (size_t)b * 7;
    const double q0 = ps[0], q1 = ps[1], q2 = ps[2], q3 = ps[3];
    const double nrm = fmax(sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3), 1e-12);
    const double qw = q0 / nrm, u[3] = {q1 / nrm, q2 / nrm, q3 / nrm};
    double Rq[3][3];                                     // column i = qrot(q, e_i)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double e[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
        const double uv[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
        const double uuv[3] = {u[1] * uv[2] - u[2] * uv[1], u[2] * uv[0] - u[0] * uv[2], u[0] * uv[1] - u[1] * uv[0]};
#pragma unroll
        for (int j = 0; j < 3; j++) Rq[j][i] = e[j] + 2.0 * (qw * uv[j] + uuv[j]);
    }
    double Re[3][3], te[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Re[i][j] = first ? (i == j ? 1.0 : 0.0) : (double)est_R[b * 9 + i * 3 + j];
        te[i] = first ? 0.0 : (double)est_t[b * 3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float row[4];
#pragma unroll
        for (int j = 0; j < 3; j++) row[j] = (float)((Rq[i][0] * Re[0][j] + Rq[i][1] * Re[1][j]) + Rq[i][2] * Re[2][j]);
        row[3] = (float)(((Rq[i][0] * te[0] + Rq[i][1] * te[1]) + Rq[i][2] * te[2]) + (double)ps[4 + i]);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            est_R[b * 9 + i * 3 + j] = row[j];
            est_T[b * 16 + i * 4 + j] = row[j];
        }
        est_t[b * 3 + i] = row[3];
        est_T[b * 16 + i * 4 + 3] = row[3];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) est_T[b * 16 + 12 + j] = j == 3 ? 1.f : 0.f;
}

extern "C" int l3d_reg_quat_update(const float *pose7, int B, int first, float *est_R, float *est_t, float *est_T,
                                   l3d_stream_t stream)
{
    L3D_REQUIRE(pose7 && est_R && est_t && est_T && B > 0);
    if (B > (1 << 24)) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(reg_quat_update_kernel, dim3(l3d_divup(B, REG_THREADS)), dim3(REG_THREADS), 0, (hipStream_t)stream, pose7, B,
                       first, est_R, est_t, est_T);
    return l3d_check_launch();
}
