// 3D (Breaking-Bad) tail of the path: the two pose heads of Eff_GAT_3d
// (efficient_gat_3d.py:207-219: mlp_t / mlp_r second Linear, matrix_exp(vec2skew(r)),
// matrix_to_quaternion, L2 normalise) and the SE(3) DDIM update
// (spatial_diffusion_3d_test_double_diffusion.py:595-685 with so3_scale / log_rmat of
// utils_3d.py:1018-1061).  A few dozen flops per piece: one thread per piece, fp32.
// Training side: the pose head's backward (k_head3d_bwd) and the SE(3) noising of p_losses (k_q_sample_se3).
// use_6dof (13-wide pose rows: quaternion | translation | a1 | a2): the same kernels at T_CH = 9, and the Gram-Schmidt quaternion of
// (a1, a2) that the loss and the evaluation read, with its backward (k_rot6d_to_pose, k_rot6d_to_pose_bwd).
//
// matrix_exp of a skew matrix is evaluated in closed form (Rodrigues); torch.matrix_exp uses
// a scaled Taylor/Pade series -- equal to ~1e-7.  log_rmat's NaN branch (rotation by exactly
// pi, where the reference falls back to torch.linalg.eigh) takes the axis from (R + I)/2
// instead; the two agree up to the sign of the axis, which is undetermined at pi.
#include "da_common.h"
#include "da_internal.h"

namespace da {

struct M3 { float m[9]; };

__device__ inline M3 rodrigues(float v0, float v1, float v2) {   // exp(vec2skew(v))
    const float th2 = v0 * v0 + v1 * v1 + v2 * v2;
    const float th = sqrtf(th2);
    float a, b;
    if (th < 1e-4f) {
        a = 1.0f - th2 * (1.0f / 6.0f);
        b = 0.5f - th2 * (1.0f / 24.0f);
    } else {
        a = sinf(th) / th;
        const float h = sinf(0.5f * th) / (0.5f * th);
        b = 0.5f * h * h;
    }
    M3 r;
    // I + a*S + b*(v v^T - th2 I), S = [[0,-v2,v1],[v2,0,-v0],[-v1,v0,0]]
    r.m[0] = 1.0f + b * (v0 * v0 - th2); r.m[1] = -a * v2 + b * v0 * v1;     r.m[2] = a * v1 + b * v0 * v2;
    r.m[3] = a * v2 + b * v0 * v1;       r.m[4] = 1.0f + b * (v1 * v1 - th2); r.m[5] = -a * v0 + b * v1 * v2;
    r.m[6] = -a * v1 + b * v0 * v2;      r.m[7] = a * v0 + b * v1 * v2;      r.m[8] = 1.0f + b * (v2 * v2 - th2);
    return r;
}

__device__ inline void mat_to_quat(const M3 &R, float q[4]) {    // pytorch3d matrix_to_quaternion
    const float m00 = R.m[0], m01 = R.m[1], m02 = R.m[2], m10 = R.m[3], m11 = R.m[4], m12 = R.m[5],
                m20 = R.m[6], m21 = R.m[7], m22 = R.m[8];
    float qa[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    int best = 0;
    for (int i = 0; i < 4; ++i) qa[i] = qa[i] > 0.f ? sqrtf(qa[i]) : 0.f;
    for (int i = 1; i < 4; ++i) if (qa[i] > qa[best]) best = i;      // argmax: first maximum
    float c[4];
    if (best == 0) { c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; }
    else if (best == 1) { c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20; }
    else if (best == 2) { c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21; }
    else { c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3]; }
    const float den = 2.0f * fmaxf(qa[best], 0.1f);
    const float sgn = (c[0] / den) < 0.f ? -1.f : 1.f;              // standardize_quaternion
    for (int i = 0; i < 4; ++i) q[i] = sgn * (c[i] / den);
}

__device__ inline M3 quat_to_mat(const float q[4]) {             // pytorch3d quaternion_to_matrix
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
    M3 o;
    o.m[0] = 1 - two_s * (j * j + k * k); o.m[1] = two_s * (i * j - k * r);     o.m[2] = two_s * (i * k + j * r);
    o.m[3] = two_s * (i * j + k * r);     o.m[4] = 1 - two_s * (i * i + k * k); o.m[5] = two_s * (j * k - i * r);
    o.m[6] = two_s * (i * k - j * r);     o.m[7] = two_s * (j * k + i * r);     o.m[8] = 1 - two_s * (i * i + j * j);
    return o;
}

__device__ inline M3 so3_scale(const M3 &R, float sc) {          // matrix_exp(sc * log_rmat(R))
    // log_rmat, utils_3d.py:1018-1046
    const float k0 = R.m[7] - R.m[5];      // skew[2,1]
    const float k1 = -(R.m[6] - R.m[2]);   // -skew[2,0]
    const float k2 = R.m[3] - R.m[1];      // skew[1,0]
    const float s_angle = sqrtf(k0 * k0 + k1 * k1 + k2 * k2) * 0.5f;
    const float c_angle = (R.m[0] + R.m[4] + R.m[8] - 1.0f) * 0.5f;
    const float angle = atan2f(s_angle, c_angle);
    float w0, w1, w2;
    if (angle == 0.0f) {
        w0 = w1 = w2 = 0.f;
    } else if (s_angle == 0.0f) {          // rotation by pi: axis from (R + I) / 2
        float d0 = (R.m[0] + 1.f) * 0.5f, d1 = (R.m[4] + 1.f) * 0.5f, d2 = (R.m[8] + 1.f) * 0.5f;
        float a0, a1, a2;
        if (d0 >= d1 && d0 >= d2) { a0 = sqrtf(fmaxf(d0, 0.f)); a1 = (R.m[1] + R.m[3]) * 0.25f / a0; a2 = (R.m[2] + R.m[6]) * 0.25f / a0; }
        else if (d1 >= d2) { a1 = sqrtf(fmaxf(d1, 0.f)); a0 = (R.m[1] + R.m[3]) * 0.25f / a1; a2 = (R.m[5] + R.m[7]) * 0.25f / a1; }
        else { a2 = sqrtf(fmaxf(d2, 0.f)); a0 = (R.m[2] + R.m[6]) * 0.25f / a2; a1 = (R.m[5] + R.m[7]) * 0.25f / a2; }
        w0 = angle * a0; w1 = angle * a1; w2 = angle * a2;
    } else {
        const float scale = angle / (2.0f * s_angle);
        w0 = scale * k0; w1 = scale * k1; w2 = scale * k2;     // skew2vec(scale * skew)
    }
    return rodrigues(sc * w0, sc * w1, sc * w2);
}

__device__ inline M3 matmul(const M3 &A, const M3 &B) {
    M3 C;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C.m[i * 3 + j] = A.m[i * 3] * B.m[j] + A.m[i * 3 + 1] * B.m[3 + j] + A.m[i * 3 + 2] * B.m[6 + j];
    return C;
}
__device__ inline M3 transpose(const M3 &A) {
    M3 C;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C.m[i * 3 + j] = A.m[j * 3 + i];
    return C;
}

// One wave per piece: T_CH + 3 dot products of length 256 (mlp_t.2 / mlp_r.2), then lane 0 finishes.  T_CH = 3: the translation;
// T_CH = 9 (use_6dof): translation | a1 | a2, the two 3-vectors the loss and the evaluation orthonormalise (k_rot6d_to_pose).
// Rows of out are 4 + T_CH wide, rows of pre 3 + T_CH = [r | t].
template <typename T, int T_CH>
__global__ __launch_bounds__(256) void k_head3d(int n, const T *__restrict__ hh, const float *__restrict__ wt,
                                                const float *__restrict__ bt, const float *__restrict__ wr,
                                                const float *__restrict__ br, float *__restrict__ out7,
                                                float *__restrict__ pre) {
    const int lane = threadIdx.x & 63;
    const int r = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (r >= n) return;
    float acc[T_CH + 3];
#pragma unroll
    for (int c = 0; c < T_CH + 3; ++c) acc[c] = 0.f;
    const T *ht = hh + (size_t)r * 512, *hr = ht + 256;
    for (int k = lane; k < 256; k += 64) {
        const float a = ldf(ht + k), b = ldf(hr + k);
#pragma unroll
        for (int c = 0; c < 3; ++c) { acc[c] = fmaf(wt[c * 256 + k], a, acc[c]); acc[T_CH + c] = fmaf(wr[c * 256 + k], b, acc[T_CH + c]); }
#pragma unroll
        for (int c = 3; c < T_CH; ++c) acc[c] = fmaf(wt[c * 256 + k], a, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < T_CH + 3; ++c)
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
    if (lane != 0) return;
    float tv[T_CH];
#pragma unroll
    for (int c = 0; c < T_CH; ++c) tv[c] = acc[c] + bt[c];
    const float r0 = acc[T_CH] + br[0], r1 = acc[T_CH + 1] + br[1], r2 = acc[T_CH + 2] + br[2];
    if (pre) {
        float *p = pre + (size_t)r * (3 + T_CH);
        p[0] = r0; p[1] = r1; p[2] = r2;
#pragma unroll
        for (int c = 0; c < T_CH; ++c) p[3 + c] = tv[c];
    }
    float q[4];
    mat_to_quat(rodrigues(r0, r1, r2), q);
    const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);  // F.normalize eps
    float *o = out7 + (size_t)r * (4 + T_CH);
    o[0] = q[0] / nrm; o[1] = q[1] / nrm; o[2] = q[2] / nrm; o[3] = q[3] / nrm;
#pragma unroll
    for (int c = 0; c < T_CH; ++c) o[4 + c] = tv[c];
}

// Rows of 4 + T_CH: the Gaussian DDIM update on columns 4 .. 4 + T_CH, the SO(3) update on the quaternion in columns 0 .. 3.
template <int T_CH>
__global__ __launch_bounds__(64) void k_ddim3d(DeviceSchedule s, int mean_type, int n, const float *__restrict__ x,
                                               const float *__restrict__ mo, const int64_t *__restrict__ t,
                                               int64_t t_scalar, int ratio, int prev_all_nonneg,
                                               float *__restrict__ x_prev) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int64_t ti = t ? t[r] : t_scalar;
    ti = ti < 0 ? 0 : (ti >= s.steps ? s.steps - 1 : ti);
    const int64_t tp = ti - ratio;
    const float ap = s.alphas_cumprod[ti];
    const float ap_prev = (prev_all_nonneg && tp >= 0) ? s.alphas_cumprod[tp] : 1.0f;
    const float beta = 1.0f - ap;
    constexpr int W = 4 + T_CH;
    float xv[W], x0[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        xv[c] = x[(size_t)r * W + c];
        const float m = mo[(size_t)r * W + c];
        x0[c] = mean_type == DA_MEAN_START_X ? m : (xv[c] - sqrtf(beta) * m) / sqrtf(ap);
    }
    const float sr = s.sqrt_recip_alphas_cumprod[ti], srm1 = s.sqrt_recipm1_alphas_cumprod[ti];
    const float sq_prev = sqrtf(ap_prev), sq_dir = sqrtf(1.0f - ap_prev);
    float *o = x_prev + (size_t)r * W;
#pragma unroll
    for (int c = 4; c < W; ++c) {
        const float eps = (sr * xv[c] - x0[c]) / srm1;
        o[c] = sq_prev * x0[c] + sq_dir * eps;
    }
    const M3 Rx = quat_to_mat(xv), R0 = quat_to_mat(x0);
    const M3 xt_term = so3_scale(Rx, sr / srm1);
    const M3 x0_term = so3_scale(R0, 1.0f / srm1);
    float qe[4];
    mat_to_quat(matmul(xt_term, transpose(x0_term)), qe);
    const M3 dir = so3_scale(quat_to_mat(qe), sq_dir);
    float qp[4];
    mat_to_quat(matmul(so3_scale(R0, sq_prev), dir), qp);
    o[0] = qp[0]; o[1] = qp[1]; o[2] = qp[2]; o[3] = qp[3];
}

// Backward of the pose head (the tail of k_head3d): pre [n, 6] = [r | t] as the forward saved it, d_out [n, 7] the gradient of
// [q | t] -> d_pre [n, 6].  The translation passes through.  The rotation is q = normalize(matrix_to_quaternion(exp(skew(r)))):
// on the forward's branch q = s (cos(th/2), k r) with th = |r|, k = sin(th/2) / th and s = +-1 so that w >= 0
// (standardize_quaternion); |q| = 1, so F.normalize contributes the tangent projection g' = g - q <q, g> and
//   d r_j = s (-(k/2) r_j g'_w + k g'_j + m r_j <r, g'_v>),   m = (cos(th/2) / 2 - k) / th^2
// (k -> 1/2 - th^2/48, m -> -1/24 + th^2/960 below rodrigues' th < 1e-4 switch).  One thread per piece, fp32, no atomics.
// T_CH = 9 (use_6dof): pre [n, 12], d_out [n, 13], d_pre [n, 12]; all nine translation-head channels pass through.
template <int T_CH>
__global__ __launch_bounds__(64) void k_head3d_bwd(int n, const float *__restrict__ pre, const float *__restrict__ d_out,
                                                   float *__restrict__ d_pre) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int LP = 3 + T_CH;
    const float r0 = pre[(size_t)i * LP], r1 = pre[(size_t)i * LP + 1], r2 = pre[(size_t)i * LP + 2];
    const float *g = d_out + (size_t)i * (4 + T_CH);
    const float th2 = r0 * r0 + r1 * r1 + r2 * r2, th = sqrtf(th2);
    float c, k, m;
    if (th < 1e-4f) {
        c = 1.0f - th2 * 0.125f;
        k = 0.5f - th2 * (1.0f / 48.0f);
        m = -1.0f / 24.0f + th2 * (1.0f / 960.0f);
    } else {
        c = cosf(0.5f * th);
        k = sinf(0.5f * th) / th;
        m = (0.5f * c - k) / th2;
    }
    const float s = c < 0.f ? -1.f : 1.f;
    const float qw = s * c, q1 = s * k * r0, q2 = s * k * r1, q3 = s * k * r2;
    const float dot = qw * g[0] + q1 * g[1] + q2 * g[2] + q3 * g[3];
    const float gw = g[0] - qw * dot, g1 = g[1] - q1 * dot, g2 = g[2] - q2 * dot, g3 = g[3] - q3 * dot;
    const float rg = r0 * g1 + r1 * g2 + r2 * g3;
    const float a = m * rg - 0.5f * k * gw;                 // coefficient of r_j
    float *o = d_pre + (size_t)i * LP;
    o[0] = s * (k * g1 + a * r0);
    o[1] = s * (k * g2 + a * r1);
    o[2] = s * (k * g3 + a * r2);
#pragma unroll
    for (int c = 0; c < T_CH; ++c) o[3 + c] = g[4 + c];
}

// SE(3) noising of p_losses (spatial_diffusion_3d_test_double_diffusion.py:421-441) as one launch, one thread per piece:
// translation = q_sample; rotation = so3_scale(R0, sqrt_alphas_cumprod[t]) @ noise, noise an IGSO(3) draw by inverse-transform
// sampling on the piece's CDF row trap[t] (IsotropicGaussianSO3.sample, distributions.py:507-526): idx_1 = #{trap[t] <= u}
// (the row is non-decreasing: a binary search), idx_0 = max(idx_1 - 1, 0), angle = lerp of the two sample locations
// pi linspace(0, 1, 1000)[1:]^3 with the clamped weight (u - trap_start) / max(trap_end - trap_start, 1e-6).
// The reference gathers trap_start / trap_end with an index of shape [P, 1] along dim 0 of its [999, P] table, i.e. from the
// FIRST piece's column whatever the piece (distributions.py:516-517); the weights here come from row t[0] for the same reason.
// idx_1 can reach 999 for u = 1 (the reference's gather would raise): clamped to 998.
constexpr int IGSO3_ROW = 999;
__device__ __forceinline__ float igso3_loc(int k) {                // pi * linspace(0, 1, 1000)[k + 1]^3 (torch's two-sided linspace)
    const int j = k + 1;
    const float step = 1.0f / 999.0f;
    const float x = j < 500 ? step * (float)j : 1.0f - step * (float)(999 - j);
    return 3.14159265358979323846f * (x * x * x);
}
// SIXD (use_6dof, :424-431): x_start stays 7 wide; the Gaussian part is nine wide, [t | R0[:, 0] | R0[:, 1]] with R0 = quat_to_mat(x_start)
// (its first two COLUMNS), noise_tr is [n, 9] and the rows written are 13 wide.  The rotation half is the same.
template <bool SIXD>
__global__ __launch_bounds__(64) void k_q_sample_se3(int steps, int n, const float *__restrict__ sac, const float *__restrict__ somac,
                                                     const float *__restrict__ trap, const float *__restrict__ x_start,
                                                     const int64_t *__restrict__ t, const float *__restrict__ noise_tr,
                                                     const float *__restrict__ axes, const float *__restrict__ unif,
                                                     float *__restrict__ x_noisy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto clampt = [&](int64_t v) { return v < 0 ? (int64_t)0 : (v >= steps ? (int64_t)steps - 1 : v); };
    const int64_t ti = clampt(t[i]), t0 = clampt(t[0]);
    const float a = sac[ti], b = somac[ti];
    const float *xs = x_start + (size_t)i * 7;
    constexpr int T_CH = SIXD ? 9 : 3;
    float *o = x_noisy + (size_t)i * (4 + T_CH);
    const float *nz = noise_tr + (size_t)i * T_CH;
    for (int c = 0; c < 3; ++c) o[4 + c] = __fadd_rn(__fmul_rn(a, xs[4 + c]), __fmul_rn(b, nz[c]));      // k_q_sample's expression
    if constexpr (SIXD) {
        const M3 R0 = quat_to_mat(xs);
#pragma unroll
        for (int c = 0; c < 3; ++c) {                              // columns 0 and 1 of R0
            o[7 + c] = __fadd_rn(__fmul_rn(a, R0.m[3 * c]), __fmul_rn(b, nz[3 + c]));
            o[10 + c] = __fadd_rn(__fmul_rn(a, R0.m[3 * c + 1]), __fmul_rn(b, nz[6 + c]));
        }
    }
    const float *row = trap + (size_t)ti * IGSO3_ROW, *row0 = trap + (size_t)t0 * IGSO3_ROW;
    const float u = unif[i];
    int lo = 0, hi = IGSO3_ROW;                                    // first index with row[k] > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] <= u) lo = mid + 1; else hi = mid;
    }
    const int idx1 = lo > IGSO3_ROW - 1 ? IGSO3_ROW - 1 : lo, idx0 = idx1 > 0 ? idx1 - 1 : 0;
    const float ts = row0[idx0], te = row0[idx1];
    const float diff = fmaxf(te - ts, 1e-6f);
    const float wgt = fminf(fmaxf((u - ts) / diff, 0.f), 1.f);
    const float a0 = igso3_loc(idx0), a1 = igso3_loc(idx1);
    const float ang = wgt < 0.5f ? a0 + wgt * (a1 - a0) : a1 - (a1 - a0) * (1.0f - wgt);      // torch.lerp
    const float v0 = axes[(size_t)i * 3], v1 = axes[(size_t)i * 3 + 1], v2 = axes[(size_t)i * 3 + 2];
    const float inv = ang / sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    const M3 noise = rodrigues(v0 * inv, v1 * inv, v2 * inv);      // aa_to_rmat(axis, angle)
    float q[4];
    mat_to_quat(matmul(so3_scale(quat_to_mat(xs), a), noise), q);
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
}

// use_6dof: the pose the loss and the evaluation read out of a 13-wide prediction (:480-490, :826-845): translation = columns 4:7,
// rotation = matrix_to_quaternion([b1 b2 b3]) with the Gram-Schmidt frame of a1 = columns 7:10, a2 = columns 10:13,
//   b1 = a1 / max(|a1|, 1e-12),  u = a2 - (a2.b1) b1,  b2 = u / max(|u|, 1e-12),  b3 = b1 x b2      (the b's are the COLUMNS)
// -> pose7 [n, 7] = [q | t].  One thread per piece, fp32, no atomics.
struct Frame6 { float b1[3], b2[3], b3[3], n1, n2, d; };
__device__ inline Frame6 gram_schmidt(const float *a1, const float *a2) {
    Frame6 f;
    f.n1 = fmaxf(sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12f);
    for (int c = 0; c < 3; ++c) f.b1[c] = a1[c] / f.n1;
    f.d = a2[0] * f.b1[0] + a2[1] * f.b1[1] + a2[2] * f.b1[2];
    float u[3];
    for (int c = 0; c < 3; ++c) u[c] = a2[c] - f.d * f.b1[c];
    f.n2 = fmaxf(sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12f);
    for (int c = 0; c < 3; ++c) f.b2[c] = u[c] / f.n2;
    f.b3[0] = f.b1[1] * f.b2[2] - f.b1[2] * f.b2[1];
    f.b3[1] = f.b1[2] * f.b2[0] - f.b1[0] * f.b2[2];
    f.b3[2] = f.b1[0] * f.b2[1] - f.b1[1] * f.b2[0];
    return f;
}
__device__ inline void frame_quat(const Frame6 &f, float q[4]) {
    M3 R;
    for (int c = 0; c < 3; ++c) { R.m[3 * c] = f.b1[c]; R.m[3 * c + 1] = f.b2[c]; R.m[3 * c + 2] = f.b3[c]; }
    mat_to_quat(R, q);
}
__global__ __launch_bounds__(64) void k_rot6d_to_pose(int n, const float *__restrict__ pred, int ld, float *__restrict__ pose7) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = pred + (size_t)i * ld;
    float a[6];
    for (int c = 0; c < 6; ++c) a[c] = p[7 + c];
    float q[4];
    frame_quat(gram_schmidt(a, a + 3), q);
    float *o = pose7 + (size_t)i * 7;
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
    o[4] = p[4]; o[5] = p[5]; o[6] = p[6];
}

// Its backward: d_pose7 [n, 7] = g -> d_pred [n, 13]; columns 0:4 (the head's own quaternion) get zeros, 4:7 pass through.
// The four branches of matrix_to_quaternion are one function on SO(3), and R = [b1 b2 b3] is a rotation whatever a1, a2 are, so only
// the differential along SO(3) matters and ONE form serves every branch.  For dR = [dw]x R the quaternion moves by
// dq = (0, dw) (x) q / 2; with q = (w, v) as the forward returns it (the w >= 0 sign s is inside q, and constant nearby)
//   m := dL/dw = (w g_v - g_w v + v x g_v) / 2.
// The frame turns by dw = (b3.db2) b1 - (b3.db1) b2 + (b2.db1) b3, and with n1 = |a1|, n2 = |u|, d = a2.b1
//   db1 = (I - b1 b1^T) da1 / n1,   b3.db2 = (b3.da2 - d b3.db1) / n2,
// so   d a2 = (m.b1) b3 / n2,   d a1 = ((m.b3) b2 - ((m.b2) + (m.b1) d / n2) b3) / n1.
// (Where a norm is below the 1e-12 clamp the frame is degenerate and the result is merely finite.)
__global__ __launch_bounds__(64) void k_rot6d_to_pose_bwd(int n, const float *__restrict__ pred, int ld, const float *__restrict__ d_pose7,
                                                          float *__restrict__ d_pred) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = pred + (size_t)i * ld, *g = d_pose7 + (size_t)i * 7;
    float a[6];
    for (int c = 0; c < 6; ++c) a[c] = p[7 + c];
    const Frame6 f = gram_schmidt(a, a + 3);
    float q[4];
    frame_quat(f, q);
    const float w = q[0], gw = g[0];
    const float m0 = 0.5f * (w * g[1] - gw * q[1] + (q[2] * g[3] - q[3] * g[2]));
    const float m1 = 0.5f * (w * g[2] - gw * q[2] + (q[3] * g[1] - q[1] * g[3]));
    const float m2 = 0.5f * (w * g[3] - gw * q[3] + (q[1] * g[2] - q[2] * g[1]));
    const float mb1 = m0 * f.b1[0] + m1 * f.b1[1] + m2 * f.b1[2];
    const float mb2 = m0 * f.b2[0] + m1 * f.b2[1] + m2 * f.b2[2];
    const float mb3 = m0 * f.b3[0] + m1 * f.b3[1] + m2 * f.b3[2];
    const float k2 = mb1 / f.n2, k3 = mb2 + k2 * f.d;
    float *o = d_pred + (size_t)i * 13;
    o[0] = o[1] = o[2] = o[3] = 0.f;
    o[4] = g[4]; o[5] = g[5]; o[6] = g[6];
    for (int c = 0; c < 3; ++c) {
        o[7 + c] = (mb3 * f.b2[c] - k3 * f.b3[c]) / f.n1;
        o[10 + c] = k2 * f.b3[c];
    }
}

int launch_head3d(int prec, int n, int t_ch, const void *hh, const float *wt, const float *bt, const float *wr, const float *br,
                  float *out7, float *pre_head, hipStream_t st) {
    if (n <= 0) return 0;
    if (t_ch != 3 && t_ch != 9) { set_error("launch_head3d: t_ch %d is neither 3 nor 9", t_ch); return 2; }
    const int grid = (int)(((size_t)n * 64 + 255) / 256);
    if (prec == DA_PREC_BF16) {
        if (t_ch == 9) k_head3d<bf16_t, 9><<<grid, 256, 0, st>>>(n, (const bf16_t *)hh, wt, bt, wr, br, out7, pre_head);
        else k_head3d<bf16_t, 3><<<grid, 256, 0, st>>>(n, (const bf16_t *)hh, wt, bt, wr, br, out7, pre_head);
    } else {
        if (t_ch == 9) k_head3d<float, 9><<<grid, 256, 0, st>>>(n, (const float *)hh, wt, bt, wr, br, out7, pre_head);
        else k_head3d<float, 3><<<grid, 256, 0, st>>>(n, (const float *)hh, wt, bt, wr, br, out7, pre_head);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

int launch_ddim3d(const DeviceSchedule &s, int mean_type, int n, int t_ch, const float *x, const float *mo, const int64_t *t,
                  int64_t t_scalar, int ratio, int prev_all_nonneg, float *x_prev, hipStream_t st) {
    if (n <= 0) return 0;
    if (t_ch != 3 && t_ch != 9) { set_error("launch_ddim3d: t_ch %d is neither 3 nor 9", t_ch); return 2; }
    if (t_ch == 9) k_ddim3d<9><<<(n + 63) / 64, 64, 0, st>>>(s, mean_type, n, x, mo, t, t_scalar, ratio, prev_all_nonneg, x_prev);
    else k_ddim3d<3><<<(n + 63) / 64, 64, 0, st>>>(s, mean_type, n, x, mo, t, t_scalar, ratio, prev_all_nonneg, x_prev);
    DA_LAUNCH_CHECK();
    return 0;
}

int launch_head3d_bwd(int n, int t_ch, const float *pre, const float *d_out, float *d_pre, hipStream_t st) {
    if (n <= 0) return 0;
    if (t_ch != 3 && t_ch != 9) { set_error("launch_head3d_bwd: t_ch %d is neither 3 nor 9", t_ch); return 2; }
    if (t_ch == 9) k_head3d_bwd<9><<<(n + 63) / 64, 64, 0, st>>>(n, pre, d_out, d_pre);
    else k_head3d_bwd<3><<<(n + 63) / 64, 64, 0, st>>>(n, pre, d_out, d_pre);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

using namespace da;

extern "C" {

int da_head3d_backward(int n, const float *pre, const float *d_out, float *d_pre, void *stream) {
    DA_REQUIRE(n >= 0, "da_head3d_backward: n < 0");
    DA_REQUIRE(pre && d_out && d_pre, "da_head3d_backward: null argument");
    return launch_head3d_bwd(n, 3, pre, d_out, d_pre, (hipStream_t)stream);
}

int da_head3d_backward_ex(int n, int t_channels, const float *pre, const float *d_out, float *d_pre, void *stream) {
    DA_REQUIRE(n >= 0, "da_head3d_backward_ex: n < 0");
    DA_REQUIRE(t_channels == 3 || t_channels == 9, "da_head3d_backward_ex: t_channels = %d is neither 3 nor 9 (use_6dof)", t_channels);
    DA_REQUIRE(pre && d_out && d_pre, "da_head3d_backward_ex: null argument");
    return launch_head3d_bwd(n, t_channels, pre, d_out, d_pre, (hipStream_t)stream);
}

int da_rot6d_to_pose(int n, const float *pred, int ld, float *pose7, void *stream) {
    DA_REQUIRE(n >= 0 && ld >= 13, "da_rot6d_to_pose: n >= 0 and ld >= 13 (got n = %d, ld = %d)", n, ld);
    DA_REQUIRE(pred && pose7, "da_rot6d_to_pose: null argument");
    if (n == 0) return 0;
    k_rot6d_to_pose<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(n, pred, ld, pose7);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_rot6d_to_pose_backward(int n, const float *pred, int ld, const float *d_pose7, float *d_pred, void *stream) {
    DA_REQUIRE(n >= 0 && ld >= 13, "da_rot6d_to_pose_backward: n >= 0 and ld >= 13 (got n = %d, ld = %d)", n, ld);
    DA_REQUIRE(pred && d_pose7 && d_pred, "da_rot6d_to_pose_backward: null argument");
    if (n == 0) return 0;
    k_rot6d_to_pose_bwd<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(n, pred, ld, d_pose7, d_pred);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_q_sample_se3(int steps, int n, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, const float *trap,
                    const float *x_start, const int64_t *t, const float *noise_tr, const float *axes, const float *unif, float *x_noisy,
                    void *stream) {
    DA_REQUIRE(steps > 0 && n >= 0, "da_q_sample_se3: steps must be positive and n >= 0");
    DA_REQUIRE(sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod && trap && x_start && t && noise_tr && axes && unif && x_noisy,
               "da_q_sample_se3: null argument");
    if (n == 0) return 0;
    k_q_sample_se3<false><<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(steps, n, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, trap, x_start, t,
                                                                         noise_tr, axes, unif, x_noisy);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_q_sample_se3_6d(int steps, int n, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, const float *trap,
                       const float *x_start, const int64_t *t, const float *noise_tr, const float *axes, const float *unif, float *x_noisy,
                       void *stream) {
    DA_REQUIRE(steps > 0 && n >= 0, "da_q_sample_se3_6d: steps must be positive and n >= 0");
    DA_REQUIRE(sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod && trap && x_start && t && noise_tr && axes && unif && x_noisy,
               "da_q_sample_se3_6d: null argument");
    if (n == 0) return 0;
    k_q_sample_se3<true><<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(steps, n, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, trap, x_start, t,
                                                                        noise_tr, axes, unif, x_noisy);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
