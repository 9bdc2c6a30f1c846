// 3D (Breaking-Bad) tail of the path: the two pose heads of Eff_GAT_3d
// (efficient_gat_3d.py:207-219: mlp_t / mlp_r second Linear, matrix_exp(vec2skew(r)),
// matrix_to_quaternion, L2 normalise) and the SE(3) DDIM update
// (spatial_diffusion_3d_test_double_diffusion.py:595-685 with so3_scale / log_rmat of
// utils_3d.py:1018-1061).  A few dozen flops per piece: one thread per piece, fp32.
// Training side: the pose head's backward (k_head3d_bwd) and the SE(3) noising of p_losses (k_q_sample_se3).
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

// One wave per piece: 6 dot products of length 256 (mlp_t.2 / mlp_r.2), then lane 0 finishes.
template <typename T>
__global__ __launch_bounds__(256) void k_head3d(int n, const T *__restrict__ hh, const float *__restrict__ wt,
                                                const float *__restrict__ bt, const float *__restrict__ wr,
                                                const float *__restrict__ br, float *__restrict__ out7,
                                                float *__restrict__ pre) {
    const int lane = threadIdx.x & 63;
    const int r = (int)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (r >= n) return;
    float acc[6] = {0, 0, 0, 0, 0, 0};
    const T *ht = hh + (size_t)r * 512, *hr = ht + 256;
    for (int k = lane; k < 256; k += 64) {
        const float a = ldf(ht + k), b = ldf(hr + k);
#pragma unroll
        for (int c = 0; c < 3; ++c) { acc[c] = fmaf(wt[c * 256 + k], a, acc[c]); acc[3 + c] = fmaf(wr[c * 256 + k], b, acc[3 + c]); }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c)
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
    if (lane != 0) return;
    const float t0 = acc[0] + bt[0], t1 = acc[1] + bt[1], t2 = acc[2] + bt[2];
    const float r0 = acc[3] + br[0], r1 = acc[4] + br[1], r2 = acc[5] + br[2];
    if (pre) { float *p = pre + (size_t)r * 6; p[0] = r0; p[1] = r1; p[2] = r2; p[3] = t0; p[4] = t1; p[5] = t2; }
    float q[4];
    mat_to_quat(rodrigues(r0, r1, r2), q);
    const float nrm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);  // F.normalize eps
    float *o = out7 + (size_t)r * 7;
    o[0] = q[0] / nrm; o[1] = q[1] / nrm; o[2] = q[2] / nrm; o[3] = q[3] / nrm;
    o[4] = t0; o[5] = t1; o[6] = t2;
}

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
    float xv[7], x0[7];
    for (int c = 0; c < 7; ++c) {
        xv[c] = x[(size_t)r * 7 + c];
        const float m = mo[(size_t)r * 7 + c];
        x0[c] = mean_type == DA_MEAN_START_X ? m : (xv[c] - sqrtf(beta) * m) / sqrtf(ap);
    }
    const float sr = s.sqrt_recip_alphas_cumprod[ti], srm1 = s.sqrt_recipm1_alphas_cumprod[ti];
    const float sq_prev = sqrtf(ap_prev), sq_dir = sqrtf(1.0f - ap_prev);
    float *o = x_prev + (size_t)r * 7;
    for (int c = 4; c < 7; ++c) {
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
__global__ __launch_bounds__(64) void k_head3d_bwd(int n, const float *__restrict__ pre, const float *__restrict__ d_out,
                                                   float *__restrict__ d_pre) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r0 = pre[(size_t)i * 6], r1 = pre[(size_t)i * 6 + 1], r2 = pre[(size_t)i * 6 + 2];
    const float *g = d_out + (size_t)i * 7;
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
    float *o = d_pre + (size_t)i * 6;
    o[0] = s * (k * g1 + a * r0);
    o[1] = s * (k * g2 + a * r1);
    o[2] = s * (k * g3 + a * r2);
    o[3] = g[4]; o[4] = g[5]; o[5] = g[6];
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
    float *o = x_noisy + (size_t)i * 7;
    for (int c = 0; c < 3; ++c) o[4 + c] = __fadd_rn(__fmul_rn(a, xs[4 + c]), __fmul_rn(b, noise_tr[(size_t)i * 3 + c]));      // k_q_sample's expression
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

int launch_head3d(int prec, int n, const void *hh, const float *wt, const float *bt, const float *wr, const float *br,
                  float *out7, float *pre_head, hipStream_t st) {
    if (n <= 0) return 0;
    const int grid = (int)(((size_t)n * 64 + 255) / 256);
    if (prec == DA_PREC_BF16)
        k_head3d<bf16_t><<<grid, 256, 0, st>>>(n, (const bf16_t *)hh, wt, bt, wr, br, out7, pre_head);
    else
        k_head3d<float><<<grid, 256, 0, st>>>(n, (const float *)hh, wt, bt, wr, br, out7, pre_head);
    DA_LAUNCH_CHECK();
    return 0;
}

int launch_ddim3d(const DeviceSchedule &s, int mean_type, int n, const float *x, const float *mo, const int64_t *t,
                  int64_t t_scalar, int ratio, int prev_all_nonneg, float *x_prev, hipStream_t st) {
    if (n <= 0) return 0;
    k_ddim3d<<<(n + 63) / 64, 64, 0, st>>>(s, mean_type, n, x, mo, t, t_scalar, ratio, prev_all_nonneg, x_prev);
    DA_LAUNCH_CHECK();
    return 0;
}

int launch_head3d_bwd(int n, const float *pre, const float *d_out, float *d_pre, hipStream_t st) {
    if (n <= 0) return 0;
    k_head3d_bwd<<<(n + 63) / 64, 64, 0, st>>>(n, pre, d_out, d_pre);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

using namespace da;

extern "C" {

int da_head3d_backward(int n, const float *pre, const float *d_out, float *d_pre, void *stream) {
    DA_REQUIRE(n >= 0, "da_head3d_backward: n < 0");
    DA_REQUIRE(pre && d_out && d_pre, "da_head3d_backward: null argument");
    return launch_head3d_bwd(n, pre, d_out, d_pre, (hipStream_t)stream);
}

int da_q_sample_se3(int steps, int n, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, const float *trap,
                    const float *x_start, const int64_t *t, const float *noise_tr, const float *axes, const float *unif, float *x_noisy,
                    void *stream) {
    DA_REQUIRE(steps > 0 && n >= 0, "da_q_sample_se3: steps must be positive and n >= 0");
    DA_REQUIRE(sqrt_alphas_cumprod && sqrt_one_minus_alphas_cumprod && trap && x_start && t && noise_tr && axes && unif && x_noisy,
               "da_q_sample_se3: null argument");
    if (n == 0) return 0;
    k_q_sample_se3<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(steps, n, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, trap, x_start, t,
                                                                  noise_tr, axes, unif, x_noisy);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
