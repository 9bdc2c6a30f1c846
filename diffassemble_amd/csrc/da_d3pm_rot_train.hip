// Training side of the discrete position + rotation diffusion (spatial_diffusion_discrete_rot.py:161-279): the two-head loss
// (variational bound, cross entropy, their hybrid) with its gradient with respect to both heads' logits.  Both processes have the
// uniform transition, so everything is da_d3pm_train.hip's closed form, once with K classes and once with four: one wave per piece,
// fp32, any K in [2, 1024].  The position row is d3pm_loss_row of da_d3pm_common.h, the copy k_d3pm_loss runs (two K-wide LDS images
// per wave); the rotation row is four values and is evaluated by the same wave in registers.  The two forward noisings of p_losses
// are one launch of da_d3pm_train.hip's noising kernel with both halves.
//
// What differs from the position model's loss (the reference's own choice, :208-273): "cross_entropy" smooths NEITHER head, "hybrid"
// smooths the position head's cross entropy (label_smoothing = 1e-2) and not the rotation head's.
#include "da_common.h"
#include "da_d3pm_common.h"
#include "da_internal.h"

namespace da {

constexpr int D3R_ROWS = 4;                       // pieces per workgroup = waves per workgroup

// ------------------------------------------------------------------------------------------ the rotation row, in registers
// k_d3pm_loss's formulas for four classes, every lane of the wave computing the same scalars (the loops are unrolled: z, pi, m, h are
// registers; the class of an index is found by comparison, never by indexing).  Cross entropy unsmoothed.
__device__ __forceinline__ void rot_loss_row(const float *__restrict__ zr, int x0, int xt, int64_t ti, const float *__restrict__ alphas_cumprod,
                                             int want_vb, float w_vb, float w_ce, float inv_n, float dz[4], float &vb_row, float &ce_row) {
    const float inv_ln2 = 1.4426950408889634f;
    float z[4], pi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = zr[k];
    const float zmax = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { pi[k] = expf(z[k] - zmax); se += pi[k]; }
    const float lse = logf(se), inv_se = 1.0f / se;
    float z_x0 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { pi[k] *= inv_se; z_x0 = k == x0 ? z[k] : z_x0; }
    const float lp_x0 = z_x0 - zmax - lse;
    ce_row = -lp_x0;
    vb_row = 0.f;
    if (!want_vb || ti == 0) {
        if (want_vb) vb_row = -lp_x0 * inv_ln2;
        const float wv0 = want_vb ? w_vb * inv_ln2 : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = pi[k] - (k == x0 ? 1.f : 0.f);
            dz[k] = (wv0 * d + w_ce * d) * inv_n;
        }
        return;
    }
    const float at = alphas_cumprod[ti], ap = alphas_cumprod[ti - 1];
    const float rr = at / ap, c1 = ((ap - at) / ap) * 0.25f, c2 = (1.0f - ap) * 0.25f;
    const float lf_hit = logf(rr + c1 + 1e-8f), lf_miss = logf(c1 + 1e-8f);
    const float l2_hit = logf(ap + c2 + 1e-8f), l2_miss = logf(c2 + 1e-8f);
    float m[4], qt[4], den[4];
    float mmax = -FLT_MAX, qmax = -FLT_MAX;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lf = k == xt ? lf_hit : lf_miss;
        den[k] = fmaf(ap, pi[k], c2) + 1e-8f;
        m[k] = lf + logf(den[k]);
        qt[k] = lf + (k == x0 ? l2_hit : l2_miss);
        mmax = fmaxf(mmax, m[k]);
        qmax = fmaxf(qmax, qt[k]);
    }
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sm += expf(m[k] - mmax); sq += expf(qt[k] - qmax); }
    const float lsm = logf(sm), inv_sm = 1.0f / sm, lsq = logf(sq);
    float kl = 0.f, sph = 0.f, h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lq = qt[k] - qmax - lsq, q = expf(lq), d = m[k] - mmax;
        kl += q * (lq - (d - lsm));
        h[k] = (expf(d) * inv_sm - q) * inv_ln2 * ap / den[k];
        sph += pi[k] * h[k];
    }
    vb_row = kl * inv_ln2;
#pragma unroll
    for (int k = 0; k < 4; ++k) dz[k] = (w_vb * pi[k] * (h[k] - sph) + w_ce * (pi[k] - (k == x0 ? 1.f : 0.f))) * inv_n;
}

// ------------------------------------------------------------------------------------------ loss + d loss / d logits, both heads
// One wave per piece.  Position row: d3pm_loss_row with the label smoothing `smooth` of its cross entropy.  logits == NULL
// (only_rotation): the position half is skipped, d_logits is not written and the row's position terms read 0.  Then the rotation row.
// row_terms [n, 4] = {x_vb, x_ce, rot_vb, rot_ce}.
__global__ __launch_bounds__(64 * D3R_ROWS) void k_d3pm_rot_loss(int n, int K, int steps, const float *__restrict__ alphas_cumprod, int want_vb,
                                                                 float w_vb, float w_ce, float smooth, const float *__restrict__ logits,
                                                                 const float *__restrict__ rot_logits, const int32_t *__restrict__ x_start,
                                                                 const int32_t *__restrict__ x_t, const int32_t *__restrict__ rot_start,
                                                                 const int32_t *__restrict__ rot_t, const int64_t *__restrict__ t,
                                                                 float *__restrict__ d_logits, float *__restrict__ d_rot_logits,
                                                                 float *__restrict__ row_terms) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = blockIdx.x * D3R_ROWS + wv;
    if (r >= n) return;                                              // (no workgroup barrier below: a wave owns its LDS rows)
    const float inv_n = 1.0f / (float)n;
    const int64_t ti = clamp_t(t[r], steps);
    float vb_row = 0.f, ce_row = 0.f;
    if (logits) {
        float *z = lds + (size_t)wv * 2 * K;
        d3pm_loss_row(z, z + K, K, lane, logits + (size_t)r * K, d_logits + (size_t)r * K, clamp_idx(x_start[r], K), x_t + r,
                      ti, alphas_cumprod, want_vb, w_vb, w_ce, smooth, inv_n, vb_row, ce_row);
    }
    float rdz[4], rvb, rce;
    rot_loss_row(rot_logits + (size_t)r * 4, rot_start[r] & 3, rot_t[r] & 3, ti, alphas_cumprod, want_vb, w_vb, w_ce, inv_n, rdz, rvb, rce);
    if (lane == 0) {
        *(float4 *)(d_rot_logits + (size_t)r * 4) = make_float4(rdz[0], rdz[1], rdz[2], rdz[3]);
        *(float4 *)(row_terms + (size_t)r * 4) = make_float4(vb_row, ce_row, rvb, rce);
    }
}

// loss[0 .. 5] = {x_loss, rot_loss, mean x_vb, mean x_ce, mean rot_vb, mean rot_ce}: ONE workgroup, thread-strided partial sums, then a
// tree in LDS (k_d3pm_loss_finish's order): deterministic.  A term the kind does not use reads 0; without the position head so do its three.
__global__ __launch_bounds__(1024) void k_d3pm_rot_loss_finish(int n, int want_vb, float w_vb, float w_ce, int has_x,
                                                               const float *__restrict__ row_terms, float *__restrict__ loss) {
    __shared__ float red[4][1024];
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < n; r += 1024) {
        const float4 v = *(const float4 *)(row_terms + (size_t)r * 4);
        a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = a[c];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float inv = 1.0f / (float)n;
        const float xvb = (want_vb && has_x) ? red[0][0] * inv : 0.f, xce = (w_ce != 0.f && has_x) ? red[1][0] * inv : 0.f;
        const float rvb = want_vb ? red[2][0] * inv : 0.f, rce = w_ce != 0.f ? red[3][0] * inv : 0.f;
        loss[0] = w_vb * xvb + w_ce * xce;
        loss[1] = w_vb * rvb + w_ce * rce;
        loss[2] = xvb; loss[3] = xce; loss[4] = rvb; loss[5] = rce;
    }
}

}  // namespace da

using namespace da;

extern "C" {

int da_d3pm_q_sample_rot(const da_schedule *s, int n, int K, const int32_t *x_start, const int32_t *rot_start, const int64_t *t,
                         const float *noise_x, const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_noisy,
                         int32_t *rot_noisy, void *stream) {
    DA_REQUIRE(s && rot_start && t && rot_noisy, "da_d3pm_q_sample_rot: null argument");
    DA_REQUIRE(!x_noisy || x_start, "da_d3pm_q_sample_rot: x_noisy asked for without x_start");
    DA_REQUIRE(n >= 0 && K >= 2 && K <= 1024, "da_d3pm_q_sample_rot: K = %d outside [2, 1024]", K);
    DA_REQUIRE(s->steps >= 1 && s->alphas_cumprod, "da_d3pm_q_sample_rot: bad schedule");
    DA_REQUIRE(seed || (noise_rot && (noise_x || !x_noisy)), "da_d3pm_q_sample_rot: needs the uniforms (noise_x, noise_rot) or a seed");
    return launch_d3pm_q_sample(n, K, s, x_start, rot_start, t, noise_x, noise_rot, seed, iteration, x_noisy, rot_noisy, (hipStream_t)stream);
}

int da_d3pm_rot_loss(const da_schedule *s, int n, int K, int kind, float lambda, const float *logits, const float *rot_logits,
                     const int32_t *x_start, const int32_t *x_t, const int32_t *rot_start, const int32_t *rot_t, const int64_t *t,
                     float *loss, float *d_logits, float *d_rot_logits, float *row_terms, void *stream) {
    DA_REQUIRE(s && rot_logits && rot_start && rot_t && t && loss && d_rot_logits && row_terms, "da_d3pm_rot_loss: null argument");
    DA_REQUIRE(!logits || (x_start && x_t && d_logits), "da_d3pm_rot_loss: logits given without x_start / x_t / d_logits");
    DA_REQUIRE(n >= 1 && K >= 2 && K <= 1024, "da_d3pm_rot_loss: n = %d, K = %d (n >= 1, K in [2, 1024])", n, K);
    DA_REQUIRE(s->steps >= 1 && s->alphas_cumprod, "da_d3pm_rot_loss: bad schedule");
    DA_REQUIRE(kind == DA_D3PM_LOSS_VB || kind == DA_D3PM_LOSS_CE || kind == DA_D3PM_LOSS_HYBRID, "da_d3pm_rot_loss: unknown kind %d", kind);
    const int want_vb = kind != DA_D3PM_LOSS_CE;
    const float w_vb = want_vb ? 1.f : 0.f, w_ce = kind == DA_D3PM_LOSS_CE ? 1.f : (kind == DA_D3PM_LOSS_HYBRID ? lambda : 0.f);
    const float smooth = kind == DA_D3PM_LOSS_HYBRID ? 0.01f : 0.f;      // the position head's cross entropy; the rotation head's never is
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = logits ? (size_t)D3R_ROWS * 2 * K * sizeof(float) : 0;                // <= 32 KiB at K = 1024
    k_d3pm_rot_loss<<<(unsigned)((n + D3R_ROWS - 1) / D3R_ROWS), 64 * D3R_ROWS, lds, st>>>(
        n, K, s->steps, s->alphas_cumprod, want_vb, w_vb, w_ce, smooth, logits, rot_logits, x_start, x_t, rot_start, rot_t, t, d_logits,
        d_rot_logits, row_terms);
    k_d3pm_rot_loss_finish<<<1, 1024, 0, st>>>(n, want_vb, w_vb, w_ce, logits ? 1 : 0, row_terms, loss);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
