// Training side of the discrete position + rotation diffusion (spatial_diffusion_discrete_rot.py:161-279): the two forward noisings of
// p_losses in one launch, and the two-head loss (variational bound, cross entropy, their hybrid) with its gradient with respect to both
// heads' logits.  Both processes have the uniform transition, so everything is da_d3pm_train.hip's closed form, once with K classes and
// once with four: one wave per piece, fp32, any K in [2, 1024].  The position row lives in LDS as there (two K-wide images per wave); the
// rotation row is four values and is evaluated by the same wave in registers.  k_d3pm_q_sample and k_d3pm_loss are not touched: the
// position model's bits stay what they were.
//
// What differs from the position model's loss (the reference's own choice, :208-273): "cross_entropy" smooths NEITHER head, "hybrid"
// smooths the position head's cross entropy (label_smoothing = 1e-2) and not the rotation head's.
#include <float.h>

#include "da_common.h"
#include "da_internal.h"

namespace da {

namespace {

constexpr int D3R_ROWS = 4;                       // pieces per workgroup = waves per workgroup

__device__ __forceinline__ float rt_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float rt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int rt_clamp_idx(int k, int K) { return k < 0 ? 0 : (k >= K ? K - 1 : k); }
__device__ __forceinline__ int64_t rt_clamp_t(int64_t t, int steps) { return t < 0 ? 0 : (t >= steps ? steps - 1 : t); }

// x_t = argmax_k( log(a_t [k == x0] + (1 - a_t) / Kc + 1e-9) - log(-log(clip(u_k, FLT_MIN, 1))) ) of one piece with Kc classes, by one
// wave: the expressions, the 2^-25 floor of -log u and the lowest-index tie rule of k_d3pm_q_sample.  e0 = r * Kc: the piece's first
// flat element (noise index, generator counter); `word` names the draw domain.  Every lane returns the winner.
__device__ __forceinline__ int q_sample_row(int Kc, int lane, size_t e0, float at, int x0, const float *__restrict__ noise,
                                            const uint64_t *__restrict__ seed, uint32_t iteration, uint32_t word) {
    const float off = (1.0f - at) / (float)Kc;
    const float l_hit = logf(at + off + 1e-9f), l_miss = logf(off + 1e-9f);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < Kc; k += 64) {
        const size_t e = e0 + k;
        float u = noise ? noise[e] : philox_uniform(seed[0], (uint64_t)e + seed[1], iteration, word);
        u = fminf(fmaxf(u, FLT_MIN), 1.0f);
        const float v = (k == x0 ? l_hit : l_miss) - logf(fmaxf(-logf(u), 2.98023223876953125e-8f));
        if (v > best) { best = v; bi = k; }                        // ascending k per lane: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi == 0x7fffffff ? 0 : bi;
}

}  // namespace

// ------------------------------------------------------------------------------------------ the two noisings
// One wave per piece: the K-wide position draw (skipped when x_noisy == NULL: only_rotation), then the four-wide rotation draw on
// lanes 0..3 of the same wave.  The position half draws in the TRAINING domain (the stream of k_d3pm_q_sample), the rotation half in
// TRAINING_ROT, flat element r * 4 + k.
__global__ __launch_bounds__(64 * D3R_ROWS) void k_d3pm_q_sample_rot(int n, int K, int steps, const float *__restrict__ alphas_cumprod,
                                                                     const int32_t *__restrict__ x_start, const int32_t *__restrict__ rot_start,
                                                                     const int64_t *__restrict__ t, const float *__restrict__ noise_x,
                                                                     const float *__restrict__ noise_rot, const uint64_t *__restrict__ seed,
                                                                     uint32_t iteration, int32_t *__restrict__ x_noisy,
                                                                     int32_t *__restrict__ rot_noisy) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * D3R_ROWS + (threadIdx.x >> 6);
    if (r >= n) return;
    const float at = alphas_cumprod[rt_clamp_t(t[r], steps)];
    if (x_noisy) {
        const int xn = q_sample_row(K, lane, (size_t)r * K, at, rt_clamp_idx(x_start[r], K), noise_x, seed, iteration, D3PM_WORD_TRAINING);
        if (lane == 0) x_noisy[r] = xn;
    }
    const int rn = q_sample_row(4, lane, (size_t)r * 4, at, rot_start[r] & 3, noise_rot, seed, iteration, D3PM_WORD_TRAINING_ROT);
    if (lane == 0) rot_noisy[r] = rn;
}

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
// One wave per piece.  Position row: k_d3pm_loss's walk over z and a second K-wide image (m, then h) in LDS, with the label smoothing
// `smooth` of its cross entropy an argument (y = (1 - smooth) e_x0 + smooth / K; 0 gives the plain cross entropy).  logits == NULL
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
    const float inv_ln2 = 1.4426950408889634f, inv_n = 1.0f / (float)n;
    const int64_t ti = rt_clamp_t(t[r], steps);
    float vb_row = 0.f, ce_row = 0.f;
    if (logits) {
        float *z = lds + (size_t)wv * 2 * K, *mh = z + K;
        const float *zr = logits + (size_t)r * K;
        float *dz = d_logits + (size_t)r * K;
        const int x0 = rt_clamp_idx(x_start[r], K);
        float zmax = -FLT_MAX;
        for (int k = lane; k < K; k += 64) { const float v = zr[k]; z[k] = v; zmax = fmaxf(zmax, v); }
        zmax = rt_wave_max(zmax);
        float se = 0.f, sz = 0.f;
        for (int k = lane; k < K; k += 64) { const float d = z[k] - zmax; se += expf(d); sz += d; }
        se = rt_wave_sum(se);
        sz = rt_wave_sum(sz);                                        // sum_k (z[k] - zmax)
        const float lse = logf(se), inv_se = 1.0f / se;
        const float lp_x0 = __shfl((x0 & 63) == lane ? z[x0] : 0.f, x0 & 63, 64) - zmax - lse;
        const float y_miss = smooth / (float)K, y_hit = (1.0f - smooth) + y_miss;
        ce_row = smooth > 0.f ? -((1.0f - smooth) * lp_x0 + y_miss * (sz - (float)K * lse)) : -lp_x0;
        if (!want_vb || ti == 0) {
            if (want_vb) vb_row = -lp_x0 * inv_ln2;
            const float wv0 = want_vb ? w_vb * inv_ln2 : 0.f;
            for (int k = lane; k < K; k += 64) {
                const float pi = expf(z[k] - zmax) * inv_se;
                dz[k] = (wv0 * (pi - (k == x0 ? 1.f : 0.f)) + w_ce * (pi - (k == x0 ? y_hit : y_miss))) * inv_n;
            }
        } else {
            const int xt = rt_clamp_idx(x_t[r], K);
            const float at = alphas_cumprod[ti], ap = alphas_cumprod[ti - 1];
            const float rr = at / ap, c1 = ((ap - at) / ap) / (float)K, c2 = (1.0f - ap) / (float)K;
            const float lf_hit = logf(rr + c1 + 1e-8f), lf_miss = logf(c1 + 1e-8f);
            float mmax = -FLT_MAX;
            for (int k = lane; k < K; k += 64) {
                const float pi = expf(z[k] - zmax) * inv_se;
                const float v = (k == xt ? lf_hit : lf_miss) + logf(fmaf(ap, pi, c2) + 1e-8f);
                mh[k] = v;
                mmax = fmaxf(mmax, v);
            }
            mmax = rt_wave_max(mmax);
            float sm = 0.f;
            for (int k = lane; k < K; k += 64) sm += expf(mh[k] - mmax);
            sm = rt_wave_sum(sm);
            const float lsm = logf(sm), inv_sm = 1.0f / sm;
            // true posterior: at most four distinct values, classes both | x_t only | x0 only | neither
            const float l2_hit = logf(ap + c2 + 1e-8f), l2_miss = logf(c2 + 1e-8f);
            const bool same = xt == x0;
            const float qv[4] = {lf_hit + l2_hit, lf_hit + l2_miss, lf_miss + l2_hit, lf_miss + l2_miss};
            const float cnt[4] = {same ? 1.f : 0.f, same ? 0.f : 1.f, same ? 0.f : 1.f, (float)(K - (same ? 1 : 2))};
            float qmax = -FLT_MAX;
#pragma unroll
            for (int c = 0; c < 4; ++c) if (cnt[c] > 0.f) qmax = fmaxf(qmax, qv[c]);
            float qz = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) if (cnt[c] > 0.f) qz += cnt[c] * expf(qv[c] - qmax);
            const float lqz = logf(qz);
            float lq[4], q[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { lq[c] = qv[c] - qmax - lqz; q[c] = expf(lq[c]); }
            float kl = 0.f, sph = 0.f;
            for (int k = lane; k < K; k += 64) {
                const int c = (k == xt ? 0 : 2) + (k == x0 ? 0 : 1);
                const float qk = c == 0 ? q[0] : (c == 1 ? q[1] : (c == 2 ? q[2] : q[3]));
                const float lqk = c == 0 ? lq[0] : (c == 1 ? lq[1] : (c == 2 ? lq[2] : lq[3]));
                const float d = mh[k] - mmax;
                kl += qk * (lqk - (d - lsm));
                const float pi = expf(z[k] - zmax) * inv_se;
                const float h = (expf(d) * inv_sm - qk) * inv_ln2 * ap / (fmaf(ap, pi, c2) + 1e-8f);
                mh[k] = h;
                sph += pi * h;
            }
            kl = rt_wave_sum(kl);
            sph = rt_wave_sum(sph);
            vb_row = kl * inv_ln2;
            for (int k = lane; k < K; k += 64) {
                const float pi = expf(z[k] - zmax) * inv_se;
                dz[k] = (w_vb * pi * (mh[k] - sph) + w_ce * (pi - (k == x0 ? y_hit : y_miss))) * inv_n;
            }
        }
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
    if (n == 0) return 0;
    k_d3pm_q_sample_rot<<<(unsigned)((n + D3R_ROWS - 1) / D3R_ROWS), 64 * D3R_ROWS, 0, (hipStream_t)stream>>>(
        n, K, s->steps, s->alphas_cumprod, x_start, rot_start, t, noise_x, noise_rot, seed, (uint32_t)iteration, x_noisy, rot_noisy);
    DA_LAUNCH_CHECK();
    return 0;
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
