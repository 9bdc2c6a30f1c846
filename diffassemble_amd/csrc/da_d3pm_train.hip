// Training side of the discrete (D3PM, uniform transition) position diffusion: the forward noising q_sample, the loss of p_losses
// (variational bound, label-smoothed cross entropy, their hybrid) with its gradient with respect to the logits, and the gradient of
// the position-embedding lookup (spatial_diffusion_discrete.py:181-191, 229-273, 416-488; efficient_gat_discrete.py:81-86).
//
// As in da_d3pm.hip no [steps, K, K] table exists: overline_Q[t] = a_t I + (1 - a_t) / K 11^T and
// overline_Q[t] overline_Q[t - 1]^-1 = r I + (1 - r) / K 11^T with r = a_t / a_{t-1}, so every row needs a handful of scalars.
// The noising and the loss are K-wide per-piece work, one wave per piece, fp32, any K in [2, 1024], no per-lane arrays sized by K (a
// row's K values live in LDS, k_d3pm_tail's note); the embedding gradient has one workgroup per table row.
#include <float.h>

#include "da_common.h"
#include "da_internal.h"

namespace da {

constexpr int D3T_ROWS = 4;                       // pieces per workgroup = waves per workgroup

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int clamp_idx(int k, int K) { return k < 0 ? 0 : (k >= K ? K - 1 : k); }
__device__ __forceinline__ int64_t clamp_t(int64_t t, int steps) { return t < 0 ? 0 : (t >= steps ? steps - 1 : t); }

// ------------------------------------------------------------------------------------------ q_sample
// x_t = argmax_k( log(a_t [k == x0] + (1 - a_t) / K + 1e-9) - log(-log(clip(u_k, FLT_MIN, 1))) ): the first term takes two values per
// piece.  The uniforms are given (noise) or drawn here by the shared generator in the TRAINING domain.
__global__ __launch_bounds__(64 * D3T_ROWS) void k_d3pm_q_sample(int n, int K, int steps, const float *__restrict__ alphas_cumprod,
                                                                 const int32_t *__restrict__ x_start, const int64_t *__restrict__ t,
                                                                 const float *__restrict__ noise, const uint64_t *__restrict__ seed,
                                                                 uint32_t iteration, int32_t *__restrict__ x_noisy) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * D3T_ROWS + (threadIdx.x >> 6);
    if (r >= n) return;
    const float at = alphas_cumprod[clamp_t(t[r], steps)];
    const int x0 = clamp_idx(x_start[r], K);
    const float off = (1.0f - at) / (float)K;
    const float l_hit = logf(at + off + 1e-9f), l_miss = logf(off + 1e-9f);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const size_t e = (size_t)r * K + k;
        float u = noise ? noise[e] : philox_uniform(seed[0], (uint64_t)e + seed[1], iteration, D3PM_WORD_TRAINING);
        u = fminf(fmaxf(u, FLT_MIN), 1.0f);
        // the inner term is floored at 2^-25 so that u == 1 (one generated value in 2^24) stays finite (da_d3pm.hip)
        const float v = (k == x0 ? l_hit : l_miss) - logf(fmaxf(-logf(u), 2.98023223876953125e-8f));
        if (v > best) { best = v; bi = k; }                        // ascending k per lane: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) x_noisy[r] = bi == 0x7fffffff ? 0 : bi;
}

// ------------------------------------------------------------------------------------------ loss + d loss / d logits
// One wave per piece; the row's logits z and a second K-wide image (m, then h) sit in LDS.  With pi = softmax(z):
//   ce_row = -(0.99 log pi[x0] + (0.01 / K) sum_k log pi[k]),                 d / dz = pi - y
//   t == 0: vb_row = -log pi[x0] / ln 2,                                      d / dz = (pi - e_x0) / ln 2
//   t  > 0: m[k] = lf[k] + log(a_p pi[k] + c2 + eps), lf[k] = log(r [k == x_t] + c1 + eps)        (two values)
//           q~[k] = lf[k] + log(a_p [k == x0] + c2 + eps)                                          (at most four values: the classes
//                   (k == x_t, k == x0) = both | x_t only | x0 only | neither, with 1 | 1 | 1 | K - 1 or K - 2 members)
//           vb_row = sum_k q[k] (log q[k] - log_softmax(m)[k]) / ln 2
//           g[k] = (softmax(m)[k] - q[k]) / ln 2, h[k] = g[k] a_p / (a_p pi[k] + c2 + eps), d / dz[j] = pi[j] (h[j] - sum_k pi[k] h[k])
// Both softmaxes are max-subtracted.  d_logits = (w_vb d vb_row + w_ce d ce_row) / n; the row terms go to row_terms [n, 2] and
// k_d3pm_loss_finish sums them in a fixed order.
__global__ __launch_bounds__(64 * D3T_ROWS) void k_d3pm_loss(int n, int K, int steps, const float *__restrict__ alphas_cumprod, int want_vb,
                                                             float w_vb, float w_ce, const float *__restrict__ logits,
                                                             const int32_t *__restrict__ x_start, const int32_t *__restrict__ x_t,
                                                             const int64_t *__restrict__ t, float *__restrict__ d_logits,
                                                             float *__restrict__ row_terms) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = blockIdx.x * D3T_ROWS + wv;
    if (r >= n) return;                                              // (no workgroup barrier below: a wave owns its LDS rows)
    float *z = lds + (size_t)wv * 2 * K, *mh = z + K;
    const float inv_ln2 = 1.4426950408889634f, inv_n = 1.0f / (float)n;
    const float *zr = logits + (size_t)r * K;
    float *dz = d_logits + (size_t)r * K;
    const int x0 = clamp_idx(x_start[r], K);
    const int64_t ti = clamp_t(t[r], steps);

    float zmax = -FLT_MAX;
    for (int k = lane; k < K; k += 64) { const float v = zr[k]; z[k] = v; zmax = fmaxf(zmax, v); }
    zmax = wave_max(zmax);
    float se = 0.f, sz = 0.f;
    for (int k = lane; k < K; k += 64) { const float d = z[k] - zmax; se += expf(d); sz += d; }
    se = wave_sum(se);
    sz = wave_sum(sz);                                               // sum_k (z[k] - zmax)
    const float lse = logf(se), inv_se = 1.0f / se;
    // log pi[x0]: read by the lane that wrote z[x0] and handed round (every LDS word stays private to the lane that owns column k)
    const float lp_x0 = __shfl((x0 & 63) == lane ? z[x0] : 0.f, x0 & 63, 64) - zmax - lse;
    const float ce_row = -(0.99f * lp_x0 + (0.01f / (float)K) * (sz - (float)K * lse));
    const float y_hit = 0.99f + 0.01f / (float)K, y_miss = 0.01f / (float)K;

    float vb_row = 0.f;
    if (!want_vb || ti == 0) {
        // cross entropy alone, or the decoder NLL of t == 0: both gradients are pi minus a constant pattern
        if (want_vb) vb_row = -lp_x0 * inv_ln2;
        const float wv0 = want_vb ? w_vb * inv_ln2 : 0.f;
        for (int k = lane; k < K; k += 64) {
            const float pi = expf(z[k] - zmax) * inv_se;
            dz[k] = (wv0 * (pi - (k == x0 ? 1.f : 0.f)) + w_ce * (pi - (k == x0 ? y_hit : y_miss))) * inv_n;
        }
    } else {
        const int xt = clamp_idx(x_t[r], K);
        const float at = alphas_cumprod[ti], ap = alphas_cumprod[ti - 1];
        const float rr = at / ap, c1 = ((ap - at) / ap) / (float)K, c2 = (1.0f - ap) / (float)K;     // c1 = (1 - r) / K without the cancellation
        const float lf_hit = logf(rr + c1 + 1e-8f), lf_miss = logf(c1 + 1e-8f);
        // model posterior logits m, their max and partition sum
        float mmax = -FLT_MAX;
        for (int k = lane; k < K; k += 64) {
            const float pi = expf(z[k] - zmax) * inv_se;
            const float v = (k == xt ? lf_hit : lf_miss) + logf(fmaf(ap, pi, c2) + 1e-8f);
            mh[k] = v;
            mmax = fmaxf(mmax, v);
        }
        mmax = wave_max(mmax);
        float sm = 0.f;
        for (int k = lane; k < K; k += 64) sm += expf(mh[k] - mmax);
        sm = wave_sum(sm);
        const float lsm = logf(sm), inv_sm = 1.0f / sm;
        // true posterior: the four classes (every lane computes the same scalars)
        const float l2_hit = logf(ap + c2 + 1e-8f), l2_miss = logf(c2 + 1e-8f);
        const bool same = xt == x0;
        const float qv[4] = {lf_hit + l2_hit, lf_hit + l2_miss, lf_miss + l2_hit, lf_miss + l2_miss};      // both | x_t only | x0 only | neither
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
        // KL row, h[k] and sum_k pi[k] h[k]
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
        kl = wave_sum(kl);
        sph = wave_sum(sph);
        vb_row = kl * inv_ln2;
        for (int k = lane; k < K; k += 64) {
            const float pi = expf(z[k] - zmax) * inv_se;
            dz[k] = (w_vb * pi * (mh[k] - sph) + w_ce * (pi - (k == x0 ? y_hit : y_miss))) * inv_n;
        }
    }
    if (lane == 0) { row_terms[(size_t)r * 2] = vb_row; row_terms[(size_t)r * 2 + 1] = ce_row; }
}

// loss[0 .. 2] = {w_vb mean vb + w_ce mean ce, mean vb, mean ce}: ONE workgroup, thread-strided partial sums, then a tree in LDS (the
// order of da_loss_grad's reduction): deterministic, data-parallel replicas agree bit for bit
__global__ __launch_bounds__(1024) void k_d3pm_loss_finish(int n, int want_vb, float w_vb, float w_ce, const float *__restrict__ row_terms,
                                                           float *__restrict__ loss) {
    __shared__ float red[2][1024];
    float a = 0.f, b = 0.f;
    for (int r = threadIdx.x; r < n; r += 1024) { a += row_terms[(size_t)r * 2]; b += row_terms[(size_t)r * 2 + 1]; }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float vb = want_vb ? red[0][0] / (float)n : 0.f, ce = w_ce != 0.f ? red[1][0] / (float)n : 0.f;
        loss[0] = w_vb * vb + w_ce * ce;
        loss[1] = vb;
        loss[2] = ce;
    }
}

// ------------------------------------------------------------------------------------------ embedding gradient
// pos_mlp.weight.grad[k][c] += sum over the pieces r with idx[r] == k of dcomb[r][F + c].  After noising many pieces of a puzzle share an
// index, so a scatter with float atomics would make the sum's order -- and its bits -- depend on scheduling.  Here table row k has ONE
// owner, a workgroup of 32 groups x 32 channels: group g takes the 32-piece chunks g, g + 32, ... in ascending order -- its 32 lanes
// read the chunk's indices in one coalesced load, a ballot gives the chunk's matches, and lane c adds channel c of the matching pieces
// in ascending order -- and the 32 partial sums are added in a fixed order.  Every workgroup reads idx once (37 KB from the L2 at
// 9 216 pieces, nine independent loads per lane).
constexpr int EIG_GROUPS = 32;
__global__ __launch_bounds__(32 * EIG_GROUPS) void k_embed_idx_grad(int n, int K, int D, int F, const int32_t *__restrict__ idx,
                                                                   const float *__restrict__ dcomb, float *grad) {
    __shared__ float part[EIG_GROUPS][32];
    const int k = blockIdx.x, g = threadIdx.x >> 5, c = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    float s = 0.f;
    for (int r0 = g * 32; r0 < n; r0 += 32 * EIG_GROUPS) {           // (uniform over the wave's two groups up to the last chunk)
        const int r = r0 + c;
        const bool hit = r < n && clamp_idx(idx[r], K) == k;
        unsigned m = (unsigned)(__ballot(hit) >> (32 * half));      // the matches of this group's chunk
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            s += dcomb[(size_t)(r0 + b) * D + F + c];
        }
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0) {
        float a = part[0][c];
#pragma unroll
        for (int j = 1; j < EIG_GROUPS; ++j) a += part[j][c];
        grad[(size_t)k * 32 + c] += a;
    }
}

int launch_embed_idx_grad(int n, int K, int D, int F, const int32_t *idx, const float *dcomb, float *grad, hipStream_t st) {
    if (n <= 0 || K <= 0) return 0;
    k_embed_idx_grad<<<(unsigned)K, 32 * EIG_GROUPS, 0, st>>>(n, K, D, F, idx, dcomb, grad);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

using namespace da;

extern "C" {

int da_d3pm_q_sample(const da_schedule *s, int n, int K, const int32_t *x_start, const int64_t *t, const float *noise,
                     const uint64_t *seed, int iteration, int32_t *x_noisy, void *stream) {
    DA_REQUIRE(s && x_start && t && x_noisy, "da_d3pm_q_sample: null argument");
    DA_REQUIRE(n >= 0 && K >= 2 && K <= 1024, "da_d3pm_q_sample: K = %d outside [2, 1024]", K);
    DA_REQUIRE(s->steps >= 1 && s->alphas_cumprod, "da_d3pm_q_sample: bad schedule");
    DA_REQUIRE(noise || seed, "da_d3pm_q_sample: needs the uniforms (noise) or a seed");
    if (n == 0) return 0;
    k_d3pm_q_sample<<<(unsigned)((n + D3T_ROWS - 1) / D3T_ROWS), 64 * D3T_ROWS, 0, (hipStream_t)stream>>>(
        n, K, s->steps, s->alphas_cumprod, x_start, t, noise, seed, (uint32_t)iteration, x_noisy);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_d3pm_loss(const da_schedule *s, int n, int K, int kind, float lambda, const float *logits, const int32_t *x_start,
                 const int32_t *x_t, const int64_t *t, float *loss, float *d_logits, float *row_terms, void *stream) {
    DA_REQUIRE(s && logits && x_start && x_t && t && loss && d_logits && row_terms, "da_d3pm_loss: null argument");
    DA_REQUIRE(n >= 1 && K >= 2 && K <= 1024, "da_d3pm_loss: n = %d, K = %d (n >= 1, K in [2, 1024])", n, K);
    DA_REQUIRE(s->steps >= 1 && s->alphas_cumprod, "da_d3pm_loss: bad schedule");
    DA_REQUIRE(kind == DA_D3PM_LOSS_VB || kind == DA_D3PM_LOSS_CE || kind == DA_D3PM_LOSS_HYBRID, "da_d3pm_loss: unknown kind %d", kind);
    const int want_vb = kind != DA_D3PM_LOSS_CE;
    const float w_vb = want_vb ? 1.f : 0.f, w_ce = kind == DA_D3PM_LOSS_CE ? 1.f : (kind == DA_D3PM_LOSS_HYBRID ? lambda : 0.f);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)D3T_ROWS * 2 * K * sizeof(float);                             // <= 32 KiB at K = 1024
    k_d3pm_loss<<<(unsigned)((n + D3T_ROWS - 1) / D3T_ROWS), 64 * D3T_ROWS, lds, st>>>(n, K, s->steps, s->alphas_cumprod, want_vb, w_vb, w_ce,
                                                                                     logits, x_start, x_t, t, d_logits, row_terms);
    k_d3pm_loss_finish<<<1, 1024, 0, st>>>(n, want_vb, w_vb, w_ce, row_terms, loss);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
