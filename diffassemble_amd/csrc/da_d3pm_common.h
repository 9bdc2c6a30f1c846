// The closed-form D3PM (uniform transition) row routines, ONE copy for the position model (da_d3pm.hip, da_d3pm_train.hip) and the
// position + rotation model (da_d3pm_rot.hip, da_d3pm_rot_train.hip): the Gumbel term, the noising row, the reverse step's categorical
// row and the K-wide loss row.  Device only; one wave per row, fp32, any class count in [2, 1024].  The two models sample the same
// positions from the same seed because they run these very expressions; keep each expression tree as it is (the compiler contracts
// into FMAs across statements) and the class count a run-time value.
#pragma once
#include <float.h>

#include "da_internal.h"

namespace da {

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

// -log(-log u) of a uniform clipped to [FLT_MIN, 1]; the inner term is floored at 2^-25 so that u == 1 (one generated value in 2^24)
// stays finite
__device__ __forceinline__ float gumbel(float u) {
    u = fminf(fmaxf(u, FLT_MIN), 1.0f);
    return -logf(fmaxf(-logf(u), 2.98023223876953125e-8f));
}

// wave-wide (value, index) argmax with the lowest index winning ties; an all-empty wave (no lane had a candidate) gives 0
__device__ __forceinline__ int wave_argmax_first(float best, int bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi == 0x7fffffff ? 0 : bi;
}

// ------------------------------------------------------------------------------------------ noising row (q_sample)
// x_t = argmax_k( log(a_t [k == x0] + (1 - a_t) / Kc + 1e-9) - log(-log(clip(u_k, FLT_MIN, 1))) ) of one piece with Kc classes, by one
// wave: the first term takes two values per piece.  e0 = r * Kc: the piece's first flat element (noise index, generator counter);
// `word` names the draw domain.  Every lane returns the winner.
__device__ __forceinline__ int q_sample_row(int Kc, int lane, size_t e0, float at, int x0, const float *__restrict__ noise,
                                            const uint64_t *__restrict__ seed, uint32_t iteration, uint32_t word) {
    const float off = (1.0f - at) / (float)Kc;
    const float l_hit = logf(at + off + 1e-9f), l_miss = logf(off + 1e-9f);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < Kc; k += 64) {
        const size_t e = e0 + k;
        const float u = noise ? noise[e] : philox_uniform(seed[0], (uint64_t)e + seed[1], iteration, word);
        const float v = (k == x0 ? l_hit : l_miss) + gumbel(u);
        if (v > best) { best = v; bi = k; }                        // ascending k per lane: the first maximum stays
    }
    return wave_argmax_first(best, bi);
}

// ------------------------------------------------------------------------------------------ reverse-step row
// The reverse step's timestep of node r: t clamped to the schedule, and where t > 0 a_t and a_p = alphas_cumprod[t - ratio]
// (precondition: t >= ratio wherever t > 0).  Returns t == 0.
__device__ __forceinline__ bool d3pm_step_alphas(const DeviceSchedule &s, const int64_t *t, int64_t t_scalar, int ratio, int r, float &at,
                                                 float &ap) {
    const int64_t ti = clamp_t(t ? t[r] : t_scalar, s.steps);
    at = ap = 1.f;
    if (ti == 0) return true;
    const int64_t tp = ti - ratio;
    at = s.alphas_cumprod[ti];
    ap = s.alphas_cumprod[tp < 0 ? 0 : tp];
    return false;
}

// One wave, one node, one categorical variable with Kc categories whose logits l[] lie in LDS.  With pi = softmax(l):
//    post[k] = log(f1[k] + 1e-8) + log(a_p pi[k] + (1 - a_p) / Kc + 1e-8),   f1[k] = r [k == x_t] + (1 - r) / Kc,   r = a_t / a_p
// (log f1 takes two values per node), then the Gumbel term and a first-index argmax; every lane returns the winner.  t0: the argmax
// of the logits.  e0 = r * Kc: the node's first flat element (noise index, generator counter); `word` names the draw domain.
__device__ __forceinline__ int d3pm_categorical(const float *l, int Kc, int lane, size_t e0, bool t0, float at, float ap_, int xt,
                                                const float *noise, const uint64_t *seed, uint32_t iteration, uint32_t word,
                                                float *post) {
    float lf_hit = 0.f, lf_miss = 0.f, ap = 1.f, c2 = 0.f, m = 0.f, inv_s = 0.f;
    if (!t0) {
        ap = ap_;
        const float rr = at / ap, miss = ((ap - at) / ap) / (float)Kc;        // (1 - r) / K without the cancellation of 1 - r
        lf_hit = logf(rr + miss + 1e-8f);
        lf_miss = logf(miss + 1e-8f);
        c2 = (1.0f - ap) / (float)Kc;
        m = -FLT_MAX;
        for (int k = lane; k < Kc; k += 64) m = fmaxf(m, l[k]);
        m = wave_max(m);
        float s = 0.f;
        for (int k = lane; k < Kc; k += 64) s += expf(l[k] - m);
        s = wave_sum(s);
        inv_s = 1.0f / s;
    }
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < Kc; k += 64) {
        float v = l[k];
        if (!t0) {
            const float pi = expf(v - m) * inv_s;
            v = (k == xt ? lf_hit : lf_miss) + logf(fmaf(ap, pi, c2) + 1e-8f);
        }
        if (post) post[e0 + k] = v;
        if (!t0) {
            const size_t e = e0 + k;
            v += gumbel(noise ? noise[e] : philox_uniform(seed[0], (uint64_t)e + seed[1], iteration, word));
        }
        if (v > best) { best = v; bi = k; }                                // ascending k per lane: the first maximum stays
    }
    return wave_argmax_first(best, bi);
}

// ------------------------------------------------------------------------------------------ loss row + d loss / d logits
// One wave, one piece; the row's logits z and a second K-wide image mh (m, then h) sit in LDS, each word private to the lane that owns
// column k.  With pi = softmax(z) and y = (1 - smooth) e_x0 + smooth / K (smooth == 0: the plain cross entropy):
//   ce_row = -sum_k y[k] log pi[k],                                           d / dz = pi - y
//   t == 0: vb_row = -log pi[x0] / ln 2,                                      d / dz = (pi - e_x0) / ln 2
//   t  > 0: m[k] = lf[k] + log(a_p pi[k] + c2 + eps), lf[k] = log(r [k == x_t] + c1 + eps)        (two values)
//           q~[k] = lf[k] + log(a_p [k == x0] + c2 + eps)                                          (at most four values: the classes
//                   (k == x_t, k == x0) = both | x_t only | x0 only | neither, with 1 | 1 | 1 | K - 1 or K - 2 members)
//           vb_row = sum_k q[k] (log q[k] - log_softmax(m)[k]) / ln 2
//           g[k] = (softmax(m)[k] - q[k]) / ln 2, h[k] = g[k] a_p / (a_p pi[k] + c2 + eps), d / dz[j] = pi[j] (h[j] - sum_k pi[k] h[k])
// Both softmaxes are max-subtracted.  dz = (w_vb d vb_row + w_ce d ce_row) * inv_n.  x0: clamped to [0, K); x_t: the piece's
// noisy index, read (and clamped) only where t > 0; ti: clamped t.
__device__ __forceinline__ void d3pm_loss_row(float *z, float *mh, int K, int lane, const float *__restrict__ zr, float *__restrict__ dz,
                                              int x0, const int32_t *__restrict__ x_t, int64_t ti, const float *__restrict__ alphas_cumprod,
                                              int want_vb, float w_vb, float w_ce, float smooth, float inv_n, float &vb_row,
                                              float &ce_row) {
    const float inv_ln2 = 1.4426950408889634f;
    float zmax = -FLT_MAX;
    for (int k = lane; k < K; k += 64) { const float v = zr[k]; z[k] = v; zmax = fmaxf(zmax, v); }
    zmax = wave_max(zmax);
    float se = 0.f, sz = 0.f;
    for (int k = lane; k < K; k += 64) { const float d = z[k] - zmax; se += expf(d); sz += d; }
    se = wave_sum(se);
    sz = wave_sum(sz);                                               // sum_k (z[k] - zmax)
    const float lse = logf(se), inv_se = 1.0f / se;
    // log pi[x0]: read by the lane that wrote z[x0] and handed round
    const float lp_x0 = __shfl((x0 & 63) == lane ? z[x0] : 0.f, x0 & 63, 64) - zmax - lse;
    const float y_miss = smooth / (float)K, y_hit = (1.0f - smooth) + y_miss;
    ce_row = smooth > 0.f ? -((1.0f - smooth) * lp_x0 + y_miss * (sz - (float)K * lse)) : -lp_x0;
    vb_row = 0.f;
    if (!want_vb || ti == 0) {
        // cross entropy alone, or the decoder NLL of t == 0: both gradients are pi minus a constant pattern
        if (want_vb) vb_row = -lp_x0 * inv_ln2;
        const float wv0 = want_vb ? w_vb * inv_ln2 : 0.f;
        for (int k = lane; k < K; k += 64) {
            const float pi = expf(z[k] - zmax) * inv_se;
            dz[k] = (wv0 * (pi - (k == x0 ? 1.f : 0.f)) + w_ce * (pi - (k == x0 ? y_hit : y_miss))) * inv_n;
        }
        return;
    }
    const int xt = clamp_idx(*x_t, K);
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

}  // namespace da
