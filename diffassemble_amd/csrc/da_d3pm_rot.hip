// Discrete position + rotation diffusion (spatial_diffusion_discrete_rot.py over backbones/efficient_gat_discrete_rotation.py): what
// differs from the position model of da_d3pm.hip.
//   * the embedding: the lookup (pos_emb[idx] | time_emb[t]; the position model's too, with proj4 == NULL) plus the ADDEND-ROW
//     SELECT.  The reference rotates every crop by its accumulated rotation rot_acc and re-encodes it each step (:353, :373); rot_acc
//     takes four values, so the hoisted feature share of mlp.0 exists as four images per Batch (da_denoiser_set_features_rot) and a
//     step only copies row rot_acc[piece] of them into the `pre` operand of the K = 64 mlp.0 product -- in the launch that gathers
//     pos_mlp / time_emb anyway;
//   * the tail: two heads (K-wide and 4-wide) over the [n, 64] post-GELU rows of final_mlp.0 | final_mlp_rot.0, two categorical
//     posteriors of the uniform transition (d3pm_categorical of da_d3pm_common.h, the copy k_d3pm_tail runs too, with K and with 4),
//     and the loop's state update.
#include "da_common.h"
#include "da_d3pm_common.h"
#include "da_internal.h"

namespace da {

// ------------------------------------------------------------------------------------------
// comb_in[r, F:F+32] = pos_emb[idx[r]] ; comb_in[r, F+32:F+64] = time_emb[t[r]]   (efficient_gat_discrete.py:81-86)
// 64 consecutive threads per node: thread c writes comb_in[r, F + c] and, with proj4, copies elements c, c + 64, ... of the selected
// projection row.  rot_acc is taken mod 4 (it is one by construction); idx / t are clamped (k_embed_pos_time clamps t the same way).
template <typename T>
__global__ __launch_bounds__(256) void k_embed_idx_time_rot(int n, int K, int F, int D, int hidden, const int32_t *__restrict__ idx,
                                                            const int32_t *__restrict__ rot_acc, const int64_t *__restrict__ t,
                                                            int64_t t_scalar, int steps, const float *__restrict__ time_emb,
                                                            const float *__restrict__ pos_emb, T *__restrict__ comb_in,
                                                            const T *__restrict__ proj4, size_t img_stride, T *__restrict__ sel) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * 64) return;
    const size_t r = e >> 6;
    const int c = (int)(e & 63);
    float v;
    if (c < 32)
        v = pos_emb[(size_t)clamp_idx(idx[r], K) * 32 + c];
    else
        v = time_emb[clamp_t(t ? t[r] : t_scalar, steps) * 32 + (c - 32)];
    stf(comb_in + r * D + F + c, v);
    if (!proj4) return;
    const int img = rot_acc ? (rot_acc[r] & 3) : 0;
    const T *src = proj4 + (size_t)img * img_stride + r * hidden;
    for (int q = c; q < hidden; q += 64) sel[r * hidden + q] = src[q];
}

// ------------------------------------------------------------------------------------------
// The tail.  A workgroup of four waves owns D3PM_ROT_ROWS consecutive nodes.
//   phase 1  the nodes' [., 64] post-GELU rows staged in LDS (columns 0..31 final_mlp.0, 32..63 final_mlp_rot.0); thread k (k, k + 256,
//            ... < K) keeps row k of final_mlp.2 in registers and forms logits[j][k] as k_d3pm_tail does; threads 0..31 form the
//            8 x 4 rotation logits.  Both go to LDS, and to HBM only when asked.  da_d3pm_rot_step starts from given logits instead.
//   phase 2  one wave per node: the position posterior + Gumbel + argmax, rot_0 = first-index argmax of the four raw rotation logits,
//            the rotation posterior + Gumbel + argmax (rot_prev; skipped with its draws when nobody reads it), and the loop's state
//            update  rot_next = cold ? rot_prev : rot_0,  rot_acc_out = (rot_acc_in + rot_next) % 4.
// fp32 throughout; any K in [2, 1024]; no per-lane arrays (the logits live in LDS).
constexpr int D3PM_ROT_ROWS = 8;

template <typename T>
__global__ __launch_bounds__(256) void k_d3pm_rot_tail(int n, int K, const T *__restrict__ hh, const float *__restrict__ w2,
                                                       const float *__restrict__ b2, const float *__restrict__ wr,
                                                       const float *__restrict__ br, const float *__restrict__ logits_in,
                                                       const float *__restrict__ rot_logits_in, float *__restrict__ logits_out,
                                                       float *__restrict__ rot_logits_out, int do_step, D3pmRotStep sp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *hs = lds, *rl = lds + D3PM_ROT_ROWS * 64, *lg = rl + D3PM_ROT_ROWS * 4;          // hs [8][64], rl [8][4], lg [8][K]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row0 = blockIdx.x * D3PM_ROT_ROWS;
    const int rows = n - row0 < D3PM_ROT_ROWS ? n - row0 : D3PM_ROT_ROWS;
    if (logits_in) {
        for (int e = tid; e < rows * K; e += 256) lg[e] = logits_in[(size_t)row0 * K + e];
        if (tid < rows * 4) rl[tid] = rot_logits_in[(size_t)row0 * 4 + tid];
    } else {
        for (int e = tid; e < D3PM_ROT_ROWS * 64; e += 256) hs[e] = (e >> 6) < rows ? ldf(hh + (size_t)row0 * 64 + e) : 0.f;
        __syncthreads();
        if (tid < rows * 4) {
            const int j = tid >> 2, c = tid & 3;
            float a = br[c];
#pragma unroll
            for (int q = 0; q < 32; ++q) a = fmaf(wr[c * 32 + q], hs[j * 64 + 32 + q], a);
            rl[tid] = a;
            if (rot_logits_out) rot_logits_out[(size_t)row0 * 4 + tid] = a;
        }
        for (int k = tid; k < K; k += 256) {
            float wk[32];
            const float4 *wp = (const float4 *)(w2 + (size_t)k * 32);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = wp[q];
                wk[4 * q] = v.x; wk[4 * q + 1] = v.y; wk[4 * q + 2] = v.z; wk[4 * q + 3] = v.w;
            }
            const float bias = b2[k];
            for (int j = 0; j < rows; ++j) {
                float a = bias;
#pragma unroll
                for (int q = 0; q < 32; ++q) a = fmaf(wk[q], hs[j * 64 + q], a);
                lg[j * K + k] = a;
                if (logits_out) logits_out[(size_t)(row0 + j) * K + k] = a;
            }
        }
    }
    if (!do_step) return;
    __syncthreads();
    for (int j = wv; j < rows; j += 4) {
        const int r = row0 + j;
        float at, ap;
        const bool t0 = d3pm_step_alphas(sp.s, sp.t, sp.t_scalar, sp.ratio, r, at, ap);
        const int xp = d3pm_categorical(lg + j * K, K, lane, (size_t)r * K, t0, at, ap, t0 ? 0 : sp.x_t[r], sp.noise_x, sp.seed,
                                        (uint32_t)sp.iteration, D3PM_WORD_SAMPLING, sp.post_x);
        const float *q = rl + j * 4;
        int r0 = 0;
        float rb = q[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (q[k] > rb) { rb = q[k]; r0 = k; }
        int rp = r0;
        if (sp.need_prev)
            rp = d3pm_categorical(q, 4, lane, (size_t)r * 4, t0, at, ap, t0 ? 0 : (sp.rot_t[r] & 3), sp.noise_rot, sp.seed,
                                  (uint32_t)sp.iteration, D3PM_WORD_SAMPLING_ROT, sp.post_rot);
        if (lane == 0) {
            sp.x_prev[r] = xp;
            if (sp.rot_0) sp.rot_0[r] = r0;
            if (sp.rot_prev) sp.rot_prev[r] = rp;
            if (sp.rot_acc_out) {
                const int nx = sp.cold ? rp : r0;
                const int acc = sp.rot_acc_in ? sp.rot_acc_in[r] : 0;
                if (sp.rot_next) sp.rot_next[r] = nx;
                sp.rot_acc_out[r] = (acc + nx) & 3;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ launchers
int launch_embed_idx_time_rot(int prec, int n, int K, int F, int D, int hidden, const int32_t *idx, const int32_t *rot_acc, const int64_t *t,
                              int64_t t_scalar, int steps, const float *time_emb, const float *pos_emb, void *comb_in, const void *proj4,
                              size_t img_stride, void *sel, hipStream_t st) {
    if (n <= 0) return 0;
    const unsigned grid = (unsigned)(((size_t)n * 64 + 255) / 256);
    if (prec == DA_PREC_BF16)
        k_embed_idx_time_rot<bf16_t><<<grid, 256, 0, st>>>(n, K, F, D, hidden, idx, rot_acc, t, t_scalar, steps, time_emb, pos_emb,
                                                           (bf16_t *)comb_in, (const bf16_t *)proj4, img_stride, (bf16_t *)sel);
    else
        k_embed_idx_time_rot<float><<<grid, 256, 0, st>>>(n, K, F, D, hidden, idx, rot_acc, t, t_scalar, steps, time_emb, pos_emb,
                                                          (float *)comb_in, (const float *)proj4, img_stride, (float *)sel);
    DA_LAUNCH_CHECK();
    return 0;
}

int launch_d3pm_rot_tail(int prec, int n, int K, const void *hh, const float *w2, const float *b2, const float *wr, const float *br,
                         const float *logits_in, const float *rot_logits_in, float *logits_out, float *rot_logits_out,
                         const D3pmRotStep *step, hipStream_t st) {
    if (n <= 0) return 0;
    if (K < 2 || K > 1024) { set_error("d3pm rot: K = %d outside [2, 1024]", K); return 1; }
    if (logits_in ? !rot_logits_in : !(hh && w2 && b2 && wr && br)) { set_error("d3pm rot tail: neither both logits nor head rows given"); return 1; }
    const D3pmRotStep sp = step ? *step : D3pmRotStep();
    const unsigned grid = (unsigned)((n + D3PM_ROT_ROWS - 1) / D3PM_ROT_ROWS);
    const size_t lds = (size_t)(D3PM_ROT_ROWS * (64 + 4 + K)) * sizeof(float);            // <= 35 KiB at K = 1024
    if (prec == DA_PREC_BF16)
        k_d3pm_rot_tail<bf16_t><<<grid, 256, lds, st>>>(n, K, (const bf16_t *)hh, w2, b2, wr, br, logits_in, rot_logits_in, logits_out,
                                                        rot_logits_out, step ? 1 : 0, sp);
    else
        k_d3pm_rot_tail<float><<<grid, 256, lds, st>>>(n, K, (const float *)hh, w2, b2, wr, br, logits_in, rot_logits_in, logits_out,
                                                       rot_logits_out, step ? 1 : 0, sp);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

using namespace da;

extern "C" {

int da_d3pm_rot_step(const da_schedule *s, int n, int K, const int32_t *x_t, const int32_t *rot_t, const float *logits,
                     const float *rot_logits, const int64_t *t, int64_t t_scalar, int inference_ratio, const float *noise_x,
                     const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_prev, int32_t *rot_0, int32_t *rot_prev,
                     float *post_x, float *post_rot, void *stream) {
    DA_REQUIRE(s && x_t && rot_t && logits && rot_logits && x_prev, "da_d3pm_rot_step: null argument");
    DA_REQUIRE(n >= 0 && K >= 2 && K <= 1024, "da_d3pm_rot_step: K = %d outside [2, 1024]", K);
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1 && s->alphas_cumprod, "da_d3pm_rot_step: bad ratio / schedule");
    DA_REQUIRE(t || !(t_scalar > 0 && t_scalar < inference_ratio), "da_d3pm_rot_step: t = %lld lies in (0, ratio = %d): t - ratio < 0 has no posterior",
               (long long)t_scalar, inference_ratio);
    const bool need_prev = rot_prev || post_rot;
    DA_REQUIRE((noise_x && (noise_rot || !need_prev)) || seed || (!t && t_scalar <= 0), "da_d3pm_rot_step: needs the uniforms (noise_x, noise_rot) or a seed");
    D3pmRotStep sp;
    sp.s = to_dev(s);
    sp.x_t = x_t; sp.rot_t = rot_t; sp.t = t; sp.t_scalar = t_scalar; sp.ratio = inference_ratio; sp.noise_x = noise_x; sp.noise_rot = noise_rot;
    sp.seed = seed; sp.iteration = iteration; sp.x_prev = x_prev; sp.rot_0 = rot_0; sp.rot_prev = rot_prev; sp.post_x = post_x; sp.post_rot = post_rot;
    sp.need_prev = need_prev ? 1 : 0;
    return launch_d3pm_rot_tail(DA_PREC_F32, n, K, nullptr, nullptr, nullptr, nullptr, nullptr, logits, rot_logits, nullptr, nullptr, &sp,
                                (hipStream_t)stream);
}

}  // extern "C"
