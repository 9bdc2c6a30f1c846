// Discrete (D3PM, uniform transition) position diffusion: the two ends of the step that differ from the continuous 2D model
// (spatial_diffusion_discrete.py, backbones/efficient_gat_discrete.py) -- the embedding LOOKUP where the pose MLP was, and the
// tail: the K-wide logits head, classifier-free guidance, softmax, the categorical posterior, the Gumbel term and the argmax.
//
// The reference keeps three [steps, K, K] fp32 tables and inverts a [N, K, K] batch per sampling step.  For the uniform kernel
// Q_t = (1 - b_t) I + b_t / K 11^T every product of such matrices is again of that form: overline_Q[t] = a_t I + (1 - a_t) / K 11^T
// with a_t = alphas_cumprod[t], and overline_Q[t] overline_Q[p]^-1 = r I + (1 - r) / K 11^T with r = a_t / a_p.  The step below
// therefore needs two scalars per node and no K x K object.  The embedding lookup is the position + rotation model's
// kernel without its addend rows (da_d3pm_rot.hip).
#include "da_common.h"
#include "da_d3pm_common.h"
#include "da_internal.h"

namespace da {

// ------------------------------------------------------------------------------------------
// (philox_uniform: da_internal.h, shared with the training-side noising of da_d3pm_train.hip)
__global__ __launch_bounds__(256) void k_d3pm_noise(const uint64_t *__restrict__ seed, uint32_t iteration, uint32_t domain, size_t total,
                                                    float *__restrict__ u) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) u[e] = philox_uniform(seed[0], (uint64_t)e + seed[1], iteration, domain);
}

// ------------------------------------------------------------------------------------------
// The tail.  A workgroup of four waves owns D3PM_ROWS consecutive nodes.
//   phase 1  thread k (k, k + 256, ... < K) keeps row k of final_mlp.2 in registers and applies it to the workgroup's post-GELU
//            rows hh [., 32] (staged in LDS, broadcast reads; with the last-layer fold they are formed here from the per-head
//            attention outputs, D3pmRows): logits[j][k] into LDS, and to HBM only when asked.  Under guidance
//            both passes' rows are multiplied and combined as (1 + w) cond - w uncond, each product rounded on its own, i.e. the
//            values the two-forward eager path forms.  da_d3pm_step starts from given logits instead (logits_in).
//   phase 2  one wave per node: d3pm_categorical (da_d3pm_common.h, the one copy both discrete models run) -- the posterior, the
//            Gumbel term and a first-index argmax.  t == 0: argmax of the logits.
// fp32 throughout; any K in [2, 1024]; no per-lane arrays (the K values live in LDS).
constexpr int D3PM_ROWS = 8;

static_assert(D3PM_ROWS * 32 == 256, "phase 1 stages one hh element per thread");

template <typename T>
__device__ __forceinline__ float d3pm_row_value(const D3pmRows &rw, int n, int H, int r, int c) {
    if (rw.hh) return ldf((const T *)rw.hh + (size_t)r * 32 + c);
    float a = ldf((const T *)rw.pre + (size_t)r * 32 + c);                 // pre, then heads 0 .. H-1: k_head_fold's order
    for (int h = 0; h < H; ++h) a += ldf((const T *)rw.pz + ((size_t)h * n + r) * 32 + c);
    return gelu_erf(a);
}

template <typename T>
__global__ __launch_bounds__(256) void k_d3pm_tail(int n, int K, int H, D3pmRows rows_c, D3pmRows rows_u, int guided, float w_cfg,
                                                   const float *__restrict__ w2, const float *__restrict__ b2,
                                                   const float *__restrict__ logits_in, float *__restrict__ logits_out,
                                                   int do_step, D3pmStep sp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *hs_c = lds, *hs_u = lds + D3PM_ROWS * 32, *lg = lds + 2 * D3PM_ROWS * 32;          // lg [D3PM_ROWS][K]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row0 = blockIdx.x * D3PM_ROWS;
    const int rows = n - row0 < D3PM_ROWS ? n - row0 : D3PM_ROWS;
    if (logits_in) {
        for (int e = tid; e < rows * K; e += 256) lg[e] = logits_in[(size_t)row0 * K + e];
    } else {
        {
            const int j = tid >> 5, c = tid & 31;                                           // 256 threads = 8 rows x 32
            const bool ok = j < rows;
            hs_c[tid] = ok ? d3pm_row_value<T>(rows_c, n, H, row0 + j, c) : 0.f;
            hs_u[tid] = (ok && guided) ? d3pm_row_value<T>(rows_u, n, H, row0 + j, c) : 0.f;
        }
        __syncthreads();
        const float w1p = (float)(1.0 + (double)w_cfg);
        for (int k = tid; k < K; k += 256) {
            float wr[32];
            const float4 *wp = (const float4 *)(w2 + (size_t)k * 32);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = wp[q];
                wr[4 * q] = v.x; wr[4 * q + 1] = v.y; wr[4 * q + 2] = v.z; wr[4 * q + 3] = v.w;
            }
            const float bias = b2[k];
            for (int j = 0; j < rows; ++j) {
                float a = bias;
#pragma unroll
                for (int q = 0; q < 32; ++q) a = fmaf(wr[q], hs_c[j * 32 + q], a);
                if (guided) {
                    float b = bias;
#pragma unroll
                    for (int q = 0; q < 32; ++q) b = fmaf(wr[q], hs_u[j * 32 + q], b);
                    a = __fsub_rn(__fmul_rn(w1p, a), __fmul_rn(w_cfg, b));                  // (1 + w) cond - w uncond, three roundings
                }
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
        const int xp = d3pm_categorical(lg + j * K, K, lane, (size_t)r * K, t0, at, ap, t0 ? 0 : sp.x_t[r], sp.noise, sp.seed,
                                        (uint32_t)sp.iteration, D3PM_WORD_SAMPLING, sp.post);
        if (lane == 0) sp.x_prev[r] = xp;
    }
}

// ------------------------------------------------------------------------------------------ launchers
int launch_embed_idx_time(int prec, int n, int K, int F, int D, const int32_t *idx, const int64_t *t, int64_t t_scalar, int steps,
                          const float *time_emb, const float *pos_emb, void *comb_in, hipStream_t st) {
    return launch_embed_idx_time_rot(prec, n, K, F, D, 0, idx, nullptr, t, t_scalar, steps, time_emb, pos_emb, comb_in, nullptr, 0, nullptr,
                                     st);
}

int launch_d3pm_tail(int prec, int n, int K, int H, const D3pmRows *rows_c, const D3pmRows *rows_u, float cfg_w, const float *w2,
                     const float *b2, const float *logits_in, float *logits_out, const D3pmStep *step, hipStream_t st) {
    if (n <= 0) return 0;
    if (K < 2 || K > 1024) { set_error("d3pm: K = %d outside [2, 1024]", K); return 1; }
    const D3pmStep sp = step ? *step : D3pmStep();
    const D3pmRows rc = rows_c ? *rows_c : D3pmRows(), ru = rows_u ? *rows_u : D3pmRows();
    if (!logits_in && !rc.hh && !(rc.pz && rc.pre)) { set_error("d3pm tail: neither logits nor head rows given"); return 1; }
    const unsigned grid = (unsigned)((n + D3PM_ROWS - 1) / D3PM_ROWS);
    const size_t lds = (size_t)(2 * D3PM_ROWS * 32 + D3PM_ROWS * K) * sizeof(float);          // <= 34 KiB at K = 1024
    if (prec == DA_PREC_BF16)
        k_d3pm_tail<bf16_t><<<grid, 256, lds, st>>>(n, K, H, rc, ru, rows_u ? 1 : 0, cfg_w, w2, b2, logits_in, logits_out, step ? 1 : 0, sp);
    else
        k_d3pm_tail<float><<<grid, 256, lds, st>>>(n, K, H, rc, ru, rows_u ? 1 : 0, cfg_w, w2, b2, logits_in, logits_out, step ? 1 : 0, sp);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

using namespace da;

extern "C" {

int da_d3pm_step(const da_schedule *s, int n, int K, const int32_t *x_t, const float *logits, const int64_t *t, int64_t t_scalar,
                 int inference_ratio, const float *noise, const uint64_t *seed, int iteration, int32_t *x_prev, float *post,
                 void *stream) {
    DA_REQUIRE(s && x_t && logits && x_prev, "da_d3pm_step: null argument");
    DA_REQUIRE(n >= 0 && K >= 2 && K <= 1024, "da_d3pm_step: K = %d outside [2, 1024]", K);
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1 && s->alphas_cumprod, "da_d3pm_step: bad ratio / schedule");
    DA_REQUIRE(t || !(t_scalar > 0 && t_scalar < inference_ratio), "da_d3pm_step: t = %lld lies in (0, ratio = %d): t - ratio < 0 has no posterior",
               (long long)t_scalar, inference_ratio);
    DA_REQUIRE(noise || seed || (!t && t_scalar <= 0), "da_d3pm_step: needs the uniforms (noise) or a seed");
    D3pmStep sp;
    sp.s = to_dev(s);
    sp.x_t = x_t; sp.t = t; sp.t_scalar = t_scalar; sp.ratio = inference_ratio; sp.noise = noise; sp.seed = seed; sp.iteration = iteration;
    sp.x_prev = x_prev; sp.post = post;
    return launch_d3pm_tail(DA_PREC_F32, n, K, 0, nullptr, nullptr, 0.f, nullptr, nullptr, logits, nullptr, &sp, (hipStream_t)stream);
}

int da_d3pm_noise(const uint64_t *seed, int iteration, int n, int K, float *u, void *stream) {
    return da_d3pm_noise_ex(seed, iteration, n, K, DA_D3PM_DRAW_SAMPLING, u, stream);
}

int da_d3pm_noise_ex(const uint64_t *seed, int iteration, int n, int K, int domain, float *u, void *stream) {
    DA_REQUIRE(seed && u && n >= 0 && K >= 1, "da_d3pm_noise: bad argument");
    DA_REQUIRE(domain == DA_D3PM_DRAW_SAMPLING || domain == DA_D3PM_DRAW_TRAINING || domain == DA_D3PM_DRAW_SAMPLING_ROT ||
                   domain == DA_D3PM_DRAW_TRAINING_ROT, "da_d3pm_noise: unknown draw domain %d", domain);
    const size_t total = (size_t)n * K;
    if (!total) return 0;
    k_d3pm_noise<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(seed, (uint32_t)iteration, d3pm_domain_word(domain), total, u);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
