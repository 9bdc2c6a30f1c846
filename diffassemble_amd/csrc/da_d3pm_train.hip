// Training side of the discrete (D3PM, uniform transition) position diffusion: the forward noising q_sample, the loss of p_losses
// (variational bound, label-smoothed cross entropy, their hybrid) with its gradient with respect to the logits, and the gradient of
// the position-embedding lookup (spatial_diffusion_discrete.py:181-191, 229-273, 416-488; efficient_gat_discrete.py:81-86).
//
// As in da_d3pm.hip no [steps, K, K] table exists: overline_Q[t] = a_t I + (1 - a_t) / K 11^T and
// overline_Q[t] overline_Q[t - 1]^-1 = r I + (1 - r) / K 11^T with r = a_t / a_{t-1}, so every row needs a handful of scalars.
// The noising and the loss are K-wide per-piece work, one wave per piece, fp32, any K in [2, 1024]; their row routines (q_sample_row,
// d3pm_loss_row) live in da_d3pm_common.h, the one copy the position + rotation model (da_d3pm_rot_train.hip) runs too, and the noising
// kernel here serves both models.  The embedding gradient has one workgroup per table row.
#include "da_common.h"
#include "da_d3pm_common.h"
#include "da_internal.h"

namespace da {

constexpr int D3T_ROWS = 4;                       // pieces per workgroup = waves per workgroup

// ------------------------------------------------------------------------------------------ q_sample
// One wave per piece: the K-wide position draw (skipped when x_noisy == NULL: only_rotation), then the four-wide rotation draw on
// lanes 0..3 of the same wave (skipped when rot_noisy == NULL: the position model).  The uniforms are given or drawn here by the
// shared generator: the position half in the TRAINING domain, the rotation half in TRAINING_ROT, flat element r * 4 + k.
__global__ __launch_bounds__(64 * D3T_ROWS) void k_d3pm_q_sample(int n, int K, int steps, const float *__restrict__ alphas_cumprod,
                                                                 const int32_t *__restrict__ x_start, const int32_t *__restrict__ rot_start,
                                                                 const int64_t *__restrict__ t, const float *__restrict__ noise_x,
                                                                 const float *__restrict__ noise_rot, const uint64_t *__restrict__ seed,
                                                                 uint32_t iteration, int32_t *__restrict__ x_noisy,
                                                                 int32_t *__restrict__ rot_noisy) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * D3T_ROWS + (threadIdx.x >> 6);
    if (r >= n) return;
    const float at = alphas_cumprod[clamp_t(t[r], steps)];
    if (x_noisy) {
        const int xn = q_sample_row(K, lane, (size_t)r * K, at, clamp_idx(x_start[r], K), noise_x, seed, iteration, D3PM_WORD_TRAINING);
        if (lane == 0) x_noisy[r] = xn;
    }
    if (rot_noisy) {
        const int rn = q_sample_row(4, lane, (size_t)r * 4, at, rot_start[r] & 3, noise_rot, seed, iteration, D3PM_WORD_TRAINING_ROT);
        if (lane == 0) rot_noisy[r] = rn;
    }
}

int launch_d3pm_q_sample(int n, int K, const da_schedule *s, const int32_t *x_start, const int32_t *rot_start, const int64_t *t,
                         const float *noise_x, const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_noisy,
                         int32_t *rot_noisy, hipStream_t st) {
    if (n == 0) return 0;
    k_d3pm_q_sample<<<(unsigned)((n + D3T_ROWS - 1) / D3T_ROWS), 64 * D3T_ROWS, 0, st>>>(
        n, K, s->steps, s->alphas_cumprod, x_start, rot_start, t, noise_x, noise_rot, seed, (uint32_t)iteration, x_noisy, rot_noisy);
    DA_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ loss + d loss / d logits
// One wave per piece runs d3pm_loss_row over its two K-wide LDS images; the cross entropy is label-smoothed (0.01) in every kind.
// d_logits = (w_vb d vb_row + w_ce d ce_row) / n; the row terms go to row_terms [n, 2] and k_d3pm_loss_finish sums them in a fixed order.
__global__ __launch_bounds__(64 * D3T_ROWS) void k_d3pm_loss(int n, int K, int steps, const float *__restrict__ alphas_cumprod, int want_vb,
                                                             float w_vb, float w_ce, const float *__restrict__ logits,
                                                             const int32_t *__restrict__ x_start, const int32_t *__restrict__ x_t,
                                                             const int64_t *__restrict__ t, float *__restrict__ d_logits,
                                                             float *__restrict__ row_terms) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = blockIdx.x * D3T_ROWS + wv;
    if (r >= n) return;                                              // (no workgroup barrier below: a wave owns its LDS rows)
    float *z = lds + (size_t)wv * 2 * K;
    float vb_row, ce_row;
    d3pm_loss_row(z, z + K, K, lane, logits + (size_t)r * K, d_logits + (size_t)r * K, clamp_idx(x_start[r], K), x_t + r,
                  clamp_t(t[r], steps), alphas_cumprod, want_vb, w_vb, w_ce, 0.01f, 1.0f / (float)n, vb_row, ce_row);
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
    return launch_d3pm_q_sample(n, K, s, x_start, nullptr, t, noise, nullptr, seed, iteration, x_noisy, nullptr, (hipStream_t)stream);
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
