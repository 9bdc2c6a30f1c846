// Fused Adafactor step for ANY list of fp32 tensors of any rank, addressed by pointer (da_adafactor_nd_step).
//
// Replaces, for every trainable tensor outside the training engine's flat buffer (the piece encoder's 5-D group-convolution
// banks, its BatchNorm affines, linear1 [544, 16384] / linear2 [544, 8192]; the VN-DGCNN fragment encoder's parameters),
// transformers.optimization.Adafactor as the reference configures it (spatial_diffusion.py:701-705: relative step,
// scale_parameter, eps = (1e-30, 1e-3), clip_threshold 1, decay_rate -0.8, no first moment, no weight decay).  da_optim.hip
// covers the flat buffer's vectors and matrices of at most 1280 columns; here a tensor [..., R, C] is B = prod(shape[:-2])
// independent [R, C] slices for the second moment, exactly as transformers' _approx_sq_grad treats it:
//   t = step + 1 (PER TENSOR, a device counter),  beta = 1 - t^decay,  rho = min(1e-2, 1/sqrt(t)),  lr = max(eps2, rms(p)) * rho
//   row[b, r] <- beta row + (1-beta) mean_c(g^2 + eps1),   col[b, c] <- beta col + (1-beta) mean_r(g^2 + eps1)
//   u = g * (rsqrt(row[b, r] / mean_r(row[b, :])) * rsqrt(col[b, c]))          rank <= 1:  v <- beta v + (1-beta)(g^2 + eps1),  u = g rsqrt(v)
//   p <- p - lr * u / max(1, rms(u) / clip)            rms(p), rms(u): over the WHOLE tensor
// Three kinds of tensor, one block table:
//   kind 0  vectors: blocks of 4096 elements (as da_optim.hip)
//   kind 1  many tiny slices (R C <= 64: 3x3, 1x1, 1xk, kx1): ONE LANE owns a slice, 256 consecutive slices per block, so a wave's loads
//           cover 64 consecutive slices; row / col sums never leave the lane, u^2 is summed in phase A already
//   kind 2  everything else, any width: tiles of 16 rows x 1024 columns; a tile writes its partial row sums (per column chunk) and partial
//           column sums (per row block), phase B adds them in ascending order
// FOUR launches whatever the number of tensors; every reduction is two-stage in a fixed order (no atomics: two runs, and two data-parallel
// ranks, apply identical bits); nothing returns to the host.  A tensor whose `active` flag is 0 (no gradient this step) is skipped and
// keeps its step count.
#include <math.h>

#include "da_common.h"

namespace da {

struct NdParam {                          // one record per tensor (device table, 80 bytes)
    float *p;
    const float *g;
    long long row_off, col_off;           // state buffer: row[B][R], col[B][C]; kind 0: v[numel] at row_off
    long long colpart_off, rowpart_off;   // kind 2 scratch: colpart[B][nrb][C], rowpart[B][ncb][R]
    int B, R, C, kind;                    // kind 0: B = R = 1, C = numel
    int blk0, nblk, active, rmean_off;    // its blocks in the block table; kind 2: rmean[rmean_off + b] = mean_r(row[b, :])
};
struct NdBlock { int pid, b, r0, nr, c0, nc; };   // kind 0: nr elements from r0; kind 1: nr slices from slice r0; kind 2: tile of slice b
struct NdJob { int pid, b, c0; };                 // phase B: c0 < 0 = the rows of slice b (b == 0: also the tensor's lr); else 64 columns from c0
// (the host's table builder uses the same numbers: ND_* of diffassemble_amd/train.py, compared by tests/test_adafactor_nd_host.py)
constexpr int ND_TR = 16, ND_TC = 1024, ND_VEC = 4096, ND_BCH = 64, ND_TINY = 64, ND_SPB = 256;   // ND_SPB slices per block = its 256 lanes
constexpr int ND_CPL = ND_TC / 64;

__device__ __forceinline__ float nd_block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// transformers computes the factors with torch's rsqrt / true division: correctly rounded 1 / sqrt here, not the hardware's approximation
__device__ __forceinline__ float nd_rsq(float x) { return 1.0f / sqrtf(x); }
// beta2t of this step from the tensor's own counter, in double as math.pow does (t = 1 gives exactly 0)
__device__ __forceinline__ void nd_beta(int t, float decay, float &beta, float &omb) {
    const double b = 1.0 - exp((double)decay * log((double)t));
    beta = (float)b;
    omb = (float)(1.0 - b);
}

// one lane, one [R, C] slice: row / col EMAs (final), then this slice's u^2.  RT / CT > 0: compile-time extents (the 3x3 filters)
template <int RT, int CT>
__device__ __forceinline__ void nd_tiny_a(const NdParam &p, size_t s, float beta, float omb, float eps1, float *state, float &sp, float &su) {
    const int R = RT ? RT : p.R, C = CT ? CT : p.C;
    const float *g = p.g + s * (size_t)(R * C), *w = p.p + s * (size_t)(R * C);
    float *row = state + p.row_off + s * R, *col = state + p.col_off + s * C;
    float rsum = 0.f;
    for (int r = 0; r < R; ++r) {
        float sr = 0.f;
        for (int c = 0; c < C; ++c) {
            const float gv = g[r * C + c], wv = w[r * C + c];
            sr += fmaf(gv, gv, eps1);
            sp = fmaf(wv, wv, sp);
        }
        const float rv = beta * row[r] + omb * (sr / (float)C);
        row[r] = rv;
        rsum += rv;
    }
    const float rmean = rsum / (float)R;
    for (int c = 0; c < C; ++c) {
        float sc = 0.f;
        for (int r = 0; r < R; ++r) { const float gv = g[r * C + c]; sc += fmaf(gv, gv, eps1); }
        const float cv = beta * col[c] + omb * (sc / (float)R);
        col[c] = cv;
        const float cf = nd_rsq(cv);
        for (int r = 0; r < R; ++r) {
            const float u = g[r * C + c] * (nd_rsq(row[r] / rmean) * cf);
            su = fmaf(u, u, su);
        }
    }
}
template <int RT, int CT>
__device__ __forceinline__ void nd_tiny_d(const NdParam &p, size_t s, float step, const float *state) {
    const int R = RT ? RT : p.R, C = CT ? CT : p.C;
    const float *g = p.g + s * (size_t)(R * C);
    float *w = p.p + s * (size_t)(R * C);
    const float *row = state + p.row_off + s * R, *col = state + p.col_off + s * C;
    float rsum = 0.f;
    for (int r = 0; r < R; ++r) rsum += row[r];
    const float rmean = rsum / (float)R;
    for (int c = 0; c < C; ++c) {
        const float cf = nd_rsq(col[c]);
        for (int r = 0; r < R; ++r) w[r * C + c] -= step * (g[r * C + c] * (nd_rsq(row[r] / rmean) * cf));
    }
}

// Phase A: per block -- sum p^2; kind 0: v EMA + sum u^2; kind 1: row / col EMAs + sum u^2; kind 2: partial row and column sums of a tile
__global__ __launch_bounds__(256) void k_nd_a(const NdParam *__restrict__ P, const NdBlock *__restrict__ Bk, const int *__restrict__ steps,
                                              float *state, float *__restrict__ colpart, float *__restrict__ rowpart,
                                              float *__restrict__ part_p2, float *__restrict__ part_u2, float decay, float eps1) {
    __shared__ float red[4];
    __shared__ float colred[4][ND_TC];
    const NdBlock b = Bk[blockIdx.x];
    const NdParam p = P[b.pid];
    if (!p.active) return;
    float beta, omb;
    nd_beta(steps[b.pid] + 1, decay, beta, omb);
    float sp = 0.f, su = 0.f;
    if (p.kind == 0) {
        float *v = state + p.row_off;
        for (int i = b.r0 + threadIdx.x; i < b.r0 + b.nr; i += 256) {
            const float gv = p.g[i], wv = p.p[i];
            const float vv = beta * v[i] + omb * fmaf(gv, gv, eps1);
            v[i] = vv;
            const float u = gv * nd_rsq(vv);
            su = fmaf(u, u, su);
            sp = fmaf(wv, wv, sp);
        }
    } else if (p.kind == 1) {
        if ((int)threadIdx.x < b.nr) {
            const size_t s = (size_t)b.r0 + threadIdx.x;
            if (p.R == 3 && p.C == 3) nd_tiny_a<3, 3>(p, s, beta, omb, eps1, state, sp, su);
            else if (p.R == 1 && p.C == 1) nd_tiny_a<1, 1>(p, s, beta, omb, eps1, state, sp, su);
            else nd_tiny_a<0, 0>(p, s, beta, omb, eps1, state, sp, su);
        }
    } else {
        // wave wv takes the tile's rows wv, wv + 4, ...; lane l the columns l, l + 64, ...: a row's partial sum is a wave reduction,
        // the column sums stay in registers until the end (da_optim.hip's phase A, over a column chunk)
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int ncb = (p.C + ND_TC - 1) / ND_TC, nrb = (p.R + ND_TR - 1) / ND_TR;
        const size_t base = (size_t)b.b * p.R * p.C + b.c0 + lane;
        float *rp = rowpart + p.rowpart_off + ((size_t)b.b * ncb + b.c0 / ND_TC) * p.R;
        float *cp = colpart + p.colpart_off + ((size_t)b.b * nrb + b.r0 / ND_TR) * p.C + b.c0;
        float ca[ND_CPL];
#pragma unroll
        for (int k = 0; k < ND_CPL; ++k) ca[k] = 0.f;
        const int ncl = (b.nc - lane + 63) / 64;            // the columns this lane really has
        for (int r = b.r0 + wv; r < b.r0 + b.nr; r += 4) {
            const float *g0 = p.g + base + (size_t)r * p.C, *w0 = p.p + base + (size_t)r * p.C;
            float sr = 0.f;
#pragma unroll
            for (int k = 0; k < ND_CPL; ++k) {
                if (k < ncl) {
                    const float gv = g0[64 * k], wv_ = w0[64 * k];
                    const float q = fmaf(gv, gv, eps1);
                    sr += q;
                    ca[k] += q;
                    sp = fmaf(wv_, wv_, sp);
                }
            }
            for (int o = 32; o > 0; o >>= 1) sr += __shfl_xor(sr, o);
            if (lane == 0) rp[r] = sr;
        }
#pragma unroll
        for (int k = 0; k < ND_CPL; ++k) colred[wv][lane + 64 * k] = ca[k];
        __syncthreads();
        for (int c = threadIdx.x; c < b.nc; c += 256) cp[c] = (colred[0][c] + colred[1][c]) + (colred[2][c] + colred[3][c]);
    }
    sp = nd_block_sum(sp, red);
    su = nd_block_sum(su, red);
    if (threadIdx.x == 0) { part_p2[blockIdx.x] = sp; part_u2[blockIdx.x] = su; }
}

// Phase B: one block per job.  Column job (kind 2): the column EMA of 64 columns of a slice, four threads per column (thread (tx, ty) adds
// the row blocks' partials ty, ty + 4, ... in ascending order, the four sub-sums combine as (s0 + s1) + (s2 + s3)).  Row job: kind 2 -- the
// row EMA of every row of a slice from the column chunks' partials in ascending order, and the slice's mean of it; slice 0 of every kind --
// rms(p) -> lr.
__global__ __launch_bounds__(256) void k_nd_b(const NdParam *__restrict__ P, const NdJob *__restrict__ J, const int *__restrict__ steps,
                                              float *state, const float *__restrict__ colpart, const float *__restrict__ rowpart,
                                              const float *__restrict__ part_p2, float *__restrict__ scal /* [n][4]: lr, rms(p), -, - */,
                                              float *__restrict__ rmean, float decay, float eps2) {
    __shared__ float red[4];
    __shared__ float csub[4][ND_BCH];
    const NdJob j = J[blockIdx.x];
    const NdParam p = P[j.pid];
    if (!p.active) return;
    const int t = steps[j.pid] + 1;
    float beta, omb;
    nd_beta(t, decay, beta, omb);
    if (j.c0 >= 0) {
        const int nrb = (p.R + ND_TR - 1) / ND_TR;
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = j.c0 + tx;
        float s = 0.f;
        if (c < p.C) {
            const float *cp = colpart + p.colpart_off + (size_t)j.b * nrb * p.C + c;
            int k = ty;
            for (; k + 28 < nrb; k += 32) {              // eight of this thread's partials in flight
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = cp[(size_t)(k + 4 * u) * p.C];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; k < nrb; k += 4) s += cp[(size_t)k * p.C];
        }
        csub[ty][tx] = s;
        __syncthreads();
        if (ty == 0 && c < p.C) {
            float *col = state + p.col_off + (size_t)j.b * p.C;
            const float tot = (csub[0][tx] + csub[1][tx]) + (csub[2][tx] + csub[3][tx]);
            col[c] = beta * col[c] + omb * (tot / (float)p.R);
        }
        return;
    }
    if (p.kind == 2) {
        const int ncb = (p.C + ND_TC - 1) / ND_TC;
        float *row = state + p.row_off + (size_t)j.b * p.R;
        const float *rp = rowpart + p.rowpart_off + (size_t)j.b * ncb * p.R;
        float rm = 0.f;
        for (int r = threadIdx.x; r < p.R; r += 256) {
            float s = 0.f;
            for (int k = 0; k < ncb; ++k) s += rp[(size_t)k * p.R + r];
            const float rv = beta * row[r] + omb * (s / (float)p.C);
            row[r] = rv;
            rm += rv;
        }
        rm = nd_block_sum(rm, red);
        if (threadIdx.x == 0) rmean[p.rmean_off + j.b] = rm / (float)p.R;
    }
    if (j.b != 0) return;
    float s = 0.f;
    for (int k = threadIdx.x; k < p.nblk; k += 256) s += part_p2[p.blk0 + k];
    s = nd_block_sum(s, red);
    if (threadIdx.x == 0) {
        const double numel = (double)p.B * (double)p.R * (double)p.C;
        const float rms = (float)sqrt((double)s / numel);       // one rounding: this value is also the checkpoint's "RMS"
        const float rho = (float)fmin(1e-2, 1.0 / sqrt((double)t));
        scal[j.pid * 4 + 0] = fmaxf(eps2, rms) * rho;
        scal[j.pid * 4 + 1] = rms;
    }
}

// the factors of a kind-2 tile: row factors of its <= 16 rows into LDS; a thread's column factor is computed by the caller
__device__ __forceinline__ void nd_tile_rf(const NdParam &p, const NdBlock &b, const float *state, const float *rmean, float *rfs) {
    if ((int)threadIdx.x < b.nr) {
        const float rm = rmean[p.rmean_off + b.b];
        rfs[threadIdx.x] = nd_rsq(state[p.row_off + (size_t)b.b * p.R + b.r0 + threadIdx.x] / rm);
    }
    __syncthreads();
}

// Phase C (kind 2): sum u^2 per tile
__global__ __launch_bounds__(256) void k_nd_c(const NdParam *__restrict__ P, const NdBlock *__restrict__ Bk, const float *__restrict__ state,
                                              const float *__restrict__ rmean, float *__restrict__ part_u2) {
    __shared__ float red[4];
    __shared__ float rfs[ND_TR];
    const NdBlock b = Bk[blockIdx.x];
    const NdParam p = P[b.pid];
    if (!p.active || p.kind != 2) return;          // kinds 0 and 1 were done in phase A (uniform per block)
    nd_tile_rf(p, b, state, rmean, rfs);
    const float *col = state + p.col_off + (size_t)b.b * p.C + b.c0;
    const float *g = p.g + (size_t)b.b * p.R * p.C + (size_t)b.r0 * p.C + b.c0;
    float su = 0.f;
    for (int c = threadIdx.x; c < b.nc; c += 256) {
        const float cf = nd_rsq(col[c]);
        if (b.nr == ND_TR) {
            float gv[ND_TR];
#pragma unroll
            for (int x = 0; x < ND_TR; ++x) gv[x] = g[(size_t)x * p.C + c];
#pragma unroll
            for (int x = 0; x < ND_TR; ++x) { const float u = gv[x] * (rfs[x] * cf); su = fmaf(u, u, su); }
        } else {
            for (int x = 0; x < b.nr; ++x) { const float u = g[(size_t)x * p.C + c] * (rfs[x] * cf); su = fmaf(u, u, su); }
        }
    }
    su = nd_block_sum(su, red);
    if (threadIdx.x == 0) part_u2[blockIdx.x] = su;
}

// Phase D: clip by rms(u), apply; the tensor's first block advances its step counter (no other block of this launch reads it)
__global__ __launch_bounds__(256) void k_nd_d(const NdParam *__restrict__ P, const NdBlock *__restrict__ Bk, int *__restrict__ steps,
                                              const float *__restrict__ state, const float *__restrict__ rmean, const float *__restrict__ scal,
                                              const float *__restrict__ part_u2, float clip) {
    __shared__ float red[4];
    __shared__ float rfs[ND_TR];
    const NdBlock b = Bk[blockIdx.x];
    const NdParam p = P[b.pid];
    if (!p.active) return;
    float s = 0.f;
    for (int k = threadIdx.x; k < p.nblk; k += 256) s += part_u2[p.blk0 + k];
    s = nd_block_sum(s, red);
    const float numel = (float)p.B * (float)p.R * (float)p.C;
    const float rms_u = sqrtf(s) / sqrtf(numel);
    const float step = scal[b.pid * 4 + 0] / fmaxf(1.0f, rms_u / clip);
    if ((int)blockIdx.x == p.blk0 && threadIdx.x == 0) steps[b.pid] += 1;
    if (p.kind == 0) {
        const float *v = state + p.row_off;
        for (int i = b.r0 + threadIdx.x; i < b.r0 + b.nr; i += 256) p.p[i] -= step * (p.g[i] * nd_rsq(v[i]));
    } else if (p.kind == 1) {
        if ((int)threadIdx.x < b.nr) {
            const size_t sl = (size_t)b.r0 + threadIdx.x;
            if (p.R == 3 && p.C == 3) nd_tiny_d<3, 3>(p, sl, step, state);
            else if (p.R == 1 && p.C == 1) nd_tiny_d<1, 1>(p, sl, step, state);
            else nd_tiny_d<0, 0>(p, sl, step, state);
        }
    } else {
        nd_tile_rf(p, b, state, rmean, rfs);
        const float *col = state + p.col_off + (size_t)b.b * p.C + b.c0;
        const size_t i0 = (size_t)b.b * p.R * p.C + (size_t)b.r0 * p.C + b.c0;
        const float *g = p.g + i0;
        float *w = p.p + i0;
        for (int c = threadIdx.x; c < b.nc; c += 256) {
            const float cf = nd_rsq(col[c]);
            if (b.nr == ND_TR) {
                float gv[ND_TR], wv[ND_TR];
#pragma unroll
                for (int x = 0; x < ND_TR; ++x) { gv[x] = g[(size_t)x * p.C + c]; wv[x] = w[(size_t)x * p.C + c]; }
#pragma unroll
                for (int x = 0; x < ND_TR; ++x) w[(size_t)x * p.C + c] = wv[x] - step * (gv[x] * (rfs[x] * cf));
            } else {
                for (int x = 0; x < b.nr; ++x) w[(size_t)x * p.C + c] -= step * (g[(size_t)x * p.C + c] * (rfs[x] * cf));
            }
        }
    }
}

}  // namespace da

using namespace da;

extern "C" {

int da_adafactor_nd_step(int n_params, const void *param_table, int n_blocks, const void *block_table, int n_jobs,
                         const void *job_table, int *steps, float *state, float *scratch, size_t scratch_floats, int n_slices,
                         size_t colpart_floats, size_t rowpart_floats, float eps1, float eps2, float clip_threshold, float decay_rate, void *stream) {
    DA_REQUIRE(n_params > 0 && n_blocks > 0 && n_jobs > 0 && n_slices >= 0 && param_table && block_table && job_table && steps && state && scratch,
               "da_adafactor_nd_step: null argument");
    static_assert(sizeof(NdParam) == 80 && sizeof(NdBlock) == 24 && sizeof(NdJob) == 12, "table layouts are part of the ABI (see train.py)");
    hipStream_t st = (hipStream_t)stream;
    const NdParam *P = (const NdParam *)param_table;
    const NdBlock *B = (const NdBlock *)block_table;
    const NdJob *J = (const NdJob *)job_table;
    // scratch: [n_blocks] p^2 partials | [n_blocks] u^2 partials | [n_params][4] scalars | [n_slices] row means | column partials | row partials
    const size_t head = 2 * (size_t)n_blocks + 4 * (size_t)n_params + (size_t)n_slices;
    DA_REQUIRE(scratch_floats >= head + colpart_floats + rowpart_floats, "da_adafactor_nd_step: scratch too small");
    float *part_p2 = scratch, *part_u2 = scratch + n_blocks, *scal = scratch + 2 * (size_t)n_blocks, *rmean = scal + 4 * (size_t)n_params;
    float *colpart = scratch + head, *rowpart = colpart + colpart_floats;
    k_nd_a<<<n_blocks, 256, 0, st>>>(P, B, steps, state, colpart, rowpart, part_p2, part_u2, decay_rate, eps1);
    k_nd_b<<<n_jobs, 256, 0, st>>>(P, J, steps, state, colpart, rowpart, part_p2, scal, rmean, decay_rate, eps2);
    k_nd_c<<<n_blocks, 256, 0, st>>>(P, B, state, rmean, part_u2);
    k_nd_d<<<n_blocks, 256, 0, st>>>(P, B, steps, state, rmean, scal, part_u2, clip_threshold);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
