// PointNet fragment encoder (backbone="pointnet"): the reference's plain PointNet (backbones/pointnet.py:8-43), five 1x1
// convolutions 3 -> 64 -> 64 -> 64 -> 128 -> feat without bias, BatchNorm1d after each, ReLU after the first four, max over the
// points of a fragment.  fp32 throughout.
//
// The matrix product of every 64 / 128-wide layer is Y[point][cout] = sum_k X[point][k] W[cout][k] on v_mfma_f32_32x32x2_f32
// (exact fp32): the points of a 64-point tile are the A operand's rows, read from LDS 16 bytes at a time (the k index inside a
// step is permuted the same way for both operands: lane half h takes k = 8 s + 4 h .. + 3 of step s), the output channels are
// the B operand's columns and live in REGISTERS for the whole launch -- a wave owns 32 output channels of a layer, i.e.
// cin / 8 float4 per lane (32 VGPRs for a 64-wide input, 64 for the 128-wide one).  A workgroup (4 waves) walks over many
// tiles with its weights resident, so a tile costs no weight traffic at all.  The result has its channel on the lane
// (col = lane & 31) and 16 points in the registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): the bias is one scalar
// per lane, the next layer's LDS rows are written 32 consecutive floats per half wave, and the max over points is an in-lane
// max followed by one exchange between the two lane halves.
//
//   eval:   k_pn_eval -- ONE launch: points -> layer 1 as plain FMAs -> layers 2..5 through two LDS row buffers (activations never
//           leave the CU) -> running max per (wave, channel) over the workgroup's tiles.  A fragment cut over S > 1 workgroups
//           leaves S partial rows, reduced by k_pn_max_partials (no float atomics; everything starts from -inf).
//   train:  batch statistics need all rows of a layer before the next one can start, so the forward is one k_pn_layer launch
//           per layer (input rows normalised + ReLU'd on their way into LDS, pre-normalisation output rows kept in the state
//           for the backward) with per-workgroup Welford partials (tile mean, centred tile M2, merged tile after tile in fp32
//           in a fixed order), combined across workgroups per channel in fp64 in a fixed order (k_pn_stat_finish), then
//           k_pn_pool_train (affine, max, arg-max with ties to the lowest index).
//   backward: scatter d_out to the arg-max rows, then per layer from the last to the first: BatchNorm backward as reduce
//           (fixed-order partials) -> finish -> apply in place, the input activation rebuilt from the saved rows (k_pn_act),
//           dW = dY^T X through launch_gemm_tn (deterministic split over rows) and dX = dY W through k_pn_layer on the
//           transposed weight.
#include "da_internal.h"

namespace da {
namespace {

typedef __attribute__((ext_vector_type(4))) float pn_f4;
typedef __attribute__((ext_vector_type(16))) float pn_f16;

constexpr int PN_TILE = 64;                        // points per tile
constexpr int PN_CMAX = 128;                       // widest layer
constexpr int PN_STAT_BLOCKS = 1024;               // workgroups (= Welford partials) of a train-forward layer at most
constexpr int PN_BWD_ROWS = 256;                   // rows per workgroup of the BatchNorm backward's reduction
constexpr size_t PN_GEMM_PART = (size_t)16 << 20;  // floats of launch_gemm_tn's split scratch

// this lane's share of the 32 output channels a wave owns: v[s] = W[col][8 s + 4 half .. + 3]
template <int CIN> struct WSlice { pn_f4 v[CIN / 8]; };

template <int CIN>
__device__ __forceinline__ void load_wslice(WSlice<CIN> &ws, const float *__restrict__ W, int col, int half, bool on) {
#pragma unroll
    for (int s = 0; s < CIN / 8; ++s)
        ws.v[s] = on ? *(const pn_f4 *)(W + (size_t)col * CIN + 8 * s + 4 * half) : (pn_f4){0.f, 0.f, 0.f, 0.f};
}

// acc[b] += X[rows 32 (rb0 + b) .. + 31] . W^T over CIN columns; Xs rows LD floats apart (LD = 4 mod 32: the 16-byte reads of
// 16 consecutive rows cover all banks once)
template <int CIN, int NRB, int LD>
__device__ __forceinline__ void mma_rows(const float *Xs, int rb0, const WSlice<CIN> &ws, pn_f16 (&acc)[NRB], int lane) {
    const int r = lane & 31, half = lane >> 5;
#pragma unroll
    for (int s = 0; s < CIN / 8; ++s) {
#pragma unroll
        for (int b = 0; b < NRB; ++b) {
            const pn_f4 x = *(const pn_f4 *)(Xs + ((rb0 + b) * 32 + r) * LD + 8 * s + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], ws.v[s][e], acc[b], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ pn_f16 zero16() {
    pn_f16 z;
#pragma unroll
    for (int v = 0; v < 16; ++v) z[v] = 0.f;
    return z;
}

// the 32 x 32 result block (row block rb, this lane's column `col`) into LDS rows, + bias, optional ReLU
template <bool RELU, int LD>
__device__ __forceinline__ void acc_to_lds(float *Ys, int rb, int col, const pn_f16 &acc, float bias, int lane) {
    const int half = lane >> 5;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = rb * 32 + 8 * (v >> 2) + 4 * half + (v & 3);
        float y = acc[v] + bias;
        if (RELU) y = fmaxf(y, 0.f);
        Ys[row * LD + col] = y;
    }
}

struct PnEvalW { const float *w[5], *b[5]; };

// ---- eval: all five layers of a tile inside the CU --------------------------------------------------------------------
// workgroup = (fragment p, chunk q of `tpc` tiles); dst row p * S + q (S == 1: the output itself).  Bounded to 256 registers: two
// workgroups per CU, so one's epilogues and barriers run under the other's MFMAs (no spills: tools/kernel_resources.py)
__global__ __launch_bounds__(256, 2) void k_pn_eval(PnEvalW W, int N, int tiles, int tpc, int S, int feat,
                                                 const float *__restrict__ points, float *__restrict__ dst, int ld_dst) {
    constexpr int L64 = 68, L128 = 132;
    __shared__ __attribute__((aligned(16))) float Xa[PN_TILE * L128];
    __shared__ __attribute__((aligned(16))) float Xb[PN_TILE * L64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, half = lane >> 5;
    const int p = blockIdx.x / S, q = blockIdx.x - p * S;
    const int cb2 = w & 1, rb2 = w >> 1;                 // 64-wide outputs: (row block, column block) per wave
    const bool on5 = w * 32 < feat;                      // 128-wide outputs: column block w, both row blocks
    WSlice<64> w2, w3, w4;
    WSlice<128> w5;
    load_wslice<64>(w2, W.w[1], cb2 * 32 + r, half, true);
    load_wslice<64>(w3, W.w[2], cb2 * 32 + r, half, true);
    load_wslice<64>(w4, W.w[3], w * 32 + r, half, true);
    load_wslice<128>(w5, W.w[4], w * 32 + r, half, on5);
    const float b2 = W.b[1][cb2 * 32 + r], b3 = W.b[2][cb2 * 32 + r], b4 = W.b[3][w * 32 + r];
    const float b5 = on5 ? W.b[4][w * 32 + r] : 0.f;
    const int c1 = tid & 63, g1 = tid >> 6;              // layer 1: channel c1 of the 16 points g1 * 16 ..
    const float w1x = W.w[0][c1 * 3], w1y = W.w[0][c1 * 3 + 1], w1z = W.w[0][c1 * 3 + 2], b1 = W.b[0][c1];
    const float *pts = points + (size_t)p * N * 3;
    const int t_end = min(tiles, (q + 1) * tpc);
    float best = -INFINITY;
    for (int t = q * tpc; t < t_end; ++t) {
        const int n0 = t * PN_TILE, valid = min(PN_TILE, N - n0);
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int row = g1 * 16 + i;
            float y = 0.f;
            if (row < valid) {
                const float *pp = pts + (size_t)(n0 + row) * 3;
                y = fmaxf(fmaf(pp[2], w1z, fmaf(pp[1], w1y, fmaf(pp[0], w1x, b1))), 0.f);
            }
            Xb[row * L64 + c1] = y;
        }
        __syncthreads();
        {
            pn_f16 acc[1] = {zero16()};
            mma_rows<64, 1, L64>(Xb, rb2, w2, acc, lane);
            acc_to_lds<true, L64>(Xa, rb2, cb2 * 32 + r, acc[0], b2, lane);
        }
        __syncthreads();
        {
            pn_f16 acc[1] = {zero16()};
            mma_rows<64, 1, L64>(Xa, rb2, w3, acc, lane);
            acc_to_lds<true, L64>(Xb, rb2, cb2 * 32 + r, acc[0], b3, lane);
        }
        __syncthreads();
        {
            pn_f16 acc[2] = {zero16(), zero16()};
            mma_rows<64, 2, L64>(Xb, 0, w4, acc, lane);
            acc_to_lds<true, L128>(Xa, 0, w * 32 + r, acc[0], b4, lane);
            acc_to_lds<true, L128>(Xa, 1, w * 32 + r, acc[1], b4, lane);
        }
        __syncthreads();
        if (on5) {
            pn_f16 acc[2] = {zero16(), zero16()};
            mma_rows<128, 2, L128>(Xa, 0, w5, acc, lane);
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int row = b * 32 + 8 * (v >> 2) + 4 * half + (v & 3);
                    if (row < valid) best = fmaxf(best, acc[b][v] + b5);
                }
        }
        // the next tile's layer 1 writes Xb (last read before the barrier above); Xa is rewritten only behind its barrier
    }
    best = fmaxf(best, __shfl_xor(best, 32));
    if (on5 && half == 0) dst[(size_t)blockIdx.x * ld_dst + w * 32 + r] = best;
}

__global__ __launch_bounds__(256) void k_pn_max_partials(int P, int S, int feat, const float *__restrict__ part, float *__restrict__ out,
                                                         int ld_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)P * feat) return;
    const int p = (int)(i / feat), c = (int)(i - (long long)p * feat);
    float best = -INFINITY;
    for (int q = 0; q < S; ++q) best = fmaxf(best, part[((size_t)p * S + q) * feat + c]);
    out[(size_t)p * ld_out + c] = best;
}

void pn_eval_split(int P, int N, int *tiles, int *tpc, int *S) {
    *tiles = (N + PN_TILE - 1) / PN_TILE;
    int s = 2048 / (P > 0 ? P : 1);
    s = s < 1 ? 1 : (s > *tiles ? *tiles : s);
    *tpc = (*tiles + s - 1) / s;
    *S = (*tiles + *tpc - 1) / *tpc;
}

// ---- train: one layer over all rows -----------------------------------------------------------------------------------
// IN_MODE 0: X rows as they are; 1: relu(x * in_scale + in_shift) per input channel; 2: X = points [M][3], the
// layer is conv1 (plain FMAs, CIN unused).  Y [M][COUT] = rows . W^T (W [COUT][CIN]).  STATS: part[block][3][COUT] = this
// workgroup's (count, mean, centred second moment) per channel, its tiles merged in ascending order.
template <int CIN, int COUT, int IN_MODE, bool STATS>
__global__ __launch_bounds__(256) void k_pn_layer(long long M, const float *__restrict__ X, const float *__restrict__ in_scale,
                                                  const float *__restrict__ in_shift, const float *__restrict__ W, float *__restrict__ Y,
                                                  float *__restrict__ part) {
    constexpr int LDX = CIN + 4, LDY = COUT + 4, NCB = COUT / 32, NRB = NCB == 4 ? 2 : 1, G = 256 / COUT;
    constexpr int BUF = PN_TILE * (LDX > LDY ? LDX : LDY);
    __shared__ __attribute__((aligned(16))) float Xs[BUF];       // input rows, then (behind a barrier) the output rows
    __shared__ float red[2][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, half = lane >> 5;
    const int cb = NCB == 4 ? w : (w & 1), rb0 = NCB == 4 ? 0 : (w >> 1);
    WSlice<CIN> ws;
    float w1x = 0.f, w1y = 0.f, w1z = 0.f;
    if (IN_MODE == 2) {
        w1x = W[(tid & 63) * 3]; w1y = W[(tid & 63) * 3 + 1]; w1z = W[(tid & 63) * 3 + 2];
    } else {
        load_wslice<CIN>(ws, W, cb * 32 + r, half, true);
    }
    const int sc = tid % COUT, sg = tid / COUT;                  // statistics: channel sc, rows sg, sg + G, ...
    float run_n = 0.f, run_mean = 0.f, run_m2 = 0.f;
    const long long ntiles = (M + PN_TILE - 1) / PN_TILE;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long row0 = t * PN_TILE;
        const int valid = (int)(M - row0 < PN_TILE ? M - row0 : PN_TILE);
        if (IN_MODE == 2) {
            const int c1 = tid & 63, g1 = tid >> 6;
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int row = g1 * 16 + i;
                float y = 0.f;
                if (row < valid) {
                    const float *pp = X + (size_t)(row0 + row) * 3;
                    y = fmaf(pp[2], w1z, fmaf(pp[1], w1y, pp[0] * w1x));
                }
                Xs[row * LDY + c1] = y;
            }
        } else {
            for (int i = tid; i < PN_TILE * (CIN / 4); i += 256) {
                const int row = i / (CIN / 4), c4 = (i - row * (CIN / 4)) * 4;
                pn_f4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < valid) {
                    v = *(const pn_f4 *)(X + (size_t)(row0 + row) * CIN + c4);
                    if (IN_MODE == 1) {
                        const pn_f4 sc4 = *(const pn_f4 *)(in_scale + c4), sh4 = *(const pn_f4 *)(in_shift + c4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(v[e], sc4[e], sh4[e]), 0.f);
                    }
                }
                *(pn_f4 *)(Xs + row * LDX + c4) = v;
            }
            __syncthreads();
            pn_f16 acc[NRB];
#pragma unroll
            for (int b = 0; b < NRB; ++b) acc[b] = zero16();
            mma_rows<CIN, NRB, LDX>(Xs, rb0, ws, acc, lane);
            __syncthreads();                                     // every wave has read its input rows
#pragma unroll
            for (int b = 0; b < NRB; ++b) acc_to_lds<false, LDY>(Xs, rb0 + b, cb * 32 + r, acc[b], 0.f, lane);
        }
        __syncthreads();
        for (int i = tid; i < PN_TILE * (COUT / 4); i += 256) {
            const int row = i / (COUT / 4), c4 = (i - row * (COUT / 4)) * 4;
            if (row < valid) *(pn_f4 *)(Y + (size_t)(row0 + row) * COUT + c4) = *(const pn_f4 *)(Xs + row * LDY + c4);
        }
        if (STATS) {
            float s = 0.f;
            for (int row = sg; row < valid; row += G) s += Xs[row * LDY + sc];
            red[0][sg * COUT + sc] = s;
            __syncthreads();
            float ts = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) ts += red[0][g * COUT + sc];
            const float tmean = ts / (float)valid;
            float qd = 0.f;
            for (int row = sg; row < valid; row += G) {
                const float d = Xs[row * LDY + sc] - tmean;
                qd = fmaf(d, d, qd);
            }
            red[1][sg * COUT + sc] = qd;
            __syncthreads();
            if (sg == 0) {
                float tm2 = 0.f;
#pragma unroll
                for (int g = 0; g < G; ++g) tm2 += red[1][g * COUT + sc];
                const float nb = (float)valid, n = run_n + nb, delta = tmean - run_mean;
                run_mean += delta * (nb / n);
                run_m2 += tm2 + delta * delta * (run_n * nb / n);
                run_n = n;
            }
        }
        __syncthreads();                                         // the next tile's rows overwrite Xs
    }
    if (STATS && sg == 0) {
        float *pb = part + (size_t)blockIdx.x * 3 * COUT;
        pb[sc] = run_n; pb[COUT + sc] = run_mean; pb[2 * COUT + sc] = run_m2;
    }
}

// the workgroups' (n, mean, M2) per channel in fp64: 1024 threads = 1024 / C strided subsets of the partials per channel, each summed in
// ascending order, the subsets then added in ascending order (fixed for a given M).  stats [4][128]: mean, 1 / sqrt(var + eps),
// scale = gamma * that, shift = beta - mean * scale; run_out [2][128]: updated running mean / variance
__global__ __launch_bounds__(1024) void k_pn_stat_finish(int nblk, int C, double M, const float *__restrict__ part, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, const float *__restrict__ rmean,
                                                         const float *__restrict__ rvar, float momentum, float eps, float *__restrict__ stats,
                                                         float *__restrict__ run_out) {
    __shared__ double red[1024];
    const int tid = threadIdx.x, G = 1024 / C, c = tid % C, g = tid / C;
    double sum = 0.0;
    for (int b = g; b < nblk; b += G) sum += (double)part[(size_t)b * 3 * C + c] * (double)part[(size_t)b * 3 * C + C + c];
    red[tid] = sum;
    __syncthreads();
    sum = 0.0;
    for (int k = 0; k < G; ++k) sum += red[k * C + c];
    const double mean = sum / M;
    __syncthreads();
    double m2 = 0.0;
    for (int b = g; b < nblk; b += G) {
        const double n = part[(size_t)b * 3 * C + c], d = (double)part[(size_t)b * 3 * C + C + c] - mean;
        m2 += (double)part[(size_t)b * 3 * C + 2 * C + c] + n * d * d;
    }
    red[tid] = m2;
    __syncthreads();
    if (g != 0) return;
    m2 = 0.0;
    for (int k = 0; k < G; ++k) m2 += red[k * C + c];
    const double var = m2 / M, istd = 1.0 / sqrt(var + (double)eps);
    const float fmean = (float)mean, fistd = (float)istd, scale = gamma[c] * fistd;
    stats[c] = fmean;
    stats[PN_CMAX + c] = fistd;
    stats[2 * PN_CMAX + c] = scale;
    stats[3 * PN_CMAX + c] = fmaf(-fmean, scale, beta[c]);
    run_out[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
    run_out[PN_CMAX + c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * (m2 / (M - 1.0)));
}

// out[p][c] = max_n (Y[p, n][c] * scale[c] + shift[c]), arg[p][c] = the lowest n that attains it.  One workgroup per fragment.
__global__ __launch_bounds__(256) void k_pn_pool_train(int N, int C, const float *__restrict__ Y, const float *__restrict__ stats,
                                                       float *__restrict__ out, int ld_out, int32_t *__restrict__ arg) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int tid = threadIdx.x, G = 256 / C, c = tid % C, g = tid / C, p = blockIdx.x;
    const float scale = stats[2 * PN_CMAX + c], shift = stats[3 * PN_CMAX + c];
    const float *y = Y + (size_t)p * N * C + c;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int n = g; n < N; n += G) {
        const float z = fmaf(y[(size_t)n * C], scale, shift);
        if (z > best || at == 0x7fffffff) { best = z; at = n; }
    }
    bv[tid] = best; bi[tid] = at;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < G; ++k) {
            const float v = bv[k * C + c];
            const int i = bi[k * C + c];
            if (i != 0x7fffffff && (v > best || (v == best && i < at))) { best = v; at = i; }
        }
        out[(size_t)p * ld_out + c] = best;
        arg[(size_t)p * C + c] = at;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pn_scatter(int P, int N, int C, const float *__restrict__ go, int ld_g, const int32_t *__restrict__ arg,
                                                    float *__restrict__ DA) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)P * C) return;
    const int p = (int)(i / C), c = (int)(i - (long long)p * C);
    DA[((size_t)p * N + arg[i]) * C + c] = go[(size_t)p * ld_g + c];
}

// part[block][2][C]: sum dz, sum dz xhat over the block's rows (dz = the incoming gradient behind the ReLU mask)
__global__ __launch_bounds__(256) void k_pn_bwd_reduce(long long M, int C, int relu, const float *__restrict__ DA, const float *__restrict__ Y,
                                                       const float *__restrict__ stats, float *__restrict__ part) {
    __shared__ float red[2][256];
    const int tid = threadIdx.x, G = 256 / C, c = tid % C, g = tid / C;
    const float mean = stats[c], istd = stats[PN_CMAX + c], scale = stats[2 * PN_CMAX + c], shift = stats[3 * PN_CMAX + c];
    const long long m0 = (long long)blockIdx.x * PN_BWD_ROWS, m1 = m0 + PN_BWD_ROWS < M ? m0 + PN_BWD_ROWS : M;
    float s1 = 0.f, s2 = 0.f;
    for (long long m = m0 + g; m < m1; m += G) {
        const float y = Y[(size_t)m * C + c];
        float dz = DA[(size_t)m * C + c];
        if (relu && !(fmaf(y, scale, shift) > 0.f)) dz = 0.f;
        s1 += dz;
        s2 = fmaf(dz, (y - mean) * istd, s2);
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < G; ++k) { s1 += red[0][k * C + c]; s2 += red[1][k * C + c]; }
        part[((size_t)blockIdx.x * 2) * C + c] = s1;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = s2;
    }
}

// the blocks' sums per channel in fp64, subsets as in k_pn_stat_finish
__global__ __launch_bounds__(1024) void k_pn_bwd_finish(int nblk, int C, const float *__restrict__ part, float *__restrict__ s12,
                                                        float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double red[2][1024];
    const int tid = threadIdx.x, G = 1024 / C, c = tid % C, g = tid / C;
    double a = 0.0, b = 0.0;
    for (int k = g; k < nblk; k += G) { a += (double)part[((size_t)k * 2) * C + c]; b += (double)part[((size_t)k * 2 + 1) * C + c]; }
    red[0][tid] = a; red[1][tid] = b;
    __syncthreads();
    if (g != 0) return;
    a = b = 0.0;
    for (int k = 0; k < G; ++k) { a += red[0][k * C + c]; b += red[1][k * C + c]; }
    s12[c] = (float)a; s12[PN_CMAX + c] = (float)b;
    dbeta[c] += (float)a;
    dgamma[c] += (float)b;
}

// DA <- gamma inv_std (dz - mean(dz) - xhat mean(dz xhat)): the gradient of the layer's pre-normalisation rows, in place
__global__ __launch_bounds__(256) void k_pn_bwd_apply(long long total, int C, int relu, float *__restrict__ DA, const float *__restrict__ Y,
                                                      const float *__restrict__ stats, const float *__restrict__ s12, float inv_m) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float mean = stats[c], istd = stats[PN_CMAX + c], scale = stats[2 * PN_CMAX + c], shift = stats[3 * PN_CMAX + c];
        const float y = Y[i];
        float dz = DA[i];
        if (relu && !(fmaf(y, scale, shift) > 0.f)) dz = 0.f;
        const float xh = (y - mean) * istd;
        DA[i] = scale * (dz - s12[c] * inv_m - xh * (s12[PN_CMAX + c] * inv_m));
    }
}

__global__ __launch_bounds__(256) void k_pn_act(long long total, int C, const float *__restrict__ Y, const float *__restrict__ stats,
                                                float *__restrict__ A) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        A[i] = fmaxf(fmaf(Y[i], stats[2 * PN_CMAX + c], stats[3 * PN_CMAX + c]), 0.f);
    }
}

unsigned pn_grid(long long total) { const long long b = (total + 255) / 256; return (unsigned)(b < 1 ? 1 : (b < 16384 ? b : 16384)); }
int pn_width(int l, int feat) { return l == 0 ? 3 : (l <= 3 ? 64 : (l == 4 ? 128 : feat)); }      // width of layer l's INPUT; l == 5: the output

struct PnState {           // the saved state of a train forward
    float *stats;          // [5][4][128]
    int32_t *arg;          // [P][128]
    float *Y[5];           // pre-normalisation rows [M][cout]
    size_t bytes;
};
PnState pn_state(void *base, long long P, long long N, int feat) {
    PnState s;
    char *b = (char *)base;
    size_t o = 0;
    s.stats = (float *)(b + o); o += align_up((size_t)5 * 4 * PN_CMAX * sizeof(float), 256);
    s.arg = (int32_t *)(b + o); o += align_up((size_t)P * PN_CMAX * sizeof(int32_t), 256);
    for (int l = 0; l < 5; ++l) { s.Y[l] = (float *)(b + o); o += align_up((size_t)P * N * pn_width(l + 1, feat) * sizeof(float), 256); }
    s.bytes = o;
    return s;
}
struct PnWork {
    float *wpart;          // forward: [PN_STAT_BLOCKS][3][128]
    float *D0, *D1, *A;    // backward: [M][128] each
    float *rpart, *s12, *gpart;
    size_t bytes;
};
PnWork pn_work(void *base, long long M) {
    PnWork w;
    char *b = (char *)base;
    size_t o = 0;
    w.wpart = (float *)(b + o); o += align_up((size_t)PN_STAT_BLOCKS * 3 * PN_CMAX * sizeof(float), 256);
    w.D0 = (float *)(b + o); o += align_up((size_t)M * PN_CMAX * sizeof(float), 256);
    w.D1 = (float *)(b + o); o += align_up((size_t)M * PN_CMAX * sizeof(float), 256);
    w.A = (float *)(b + o); o += align_up((size_t)M * PN_CMAX * sizeof(float), 256);
    w.rpart = (float *)(b + o); o += align_up((size_t)((M + PN_BWD_ROWS - 1) / PN_BWD_ROWS) * 2 * PN_CMAX * sizeof(float), 256);
    w.s12 = (float *)(b + o); o += align_up((size_t)2 * PN_CMAX * sizeof(float), 256);
    w.gpart = (float *)(b + o); o += PN_GEMM_PART * sizeof(float);
    w.bytes = o;
    return w;
}

bool aligned16(const void *p) { return ((size_t)p & 15) == 0; }

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

size_t da_pointnet_workspace_bytes(int n_parts, int n_points, int feat_dim) {
    if (n_parts <= 0 || n_points <= 0 || feat_dim <= 0) return 0;
    int tiles, tpc, S;
    pn_eval_split(n_parts, n_points, &tiles, &tpc, &S);
    return S == 1 ? 0 : (size_t)n_parts * S * feat_dim * sizeof(float);
}

int da_pointnet_forward(const da_pointnet_weights *w, int n_parts, int n_points, const float *points, float *out, int ld_out,
                        void *workspace, size_t workspace_bytes, void *stream) {
    DA_REQUIRE(w, "da_pointnet_forward: null weights");
    const int feat = w->feat_dim;
    DA_REQUIRE(feat > 0 && feat % 32 == 0 && feat <= PN_CMAX,
               "da_pointnet_forward: feat_dim %d: the PointNet kernels take a multiple of 32 up to 128", feat);
    DA_REQUIRE(n_parts >= 0 && n_points >= 1, "da_pointnet_forward: n_parts %d / n_points %d (need >= 0 / >= 1)", n_parts, n_points);
    if (n_parts == 0) return 0;
    DA_REQUIRE(points && out && ld_out >= feat, "da_pointnet_forward: null points / out, or ld_out %d < feat_dim", ld_out);
    PnEvalW W;
    for (int l = 0; l < 5; ++l) {
        DA_REQUIRE(w->w[l] && w->b[l] && aligned16(w->w[l]), "da_pointnet_forward: layer %d: null or misaligned weights", l);
        W.w[l] = w->w[l]; W.b[l] = w->b[l];
    }
    int tiles, tpc, S;
    pn_eval_split(n_parts, n_points, &tiles, &tpc, &S);
    DA_REQUIRE((long long)n_parts * S < (1ll << 31), "da_pointnet_forward: too many fragments");
    hipStream_t st = (hipStream_t)stream;
    if (S == 1) {
        k_pn_eval<<<(unsigned)n_parts, 256, 0, st>>>(W, n_points, tiles, tpc, 1, feat, points, out, ld_out);
    } else {
        const size_t need = (size_t)n_parts * S * feat * sizeof(float);
        DA_REQUIRE(workspace && workspace_bytes >= need, "da_pointnet_forward: workspace of %zu bytes, need %zu", workspace_bytes, need);
        k_pn_eval<<<(unsigned)(n_parts * S), 256, 0, st>>>(W, n_points, tiles, tpc, S, feat, points, (float *)workspace, feat);
        k_pn_max_partials<<<pn_grid((long long)n_parts * feat), 256, 0, st>>>(n_parts, S, feat, (const float *)workspace, out, ld_out);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

size_t da_pointnet_train_state_bytes(int n_parts, int n_points, int feat_dim) {
    if (n_parts <= 0 || n_points <= 0 || feat_dim <= 0) return 0;
    return pn_state(nullptr, n_parts, n_points, feat_dim).bytes;
}

size_t da_pointnet_train_workspace_bytes(int n_parts, int n_points, int feat_dim) {
    if (n_parts <= 0 || n_points <= 0 || feat_dim <= 0) return 0;
    return pn_work(nullptr, (long long)n_parts * n_points).bytes;
}

static int pn_train_args_ok(const da_pointnet_train_weights *w, int n_parts, int n_points, const char *who) {
    DA_REQUIRE(w, "%s: null weights", who);
    DA_REQUIRE(w->feat_dim == PN_CMAX, "%s: feat_dim %d: the PointNet training kernels are built for feat_dim 128", who, w->feat_dim);
    DA_REQUIRE(n_parts >= 1 && n_points >= 1 && (long long)n_parts * n_points >= 2,
               "%s: batch statistics need more than one point (n_parts %d, n_points %d)", who, n_parts, n_points);
    DA_REQUIRE((long long)n_parts * n_points < (1ll << 24), "%s: %lld points: more than 2^24 per call", who, (long long)n_parts * n_points);
    for (int l = 0; l < 5; ++l)
        DA_REQUIRE(w->w[l] && aligned16(w->w[l]) && (l == 0 || (w->wt[l] && aligned16(w->wt[l]))) && w->gamma[l] && w->beta[l] &&
                       w->running_mean[l] && w->running_var[l],
                   "%s: layer %d: null or misaligned parameter", who, l);
    return 0;
}

int da_pointnet_train_forward(const da_pointnet_train_weights *w, int n_parts, int n_points, const float *points, float *out,
                              int ld_out, float *run_out, void *state, size_t state_bytes, void *workspace,
                              size_t workspace_bytes, void *stream) {
    if (int rc = pn_train_args_ok(w, n_parts, n_points, "da_pointnet_train_forward")) return rc;
    const int feat = w->feat_dim;
    const long long M = (long long)n_parts * n_points;
    DA_REQUIRE(points && out && run_out && state && workspace && ld_out >= feat, "da_pointnet_train_forward: null argument or ld_out < feat_dim");
    const PnState S = pn_state(state, n_parts, n_points, feat);
    const PnWork K = pn_work(workspace, M);
    DA_REQUIRE(state_bytes >= S.bytes && workspace_bytes >= K.bytes, "da_pointnet_train_forward: state %zu / workspace %zu bytes, need %zu / %zu",
               state_bytes, workspace_bytes, S.bytes, K.bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long ntiles = (M + PN_TILE - 1) / PN_TILE;
    const int nblk = (int)(ntiles < PN_STAT_BLOCKS ? ntiles : PN_STAT_BLOCKS);
    for (int l = 0; l < 5; ++l) {
        const float *isc = l ? S.stats + (size_t)(l - 1) * 4 * PN_CMAX + 2 * PN_CMAX : nullptr, *ish = l ? isc + PN_CMAX : nullptr;
        switch (l) {
            case 0: k_pn_layer<64, 64, 2, true><<<nblk, 256, 0, st>>>(M, points, nullptr, nullptr, w->w[0], S.Y[0], K.wpart); break;
            case 1: k_pn_layer<64, 64, 1, true><<<nblk, 256, 0, st>>>(M, S.Y[0], isc, ish, w->w[1], S.Y[1], K.wpart); break;
            case 2: k_pn_layer<64, 64, 1, true><<<nblk, 256, 0, st>>>(M, S.Y[1], isc, ish, w->w[2], S.Y[2], K.wpart); break;
            case 3: k_pn_layer<64, 128, 1, true><<<nblk, 256, 0, st>>>(M, S.Y[2], isc, ish, w->w[3], S.Y[3], K.wpart); break;
            default: k_pn_layer<128, 128, 1, true><<<nblk, 256, 0, st>>>(M, S.Y[3], isc, ish, w->w[4], S.Y[4], K.wpart); break;
        }
        const int cout = pn_width(l + 1, feat);
        k_pn_stat_finish<<<1, 1024, 0, st>>>(nblk, cout, (double)M, K.wpart, w->gamma[l], w->beta[l], w->running_mean[l], w->running_var[l],
                                            w->momentum[l], w->eps[l], S.stats + (size_t)l * 4 * PN_CMAX, run_out + (size_t)l * 2 * PN_CMAX);
    }
    k_pn_pool_train<<<(unsigned)n_parts, 256, 0, st>>>(n_points, feat, S.Y[4], S.stats + (size_t)4 * 4 * PN_CMAX, out, ld_out, S.arg);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_pointnet_train_backward(const da_pointnet_train_weights *w, int n_parts, int n_points, const float *points,
                               const float *grad_out, int ld_g, const void *state, const da_pointnet_train_grads *g,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = pn_train_args_ok(w, n_parts, n_points, "da_pointnet_train_backward")) return rc;
    const int feat = w->feat_dim;
    const long long M = (long long)n_parts * n_points;
    DA_REQUIRE(points && grad_out && state && g && workspace && ld_g >= feat, "da_pointnet_train_backward: null argument or ld_g < feat_dim");
    for (int l = 0; l < 5; ++l) DA_REQUIRE(g->w[l] && g->gamma[l] && g->beta[l], "da_pointnet_train_backward: layer %d: null gradient", l);
    const PnState S = pn_state((void *)state, n_parts, n_points, feat);
    const PnWork K = pn_work(workspace, M);
    DA_REQUIRE(workspace_bytes >= K.bytes, "da_pointnet_train_backward: workspace of %zu bytes, need %zu", workspace_bytes, K.bytes);
    hipStream_t st = (hipStream_t)stream;
    float *cur = K.D0, *oth = K.D1;
    DA_CHECK_HIP(hipMemsetAsync(cur, 0, (size_t)M * feat * sizeof(float), st));
    k_pn_scatter<<<pn_grid((long long)n_parts * feat), 256, 0, st>>>(n_parts, n_points, feat, grad_out, ld_g, S.arg, cur);
    const int nrb = (int)((M + PN_BWD_ROWS - 1) / PN_BWD_ROWS);
    const long long ntiles = (M + PN_TILE - 1) / PN_TILE;
    const int nblk = (int)(ntiles < PN_STAT_BLOCKS ? ntiles : PN_STAT_BLOCKS);
    const float inv_m = (float)(1.0 / (double)M);
    for (int l = 4; l >= 0; --l) {
        const int cout = pn_width(l + 1, feat), cin = pn_width(l, feat), relu = l < 4;
        const float *stats = S.stats + (size_t)l * 4 * PN_CMAX;
        k_pn_bwd_reduce<<<nrb, 256, 0, st>>>(M, cout, relu, cur, S.Y[l], stats, K.rpart);
        k_pn_bwd_finish<<<1, 1024, 0, st>>>(nrb, cout, K.rpart, K.s12, g->gamma[l], g->beta[l]);
        k_pn_bwd_apply<<<pn_grid(M * cout), 256, 0, st>>>(M * cout, cout, relu, cur, S.Y[l], stats, K.s12, inv_m);
        DA_LAUNCH_CHECK();
        if (l == 0) return launch_gemm_tn((int)M, cout, 3, cur, cout, points, 3, g->w[0], 3, K.gpart, st);
        k_pn_act<<<pn_grid(M * cin), 256, 0, st>>>(M * cin, cin, S.Y[l - 1], S.stats + (size_t)(l - 1) * 4 * PN_CMAX, K.A);
        if (int rc = launch_gemm_tn((int)M, cout, cin, cur, cout, K.A, cin, g->w[l], cin, K.gpart, st)) return rc;
        switch (l) {
            case 4: k_pn_layer<128, 128, 0, false><<<nblk, 256, 0, st>>>(M, cur, nullptr, nullptr, w->wt[4], oth, nullptr); break;
            case 3: k_pn_layer<128, 64, 0, false><<<nblk, 256, 0, st>>>(M, cur, nullptr, nullptr, w->wt[3], oth, nullptr); break;
            default: k_pn_layer<64, 64, 0, false><<<nblk, 256, 0, st>>>(M, cur, nullptr, nullptr, w->wt[l], oth, nullptr); break;
        }
        DA_LAUNCH_CHECK();
        float *t = cur; cur = oth; oth = t;
    }
    return 0;
}

}  // extern "C"
