// 3D piece encoder in train() mode: VN_DGCNN.forward with batch-statistics BatchNorm and its backward.
//
// Replaces (paths under /root/reference/puzzle_diff/model/):
//   backbones/vnn/vn_dgcnn.py:34-74     VN_DGCNN.forward in train(): kNN graph features, conv1..conv5 on the edges, mean pools,
//                                       conv6, mean over points, VnInv (run for its running statistics only), linear0
//   backbones/vnn/vn_layers.py:50-91    VNLinearLeakyReLU; :133-154 VNBatchNorm on the vector norm with BATCH statistics
//                                       (BatchNorm2d over P*N*20 edges, BatchNorm1d over P*N points / P fragments)
//   efficient_gat_3d.py:230-235         the backbone call of every training step, and torch autograd through all of it
// The reference materialises [P, 2C, 3, N, 20] edge tensors per layer (3.2 GB each at 640 x 1000).  Here no per-edge tensor
// outlives a pass: the first layer of a stage is A_j + U_i from per-point premaps (k_pcd_premap of the eval path), and every
// pass recomputes the edge chain from them.  A stage of two layers runs
//   forward:  statistics of layer a | apply a, statistics of layer b | apply both + pool (k_pcd_edge of the eval path)
//   backward: sums of layer b's BatchNorm backward | layer b's input gradient, sums of layer a's | per-edge dA, dU
// and the per-edge gradients of the first layer reach the neighbour j through a reverse adjacency (counting sort of the kNN
// lists, each list sorted by edge id) that is GATHERED, never scattered: no float atomics anywhere.  Weight gradients are
// fixed-order split GEMMs over component-major rows (launch_gemm_tn).  Per-channel batch sums: fp32 over a point's 20 edges,
// fp64 across lanes, waves and blocks, in a fixed order.
#include "da_internal.h"

namespace da {
namespace {

constexpr int KNN = DA_PCD_K, VC = DA_PCD_C, VROW = DA_PCD_ROW, V3 = VC * 3;
constexpr int NL = DA_PCD_TRAIN_LAYERS, CMAX = 256;
constexpr float VN_EPS = 1e-6f;                           // vn_layers.py:11
enum { R_MEAN, R_RSTD, R_GAMMA, R_BETA, R_MDY, R_MDYX, REC };   // stat record of a layer: [REC][CMAX] floats
constexpr int GB_LD = 44, H_LD = 24, E_LD = 2 * VROW, DT_LD = 84, XC_LD = 24;
constexpr size_t GEMM_PART = (size_t)16 << 20;            // floats of launch_gemm_tn's split scratch

struct Bn { float mu, rstd, gam, bet; };
__device__ __forceinline__ Bn bn_at(const float *rec, int c) {
    return {rec[R_MEAN * CMAX + c], rec[R_RSTD * CMAX + c], rec[R_GAMMA * CMAX + c], rec[R_BETA * CMAX + c]};
}

// VNBatchNorm (batch statistics) + the vector leaky ReLU, vn_layers.py:80-91 / :145-154.  p: in / out.
__device__ __forceinline__ void act_fwd(float (&p)[3], const float (&d)[3], const Bn &b) {
    const float n = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + VN_EPS;
    const float s = ((n - b.mu) * b.rstd * b.gam + b.bet) / n;
    p[0] *= s; p[1] *= s; p[2] *= s;
    const float dot = p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
    if (dot < 0.f) {
        const float c = 0.8f * dot / (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + VN_EPS);
        p[0] -= c * d[0]; p[1] -= c * d[1]; p[2] -= c * d[2];
    }
}

// Backward of act_fwd up to the BatchNorm output y (local part): g = dL/d(out).  dq: gradient of the normalised vector,
// dd: of the direction, dy: of the normalised norm (its batch coupling is applied by act_bwd_finish).
struct Loc { float n, xhat, y, s, dy, dq[3], dd[3]; };
__device__ __forceinline__ void act_bwd_local(const float (&p)[3], const float (&d)[3], const Bn &b, const float (&g)[3], Loc &L) {
    L.n = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + VN_EPS;
    L.xhat = (L.n - b.mu) * b.rstd;
    L.y = L.xhat * b.gam + b.bet;
    L.s = L.y / L.n;
    const float q0 = L.s * p[0], q1 = L.s * p[1], q2 = L.s * p[2];
    const float dot = q0 * d[0] + q1 * d[1] + q2 * d[2];
    if (dot < 0.f) {
        const float dsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + VN_EPS;
        const float c = 0.8f * dot / dsq, gd = g[0] * d[0] + g[1] * d[1] + g[2] * d[2];
        const float ddot = -0.8f * gd / dsq, ddsq2 = 2.f * 0.8f * gd * dot / (dsq * dsq);
        L.dq[0] = g[0] + ddot * d[0]; L.dq[1] = g[1] + ddot * d[1]; L.dq[2] = g[2] + ddot * d[2];
        L.dd[0] = -c * g[0] + ddot * q0 + ddsq2 * d[0];
        L.dd[1] = -c * g[1] + ddot * q1 + ddsq2 * d[1];
        L.dd[2] = -c * g[2] + ddot * q2 + ddsq2 * d[2];
    } else {
        L.dq[0] = g[0]; L.dq[1] = g[1]; L.dq[2] = g[2];
        L.dd[0] = L.dd[1] = L.dd[2] = 0.f;
    }
    L.dy = (L.dq[0] * p[0] + L.dq[1] * p[1] + L.dq[2] * p[2]) / L.n;
}
// dp from the local part and the channel's batch means mdy = mean(dy), mdyx = mean(dy xhat) (BatchNorm backward)
__device__ __forceinline__ void act_bwd_finish(const float (&p)[3], const Loc &L, const Bn &b, float mdy, float mdyx, float (&dp)[3]) {
    const float dn = b.gam * b.rstd * (L.dy - mdy - L.xhat * mdyx) - L.dy * L.y / L.n;
    const float pn = L.n - VN_EPS, f = pn > 0.f ? dn / pn : 0.f;
    dp[0] = L.s * L.dq[0] + f * p[0]; dp[1] = L.s * L.dq[1] + f * p[1]; dp[2] = L.s * L.dq[2] + f * p[2];
}

// (sum a, sum b) of the block's lanes -> dst[v], dst[NV + v] in fp64, fixed order.  All 256 threads must call it.
template <int NV>
__device__ __forceinline__ void block_sums(const float (&a)[NV], const float (&b)[NV], bool on, double *dst) {
    __shared__ double red[4][2 * NV];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int v = 0; v < 2 * NV; ++v) {
        double x = on ? (double)(v < NV ? a[v] : b[v - NV]) : 0.0;
        for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
        if (lane == 0) red[wave][v] = x;
    }
    __syncthreads();
    for (int v = tid; v < 2 * NV; v += 256) dst[v] = (red[0][v] + red[1][v]) + (red[2][v] + red[3][v]);
}

// s1[o] += u, s2[o] += v for a wave-uniform runtime o: a select per slot keeps the arrays in registers (an indexed access
// would move them to scratch, a fully unrolled channel loop hoists ~900 scalar weight loads)
__device__ __forceinline__ void acc_at(float (&s1)[VC], float (&s2)[VC], int o, float u, float v) {
#pragma unroll
    for (int q = 0; q < VC; ++q) {
        s1[q] += q == o ? u : 0.f;
        s2[q] += q == o ? v : 0.f;
    }
}

enum { M_STAT_A, M_STAT_B, M_BWD1, M_BWD2, M_BWD3 };
struct EdgeArgs {
    const float *T;            // premap rows [A | Ad | U | Ud] of the fragments, 4 * VROW floats per point
    const int32_t *idx;        // [pts][20], cloud-local
    int N;
    long long npts;            // points of this launch
    const float *recA, *recB;  // stat records of layers a and b
    const float *wb;           // packed conv_b: [21][22] feature map, [21][22] direction map
    const float *dX;           // gradient of the pooled output, component-major [pts][3][64]
    double *partial;           // [block][2][21]
    float *Gb, *Hb;            // layer b's weight-gradient operands, rows (edge, k): [dp_b | dd_b] (GB_LD), h (H_LD)
    float *E;                  // [edge][E_LD]: dp_a (63) | pad | dd_a (63) | pad
};

// One thread per point, its 20 edges in turn; MODE selects the pass (see the file header).
template <int MODE, bool HAS_B>
__global__ __launch_bounds__(256) void k_pt_edge(EdgeArgs a) {
    const long long p0 = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = p0 < a.npts;
    if (MODE == M_BWD3 && !on) return;                     // (the other passes keep every lane for the block sums)
    const long long p = on ? p0 : a.npts - 1;
    const long long base = (p / a.N) * a.N;
    float s1[VC], s2[VC];
#pragma unroll
    for (int c = 0; c < VC; ++c) s1[c] = s2[c] = 0.f;
    const float *ti = a.T + p * 4 * VROW;
    const float *gx = a.dX + p * 3 * VROW;
    const float rk = 1.f / (float)KNN;
#pragma unroll 1
    for (int r = 0; r < KNN; ++r) {
        const long long e = p * KNN + r;
        const float *tj = a.T + (base + a.idx[e]) * 4 * VROW;
        if constexpr (!HAS_B || MODE == M_STAT_A) {
#pragma unroll
            for (int c = 0; c < VC; ++c) {
                float pp[3], dd[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { pp[k] = tj[c * 3 + k] + ti[2 * VROW + c * 3 + k]; dd[k] = tj[VROW + c * 3 + k] + ti[3 * VROW + c * 3 + k]; }
                if constexpr (MODE == M_STAT_A) {
                    const float n = sqrtf(pp[0] * pp[0] + pp[1] * pp[1] + pp[2] * pp[2]) + VN_EPS;
                    s1[c] += n; s2[c] += n * n;
                } else {
                    const float g[3] = {gx[c] * rk, gx[VROW + c] * rk, gx[2 * VROW + c] * rk};
                    const Bn b = bn_at(a.recA, c);
                    Loc L;
                    act_bwd_local(pp, dd, b, g, L);
                    if constexpr (MODE == M_BWD1) { s1[c] += L.dy; s2[c] += L.dy * L.xhat; }
                    else if constexpr (MODE == M_BWD3) {
                        float dp[3];
                        act_bwd_finish(pp, L, b, a.recA[R_MDY * CMAX + c], a.recA[R_MDYX * CMAX + c], dp);
                        float *ee = a.E + e * E_LD;
#pragma unroll
                        for (int k = 0; k < 3; ++k) { ee[c * 3 + k] = dp[k]; ee[VROW + c * 3 + k] = L.dd[k]; }
                    }
                }
            }
            if constexpr (MODE == M_BWD3) { a.E[e * E_LD + V3] = 0.f; a.E[e * E_LD + VROW + V3] = 0.f; }
        } else {
            float h[V3];
#pragma unroll
            for (int c = 0; c < VC; ++c) {
                float pp[3], dd[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { pp[k] = tj[c * 3 + k] + ti[2 * VROW + c * 3 + k]; dd[k] = tj[VROW + c * 3 + k] + ti[3 * VROW + c * 3 + k]; }
                act_fwd(pp, dd, bn_at(a.recA, c));
#pragma unroll
                for (int k = 0; k < 3; ++k) h[c * 3 + k] = pp[k];
            }
            float dh[V3];
#pragma unroll
            for (int i = 0; i < V3; ++i) dh[i] = 0.f;
#pragma unroll 1
            for (int o = 0; o < VC; ++o) {
                const float *wf = a.wb + o * (VC + 1), *wd = a.wb + VC * (VC + 1) + o * (VC + 1);
                float pb[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < VC; ++c) {
                    const float f = wf[c], g = wd[c];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { pb[k] += f * h[c * 3 + k]; db[k] += g * h[c * 3 + k]; }
                }
                if constexpr (MODE == M_STAT_B) {
                    const float n = sqrtf(pb[0] * pb[0] + pb[1] * pb[1] + pb[2] * pb[2]) + VN_EPS;
                    acc_at(s1, s2, o, n, n * n);
                } else {
                    const float g[3] = {gx[o] * rk, gx[VROW + o] * rk, gx[2 * VROW + o] * rk};
                    const Bn b = bn_at(a.recB, o);
                    Loc L;
                    act_bwd_local(pb, db, b, g, L);
                    if constexpr (MODE == M_BWD1) acc_at(s1, s2, o, L.dy, L.dy * L.xhat);
                    else {
                        float dp[3];
                        act_bwd_finish(pb, L, b, a.recB[R_MDY * CMAX + o], a.recB[R_MDYX * CMAX + o], dp);
                        if (MODE == M_BWD2 && on) {
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                a.Gb[(e * 3 + k) * GB_LD + o] = dp[k];
                                a.Gb[(e * 3 + k) * GB_LD + VC + o] = L.dd[k];
                            }
                        }
#pragma unroll
                        for (int c = 0; c < VC; ++c) {
                            const float f = wf[c], g2 = wd[c];
#pragma unroll
                            for (int k = 0; k < 3; ++k) dh[c * 3 + k] += f * dp[k] + g2 * L.dd[k];
                        }
                    }
                }
            }
            if constexpr (MODE == M_BWD2 || MODE == M_BWD3) {
                if (MODE == M_BWD2 && on) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int c = 0; c < VC; ++c) a.Hb[(e * 3 + k) * H_LD + c] = h[c * 3 + k];
                }
#pragma unroll
                for (int c = 0; c < VC; ++c) {
                    float pp[3], dd[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { pp[k] = tj[c * 3 + k] + ti[2 * VROW + c * 3 + k]; dd[k] = tj[VROW + c * 3 + k] + ti[3 * VROW + c * 3 + k]; }
                    const float g[3] = {dh[c * 3], dh[c * 3 + 1], dh[c * 3 + 2]};
                    const Bn b = bn_at(a.recA, c);
                    Loc L;
                    act_bwd_local(pp, dd, b, g, L);
                    if constexpr (MODE == M_BWD2) { s1[c] += L.dy; s2[c] += L.dy * L.xhat; }
                    else {
                        float dp[3];
                        act_bwd_finish(pp, L, b, a.recA[R_MDY * CMAX + c], a.recA[R_MDYX * CMAX + c], dp);
                        float *ee = a.E + e * E_LD;
#pragma unroll
                        for (int k = 0; k < 3; ++k) { ee[c * 3 + k] = dp[k]; ee[VROW + c * 3 + k] = L.dd[k]; }
                    }
                }
                if constexpr (MODE == M_BWD3) { a.E[e * E_LD + V3] = 0.f; a.E[e * E_LD + VROW + V3] = 0.f; }
            }
        }
    }
    if constexpr (MODE != M_BWD3) block_sums<VC>(s1, s2, on, a.partial + (size_t)blockIdx.x * 2 * VC);
}

// conv6 over cat(x1, x2, x3), one thread per point (vn_dgcnn.py:61, one shared direction).  STAT: sums of the norm and its
// square; BWD1: sums of dy, dy xhat; BWD2: rows (point, k) of G6 = [dp6 (feat) | dd6] and of F = the input, component-major.
enum { C6_STAT, C6_BWD1, C6_BWD2 };
template <int MODE>
__global__ __launch_bounds__(256) void k_c6(const float *__restrict__ X1, const float *__restrict__ X2, const float *__restrict__ X3,
                                            const float *__restrict__ w6, int feat, int N, long long npts, const float *__restrict__ rec,
                                            const float *__restrict__ dm, double *partial, float *G6, int g6ld, float *F) {
    __shared__ double red[4][2 * CMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long p0 = (long long)blockIdx.x * 256 + tid;
    const bool on = p0 < npts;
    const long long p = on ? p0 : npts - 1;
    float f[3 * V3];
#pragma unroll
    for (int e = 0; e < V3; ++e) { f[e] = X1[p * VROW + e]; f[V3 + e] = X2[p * VROW + e]; f[2 * V3 + e] = X3[p * VROW + e]; }
    const float *wd = w6 + (size_t)feat * V3;
    float d[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < V3; ++c) { const float w = wd[c]; d[0] += w * f[c * 3]; d[1] += w * f[c * 3 + 1]; d[2] += w * f[c * 3 + 2]; }
    const float *gm = dm + (p / N) * feat * 3;
    const float rn = 1.f / (float)N;
    float dd6[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
    for (int o = 0; o < feat; ++o) {
        const float *w = w6 + (size_t)o * V3;
        float pp[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < V3; ++c) { const float wv = w[c]; pp[0] += wv * f[c * 3]; pp[1] += wv * f[c * 3 + 1]; pp[2] += wv * f[c * 3 + 2]; }
        float u = 0.f, v = 0.f;
        if constexpr (MODE == C6_STAT) {
            u = sqrtf(pp[0] * pp[0] + pp[1] * pp[1] + pp[2] * pp[2]) + VN_EPS;
            v = u * u;
        } else {
            const float g[3] = {gm[o * 3] * rn, gm[o * 3 + 1] * rn, gm[o * 3 + 2] * rn};
            const Bn b = bn_at(rec, o);
            Loc L;
            act_bwd_local(pp, d, b, g, L);
            if constexpr (MODE == C6_BWD1) { u = L.dy; v = L.dy * L.xhat; }
            else {
                float dp[3];
                act_bwd_finish(pp, L, b, rec[R_MDY * CMAX + o], rec[R_MDYX * CMAX + o], dp);
                dd6[0] += L.dd[0]; dd6[1] += L.dd[1]; dd6[2] += L.dd[2];
                if (on) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) G6[(p * 3 + k) * g6ld + o] = dp[k];
                }
            }
        }
        if constexpr (MODE != C6_BWD2) {
            // (a wave's 64 points in fp32, then fp64: every channel's sum has P*N terms)
            if (!on) u = v = 0.f;
            for (int off = 32; off; off >>= 1) { u += __shfl_xor(u, off); v += __shfl_xor(v, off); }
            if (lane == 0) { red[wave][o] = u; red[wave][CMAX + o] = v; }
        }
    }
    if constexpr (MODE == C6_BWD2) {
        if (!on) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            G6[(p * 3 + k) * g6ld + feat] = dd6[k];
            float *fr = F + (p * 3 + k) * VROW;
#pragma unroll
            for (int c = 0; c < V3; ++c) fr[c] = f[c * 3 + k];
            fr[V3] = 0.f;
        }
    } else {
        __syncthreads();
        double *dst = partial + (size_t)blockIdx.x * 2 * feat;
        for (int v = tid; v < 2 * feat; v += 256) {
            const int o = v < feat ? v : v - feat, s = v < feat ? 0 : CMAX;
            dst[v] = (red[0][s + o] + red[1][s + o]) + (red[2][s + o] + red[3][s + o]);
        }
    }
}

// d(cat(x1, x2, x3)) of row (point, k) = W6^T dp6 + w_dir^T dd6  -> the three component-major gradient maps (written)
__global__ __launch_bounds__(256) void k_c6_dx(const float *__restrict__ G6, int g6ld, const float *__restrict__ w6, int feat,
                                               long long rows, float *dX1, float *dX2, float *dX3) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float acc[V3];
#pragma unroll
    for (int c = 0; c < V3; ++c) acc[c] = 0.f;
    const float *g = G6 + row * g6ld;
#pragma unroll 1
    for (int o = 0; o <= feat; ++o) {                      // o == feat: the direction map (row feat of the packed blob)
        const float gv = g[o];
        const float *w = w6 + (size_t)o * V3;
#pragma unroll
        for (int c = 0; c < V3; ++c) acc[c] += w[c] * gv;
    }
#pragma unroll
    for (int c = 0; c < VC; ++c) { dX1[row * VROW + c] = acc[c]; dX2[row * VROW + c] = acc[VC + c]; dX3[row * VROW + c] = acc[2 * VC + c]; }
    dX1[row * VROW + VC] = 0.f; dX2[row * VROW + VC] = 0.f; dX3[row * VROW + VC] = 0.f;
}

// per-channel statistics -> record, scale / shift slots of the packed blob, updated running statistics (torch BatchNorm:
// biased variance normalises, the running variance takes the unbiased one).  One block per channel, fixed order.
__device__ double block_sum_d(double x, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = x;
    __syncthreads();
    for (int s = 128; s; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(256) void k_bn_fin_fwd(const double *__restrict__ partial, int nblk, int C, double count,
                                                    const float *__restrict__ gamma, const float *__restrict__ beta, float mom,
                                                    float eps, const float *__restrict__ rm, const float *__restrict__ rv,
                                                    float *rec, float *run_out, float *ss, int ss_ld) {
    __shared__ double sh[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int k = tid; k < nblk; k += 256) { a += partial[(size_t)k * 2 * C + c]; b += partial[(size_t)k * 2 * C + C + c]; }
    a = block_sum_d(a, sh);
    b = block_sum_d(b, sh);
    if (tid) return;
    const double mean = a / count;
    double var = b / count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    rec[R_MEAN * CMAX + c] = (float)mean;
    rec[R_RSTD * CMAX + c] = (float)rstd;
    rec[R_GAMMA * CMAX + c] = gamma[c];
    rec[R_BETA * CMAX + c] = beta[c];
    if (ss) {
        const double sc = (double)gamma[c] * rstd;
        ss[c] = (float)sc;
        ss[ss_ld + c] = (float)((double)beta[c] - mean * sc);
    }
    const double m = (double)mom;
    run_out[c] = (float)((1.0 - m) * (double)rm[c] + m * mean);
    run_out[CMAX + c] = (float)((1.0 - m) * (double)rv[c] + m * var * count / (count - 1.0));
}
// backward sums -> record means; dgamma += sum dy xhat, dbeta += sum dy
__global__ __launch_bounds__(256) void k_bn_fin_bwd(const double *__restrict__ partial, int nblk, int C, double count, float *rec,
                                                    float *dgamma, float *dbeta) {
    __shared__ double sh[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int k = tid; k < nblk; k += 256) { a += partial[(size_t)k * 2 * C + c]; b += partial[(size_t)k * 2 * C + C + c]; }
    a = block_sum_d(a, sh);
    b = block_sum_d(b, sh);
    if (tid) return;
    rec[R_MDY * CMAX + c] = (float)(a / count);
    rec[R_MDYX * CMAX + c] = (float)(b / count);
    dgamma[c] += (float)b;
    dbeta[c] += (float)a;
}

// VnInv (vn_layers.py:176-206, dim 3): one VNLinearLeakyReLU over [P, Cin, 3].  Only its running statistics are used.
__global__ __launch_bounds__(256) void k_vn_lin(int P, int Cin, int Cout, const float *__restrict__ X, int ldx,
                                                const float *__restrict__ Wf, const float *__restrict__ Wd, float *Pout, float *Dout) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * Cout) return;
    const int p = t / Cout, o = t - p * Cout;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < Cin; ++c) {
        const float f = Wf[(size_t)o * Cin + c], g = Wd[(size_t)o * Cin + c];
        const float *x = X + (size_t)p * ldx + c * 3;
        for (int k = 0; k < 3; ++k) { a[k] += f * x[k]; b[k] += g * x[k]; }
    }
    for (int k = 0; k < 3; ++k) { Pout[(size_t)t * 3 + k] = a[k]; Dout[(size_t)t * 3 + k] = b[k]; }
}
__global__ __launch_bounds__(256) void k_vn_stat(int P, int Cout, const float *__restrict__ Pm, double *partial) {
    __shared__ double sh[256];
    const int o = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int p = tid; p < P; p += 256) {
        const float *v = Pm + ((size_t)p * Cout + o) * 3;
        const double n = (double)(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + VN_EPS);
        a += n; b += n * n;
    }
    a = block_sum_d(a, sh);
    b = block_sum_d(b, sh);
    if (tid == 0) { partial[o] = a; partial[Cout + o] = b; }
}
__global__ __launch_bounds__(256) void k_vn_apply(int P, int Cout, const float *__restrict__ Pm, const float *__restrict__ Dm,
                                                  const float *__restrict__ rec, float *Y) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P * Cout) return;
    const int o = t % Cout;
    float p[3] = {Pm[(size_t)t * 3], Pm[(size_t)t * 3 + 1], Pm[(size_t)t * 3 + 2]};
    const float d[3] = {Dm[(size_t)t * 3], Dm[(size_t)t * 3 + 1], Dm[(size_t)t * 3 + 2]};
    act_fwd(p, d, bn_at(rec, o));
    for (int k = 0; k < 3; ++k) Y[(size_t)t * 3 + k] = p[k];
}

// gradient of the pooled map m [feat][3] of every fragment from the output gradient (vn_dgcnn.py:62-73): the output is m
// twice (inv = 0), or linear0(mean over the 2 feat channels of [m, m]) (inv = 1)
__global__ __launch_bounds__(256) void k_head_bwd(const float *__restrict__ G, int ldg, int inv, int feat, const float *__restrict__ lin0,
                                                  float *dm) {
    __shared__ float red[3][256];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float *g = G + (size_t)cl * ldg;
    float *d = dm + (size_t)cl * feat * 3;
    if (!inv) {
        for (int e = tid; e < feat * 3; e += 256) d[e] = g[e] + g[feat * 3 + e];
        return;
    }
    float s[3] = {0.f, 0.f, 0.f};
    for (int o = tid; o < 2 * feat; o += 256)
        for (int k = 0; k < 3; ++k) s[k] += g[o] * lin0[o * 3 + k];
    for (int k = 0; k < 3; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int w = 128; w; w >>= 1) {
        if (tid < w) for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + w];
        __syncthreads();
    }
    for (int e = tid; e < feat * 3; e += 256) d[e] = red[e % 3][0] / (float)feat;
}
// linear0's gradients (inv): dW0[o][k] += sum_p G[p][o] xbar_p[k], db0[o] += sum_p G[p][o]; xbar_p = mean over channels of m
__global__ __launch_bounds__(256) void k_lin0_grad(int P, const float *__restrict__ G, int ldg, const float *__restrict__ M, int ldm,
                                                   int feat, float *dW0, float *db0) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= 2 * feat) return;
    float w[3] = {0.f, 0.f, 0.f}, b = 0.f;
    for (int p = 0; p < P; ++p) {
        const float *m = M + (size_t)p * ldm;
        float x[3] = {0.f, 0.f, 0.f};
        for (int c = 0; c < feat; ++c) for (int k = 0; k < 3; ++k) x[k] += m[c * 3 + k];
        const float gv = G[(size_t)p * ldg + o];
        for (int k = 0; k < 3; ++k) w[k] += gv * (x[k] / (float)feat);
        b += gv;
    }
    for (int k = 0; k < 3; ++k) dW0[o * 3 + k] += w[k];
    db0[o] += b;
}

// reverse adjacency of a launch's kNN lists: for every point the edges (source point * 20 + rank) that end in it, ascending
__global__ void k_rev_count(long long nedge, int N, const int32_t *__restrict__ idx, int32_t *cnt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nedge) return;
    atomicAdd(&cnt[(e / KNN / N) * N + idx[e]], 1);
}
__global__ __launch_bounds__(256) void k_rev_scan(int N, const int32_t *__restrict__ cnt, int32_t *ptr, int32_t *cur) {
    __shared__ int32_t part[257];
    const int cl = blockIdx.x, tid = threadIdx.x, per = (N + 255) / 256;
    const int32_t *c = cnt + (size_t)cl * N;
    int s = 0;
    for (int i = tid * per; i < min(N, (tid + 1) * per); ++i) s += c[i];
    part[tid + 1] = s;
    __syncthreads();
    if (tid == 0) { part[0] = 0; for (int i = 1; i <= 256; ++i) part[i] += part[i - 1]; }
    __syncthreads();
    int o = cl * N * KNN + part[tid];
    for (int i = tid * per; i < min(N, (tid + 1) * per); ++i) { ptr[(size_t)cl * N + i] = o; cur[(size_t)cl * N + i] = o; o += c[i]; }
}
__global__ void k_rev_fill(long long nedge, int N, const int32_t *__restrict__ idx, int32_t *cur, int32_t *rev) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nedge) return;
    rev[atomicAdd(&cur[(e / KNN / N) * N + idx[e]], 1)] = (int32_t)e;
}
__global__ void k_rev_sort(long long npts, const int32_t *__restrict__ ptr, const int32_t *__restrict__ cnt, int32_t *rev) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= npts) return;
    int32_t *r = rev + ptr[j];
    const int n = cnt[j];
    for (int a = 1; a < n; ++a) {
        const int32_t v = r[a];
        int b = a - 1;
        while (b >= 0 && r[b] > v) { r[b + 1] = r[b]; --b; }
        r[b + 1] = v;
    }
}

// Premap backward of one point j: dT = [dA | dAd | dU | dUd], dA_j = sum of dp_a over the edges INTO j (reverse adjacency,
// ascending edge id), dU_j over j's own 20 edges.  dx_j = Wm^T dT (added into the previous stage's gradient map, or the point
// gradient for C = 1); rows (j, k) of dT and of x, component-major, for the weight GEMM.
template <int C>
__global__ __launch_bounds__(256) void k_gather(long long npts, const float *__restrict__ E, const int32_t *__restrict__ ptr,
                                                const int32_t *__restrict__ cnt, const int32_t *__restrict__ rev,
                                                const float *__restrict__ Wm, const float *__restrict__ X, int ldx, float *dXp,
                                                float *dTc, float *Xc) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= npts) return;
    float dx[C * 3];
#pragma unroll
    for (int i = 0; i < C * 3; ++i) dx[i] = 0.f;
#pragma unroll 1
    for (int m = 0; m < 4; ++m) {
        float acc[V3];
#pragma unroll
        for (int i = 0; i < V3; ++i) acc[i] = 0.f;
        const int seg = (m & 1) * VROW;
        if (m < 2) {
            const int32_t *r = rev + ptr[j];
            const int n = cnt[j];
#pragma unroll 1
            for (int q = 0; q < n; ++q) {
                const float *ee = E + (long long)r[q] * E_LD + seg;
#pragma unroll
                for (int i = 0; i < V3; ++i) acc[i] += ee[i];
            }
        } else {
#pragma unroll 1
            for (int q = 0; q < KNN; ++q) {
                const float *ee = E + (j * KNN + q) * E_LD + seg;
#pragma unroll
                for (int i = 0; i < V3; ++i) acc[i] += ee[i];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int o = 0; o < VC; ++o) dTc[(j * 3 + k) * DT_LD + m * VC + o] = acc[o * 3 + k];
#pragma unroll
        for (int o = 0; o < VC; ++o) {
            const float *w = Wm + (m * VC + o) * C;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) dx[c * 3 + k] += w[c] * acc[o * 3 + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if constexpr (C == 1) dXp[j * 3 + k] += dx[k];
            else dXp[(j * 3 + k) * VROW + c] += dx[c * 3 + k];
            Xc[(j * 3 + k) * XC_LD + c] = X[j * ldx + c * 3 + k];
        }
}

// dWm [4][21][C] (the premap blocks A, Ad, U, Ud) -> map_to_feat / map_to_dir gradients [21][2C]:
// W[:, :C] feeds A (x_j - x_i) and U = (W[:, C:] - W[:, :C]) x_i, so dW[:, :C] = dWm_A - dWm_U, dW[:, C:] = dWm_U
__global__ void k_premap_wgrad(int C, const float *__restrict__ dWm, float *dwf, float *dwd) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= VC * C) return;
    const int o = t / C, c = t - o * C;
    for (int s = 0; s < 2; ++s) {
        float *d = s ? dwd : dwf;
        const float a = dWm[(s * VC + o) * C + c], u = dWm[((2 + s) * VC + o) * C + c];
        d[o * 2 * C + c] += a - u;
        d[o * 2 * C + C + c] += u;
    }
}

// ---- layouts --------------------------------------------------------------------------------------------------------
struct StateLayout {
    int32_t *idx[3];
    float *X[3], *rec, *M;
    size_t bytes;
};
StateLayout state_layout(void *base, int P, int N, int feat) {
    StateLayout s;
    char *q = (char *)base;
    const size_t pts = (size_t)P * N;
    auto take = [&](size_t b) { char *r = q; q += align_up(b, 256); return r; };
    for (int i = 0; i < 3; ++i) s.idx[i] = (int32_t *)take(pts * KNN * 4);
    for (int i = 0; i < 3; ++i) s.X[i] = (float *)take(pts * VROW * 4);
    s.rec = (float *)take((size_t)NL * REC * CMAX * 4);
    s.M = (float *)take((size_t)P * 6 * feat * 4);
    s.bytes = (size_t)(q - (char *)base);
    return s;
}
int g6_ld(int feat) { return (feat + 1 + 3) & ~3; }
size_t nblk_total(int P, int N, int chunk) {
    size_t n = 0;
    for (int p0 = 0; p0 < P; p0 += chunk) n += ((size_t)(P - p0 < chunk ? P - p0 : chunk) * N + 255) / 256;
    return n;
}
struct WsLayout {
    float *T, *dX[3], *dm, *xn[2], *c6part, *vP, *vD, *vY, *dWm, *gpart;
    double *partial;
    // per chunk
    float *Gb, *Hb, *E, *dTc, *Xc, *G6, *F;
    int32_t *cnt, *ptr, *cur, *rev;
    size_t bytes;
};
WsLayout ws_layout(void *base, int P, int N, int chunk, int feat) {
    WsLayout w;
    char *q = (char *)base;
    const size_t pts = (size_t)P * N, cp = (size_t)chunk * N, ce = cp * KNN;
    auto take = [&](size_t b) { char *r = q; q += align_up(b, 256); return r; };
    w.T = (float *)take(pts * 4 * VROW * 4);
    for (int i = 0; i < 3; ++i) w.dX[i] = (float *)take(pts * 3 * VROW * 4);
    w.dm = (float *)take((size_t)P * feat * 3 * 4);
    for (int i = 0; i < 2; ++i) w.xn[i] = (float *)take(pts * 4);
    w.c6part = (float *)take((size_t)P * ((N + 255) / 256) * feat * 3 * 4);
    w.vP = (float *)take((size_t)P * feat * 3 * 4);
    w.vD = (float *)take((size_t)P * feat * 3 * 4);
    w.vY = (float *)take((size_t)P * feat * 3 * 4);
    w.dWm = (float *)take((size_t)4 * VC * VC * 4);
    w.gpart = (float *)take(GEMM_PART * 4);
    const size_t nb = nblk_total(P, N, 1) > nblk_total(P, N, chunk) ? nblk_total(P, N, 1) : nblk_total(P, N, chunk);
    w.partial = (double *)take((nb + 1) * 2 * CMAX * 8);
    w.Gb = (float *)take(ce * 3 * GB_LD * 4);
    w.Hb = (float *)take(ce * 3 * H_LD * 4);
    w.E = (float *)take(ce * E_LD * 4);
    w.dTc = (float *)take(cp * 3 * DT_LD * 4);
    w.Xc = (float *)take(cp * 3 * XC_LD * 4);
    w.G6 = (float *)take(cp * 3 * g6_ld(feat) * 4);
    w.F = (float *)take(cp * 3 * VROW * 4);
    w.cnt = (int32_t *)take(cp * 4);
    w.ptr = (int32_t *)take(cp * 4);
    w.cur = (int32_t *)take(cp * 4);
    w.rev = (int32_t *)take(ce * 4);
    w.bytes = (size_t)(q - (char *)base);
    return w;
}

int check_weights(const da_pcd_train_weights *w, int P, int N, int inv) {
    DA_REQUIRE(w && P >= 2 && N >= KNN, "da_pcd_train: need >= 2 fragments (batch statistics) of >= %d points", KNN);
    DA_REQUIRE(w->feat_dim >= 2 && w->feat_dim <= 128 && w->feat_dim % 2 == 0, "da_pcd_train: feat_dim %d outside 2..128 (even)", w->feat_dim);
    for (int s = 0; s < 3; ++s)
        DA_REQUIRE(w->premap[s] && w->bn_a[s] && (s == 2 || w->conv_b[s]), "da_pcd_train: stage %d weights missing", s);
    DA_REQUIRE(w->conv6 && (!inv || w->linear0), "da_pcd_train: conv6 / linear0 missing");
    for (int l = 0; l < NL; ++l)
        DA_REQUIRE(w->gamma[l] && w->beta[l] && w->running_mean[l] && w->running_var[l], "da_pcd_train: BatchNorm %d missing", l);
    DA_REQUIRE(w->inv_wf[0] && w->inv_wf[1] && w->inv_wd[0] && w->inv_wd[1], "da_pcd_train: VnInv weights missing");
    return 0;
}

// ---- launches: one helper per pass, shared by da_pcd_train_forward / _backward and by da_pcd_train_pass -------------------
int edge_launch(int mode, bool hb, const EdgeArgs &a, hipStream_t st) {
    const int nb = (int)((a.npts + 255) / 256);
    switch (mode) {
    case M_STAT_A:
        if (hb) k_pt_edge<M_STAT_A, true><<<nb, 256, 0, st>>>(a);
        else k_pt_edge<M_STAT_A, false><<<nb, 256, 0, st>>>(a);
        break;
    case M_STAT_B:
        DA_REQUIRE(hb, "da_pcd_train: the statistics of layer b need a layer b");
        k_pt_edge<M_STAT_B, true><<<nb, 256, 0, st>>>(a);
        break;
    case M_BWD1:
        if (hb) k_pt_edge<M_BWD1, true><<<nb, 256, 0, st>>>(a);
        else k_pt_edge<M_BWD1, false><<<nb, 256, 0, st>>>(a);
        break;
    case M_BWD2:
        DA_REQUIRE(hb, "da_pcd_train: the second backward pass needs a layer b");
        k_pt_edge<M_BWD2, true><<<nb, 256, 0, st>>>(a);
        break;
    case M_BWD3:
        if (hb) k_pt_edge<M_BWD3, true><<<nb, 256, 0, st>>>(a);
        else k_pt_edge<M_BWD3, false><<<nb, 256, 0, st>>>(a);
        break;
    default:
        DA_REQUIRE(false, "da_pcd_train: unknown edge pass %d", mode);
    }
    DA_LAUNCH_CHECK();
    return 0;
}
int c6_launch(int mode, const float *X1, const float *X2, const float *X3, const float *w6, int feat, int N, long long npts,
              const float *rec, const float *dm, double *partial, float *G6, int g6ld, float *F, hipStream_t st) {
    const int nb = (int)((npts + 255) / 256);
    if (mode == C6_STAT) k_c6<C6_STAT><<<nb, 256, 0, st>>>(X1, X2, X3, w6, feat, N, npts, rec, dm, partial, G6, g6ld, F);
    else if (mode == C6_BWD1) k_c6<C6_BWD1><<<nb, 256, 0, st>>>(X1, X2, X3, w6, feat, N, npts, rec, dm, partial, G6, g6ld, F);
    else k_c6<C6_BWD2><<<nb, 256, 0, st>>>(X1, X2, X3, w6, feat, N, npts, rec, dm, partial, G6, g6ld, F);
    DA_LAUNCH_CHECK();
    return 0;
}
int c6_dx_launch(const float *G6, int g6ld, const float *w6, int feat, long long rows, float *dX1, float *dX2, float *dX3,
                 hipStream_t st) {
    k_c6_dx<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(G6, g6ld, w6, feat, rows, dX1, dX2, dX3);
    DA_LAUNCH_CHECK();
    return 0;
}
int bn_fin_fwd_launch(const double *partial, int nb, int C, double count, const float *gamma, const float *beta, float mom, float eps,
                      const float *rm, const float *rv, float *rec, float *run_out, float *ss, int ss_ld, hipStream_t st) {
    k_bn_fin_fwd<<<C, 256, 0, st>>>(partial, nb, C, count, gamma, beta, mom, eps, rm, rv, rec, run_out, ss, ss_ld);
    DA_LAUNCH_CHECK();
    return 0;
}
int bn_fin_bwd_launch(const double *partial, int nb, int C, double count, float *rec, float *dgamma, float *dbeta, hipStream_t st) {
    k_bn_fin_bwd<<<C, 256, 0, st>>>(partial, nb, C, count, rec, dgamma, dbeta);
    DA_LAUNCH_CHECK();
    return 0;
}
// reverse adjacency of B clouds of N points: cnt, ptr [B N], rev [B N 20]; cur [B N]: the fill's cursors (scratch)
int rev_adj_launch(int B, int N, const int32_t *idx, int32_t *cnt, int32_t *ptr, int32_t *cur, int32_t *rev, hipStream_t st) {
    const long long cp = (long long)B * N, ne = cp * KNN;
    const unsigned ge = (unsigned)((ne + 255) / 256);
    DA_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)cp * 4, st));
    k_rev_count<<<ge, 256, 0, st>>>(ne, N, idx, cnt);
    DA_LAUNCH_CHECK();
    k_rev_scan<<<B, 256, 0, st>>>(N, cnt, ptr, cur);
    DA_LAUNCH_CHECK();
    k_rev_fill<<<ge, 256, 0, st>>>(ne, N, idx, cur, rev);
    DA_LAUNCH_CHECK();
    k_rev_sort<<<(int)((cp + 255) / 256), 256, 0, st>>>(cp, ptr, cnt, rev);
    DA_LAUNCH_CHECK();
    return 0;
}
int gather_launch(int C, long long cp, const float *E, const int32_t *ptr, const int32_t *cnt, const int32_t *rev, const float *Wm,
                  const float *X, int ldx, float *dXp, float *dTc, float *Xc, hipStream_t st) {
    const int nb = (int)((cp + 255) / 256);
    if (C == 1) k_gather<1><<<nb, 256, 0, st>>>(cp, E, ptr, cnt, rev, Wm, X, ldx, dXp, dTc, Xc);
    else k_gather<VC><<<nb, 256, 0, st>>>(cp, E, ptr, cnt, rev, Wm, X, ldx, dXp, dTc, Xc);
    DA_LAUNCH_CHECK();
    return 0;
}
int premap_wgrad_launch(int C, const float *dWm, float *dwf, float *dwd, hipStream_t st) {
    k_premap_wgrad<<<(VC * C + 255) / 256, 256, 0, st>>>(C, dWm, dwf, dwd);
    DA_LAUNCH_CHECK();
    return 0;
}
int head_bwd_launch(int P, const float *G, int ldg, int inv, int feat, const float *lin0, float *dm, hipStream_t st) {
    k_head_bwd<<<P, 256, 0, st>>>(G, ldg, inv, feat, lin0, dm);
    DA_LAUNCH_CHECK();
    return 0;
}
int lin0_grad_launch(int P, const float *G, int ldg, const float *M, int ldm, int feat, float *dW0, float *db0, hipStream_t st) {
    k_lin0_grad<<<(2 * feat + 255) / 256, 256, 0, st>>>(P, G, ldg, M, ldm, feat, dW0, db0);
    DA_LAUNCH_CHECK();
    return 0;
}
int vn_lin_launch(int P, int Cin, int Cout, const float *X, int ldx, const float *Wf, const float *Wd, float *Pm, float *Dm, hipStream_t st) {
    k_vn_lin<<<(P * Cout + 255) / 256, 256, 0, st>>>(P, Cin, Cout, X, ldx, Wf, Wd, Pm, Dm);
    DA_LAUNCH_CHECK();
    return 0;
}
int vn_stat_launch(int P, int Cout, const float *Pm, double *partial, hipStream_t st) {
    k_vn_stat<<<Cout, 256, 0, st>>>(P, Cout, Pm, partial);
    DA_LAUNCH_CHECK();
    return 0;
}
int vn_apply_launch(int P, int Cout, const float *Pm, const float *Dm, const float *rec, float *Y, hipStream_t st) {
    k_vn_apply<<<(P * Cout + 255) / 256, 256, 0, st>>>(P, Cout, Pm, Dm, rec, Y);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

size_t da_pcd_train_state_bytes(int n_parts, int n_points, int feat_dim) {
    return state_layout(nullptr, n_parts, n_points, feat_dim).bytes;
}

size_t da_pcd_train_workspace_bytes(int n_parts, int n_points, int chunk, int feat_dim) {
    if (chunk < 1) chunk = 1;
    if (chunk > n_parts) chunk = n_parts;
    return ws_layout(nullptr, n_parts, n_points, chunk, feat_dim).bytes;
}

int da_pcd_train_forward(const da_pcd_train_weights *w, int n_parts, int n_points, const float *points, int inv, float *out,
                         int ld_out, float *run_out, void *state, size_t state_bytes, void *workspace, size_t workspace_bytes,
                         void *stream) {
    if (int rc = check_weights(w, n_parts, n_points, inv)) return rc;
    const int P = n_parts, N = n_points, feat = w->feat_dim;
    DA_REQUIRE(points && out && run_out && state && workspace, "da_pcd_train_forward: null argument");
    DA_REQUIRE(ld_out >= (inv ? 2 * feat : 6 * feat), "da_pcd_train_forward: ld_out too small");
    DA_REQUIRE(state_bytes >= da_pcd_train_state_bytes(P, N, feat), "da_pcd_train_forward: state too small");
    DA_REQUIRE(workspace_bytes >= da_pcd_train_workspace_bytes(P, N, 1, feat), "da_pcd_train_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const StateLayout S = state_layout(state, P, N, feat);
    const WsLayout W = ws_layout(workspace, P, N, 1, feat);
    const long long pts = (long long)P * N;
    const int nblk = (int)((pts + 255) / 256);
    const double n_edge = (double)pts * KNN;
    auto fin = [&](int l, int C, int nb, double count, float *ss, int ss_ld) -> int {
        return bn_fin_fwd_launch(W.partial, nb, C, count, w->gamma[l], w->beta[l], w->momentum[l], w->eps[l], w->running_mean[l],
                                 w->running_var[l], S.rec + (size_t)l * REC * CMAX, run_out + (size_t)l * 2 * CMAX, ss, ss_ld, st);
    };
    int rc;
    for (int s = 0; s < 3; ++s) {
        const float *xin = s == 0 ? points : S.X[s - 1];
        const int ldx = s == 0 ? 3 : VROW, C = s == 0 ? 1 : VC;
        const int la = 2 * s, lb = 2 * s + 1;
        const bool hb = s < 2;
        if ((rc = pcd_knn_launch(P, N, s == 0 ? 3 : V3, xin, ldx, S.idx[s], s == 0 ? nullptr : W.xn[s - 1], st))) return rc;
        if ((rc = pcd_premap_launch(C, xin, ldx, w->premap[s], pts, W.T, st))) return rc;
        EdgeArgs a{};
        a.T = W.T; a.idx = S.idx[s]; a.N = N; a.npts = pts; a.partial = W.partial;
        a.recA = S.rec + (size_t)la * REC * CMAX;
        if ((rc = edge_launch(M_STAT_A, hb, a, st))) return rc;
        if ((rc = fin(la, VC, nblk, n_edge, w->bn_a[s], VC))) return rc;
        if (hb) {
            a.wb = w->conv_b[s];
            if ((rc = edge_launch(M_STAT_B, true, a, st))) return rc;
            if ((rc = fin(lb, VC, nblk, n_edge, w->conv_b[s] + 2 * VC * (VC + 1), VC))) return rc;
        }
        if ((rc = pcd_edge_launch(W.T, S.idx[s], w->bn_a[s], hb ? w->conv_b[s] : nullptr, N, P, S.X[s], s < 2 ? W.xn[s] : nullptr, st))) return rc;
    }
    // conv6 (BatchNorm1d over the P * N points), mean over points
    if ((rc = c6_launch(C6_STAT, S.X[0], S.X[1], S.X[2], w->conv6, feat, N, pts, nullptr, nullptr, W.partial, nullptr, 0, nullptr, st))) return rc;
    if ((rc = fin(5, feat, nblk, (double)pts, w->conv6 + (size_t)feat * V3 + V3, feat))) return rc;
    if ((rc = pcd_conv6_final_launch(S.X[0], S.X[1], S.X[2], w->conv6, feat, N, P, W.c6part, w->linear0, 0, S.M, 6 * feat, st))) return rc;
    if ((rc = pcd_conv6_final_launch(S.X[0], S.X[1], S.X[2], w->conv6, feat, N, P, W.c6part, w->linear0, inv, out, ld_out, st))) return rc;
    // VnInv (vn_dgcnn.py:67): vn1 over the pooled [P, 2 feat, 3], vn2 over its output -- BatchNorm1d over the P fragments
    const int cin[2] = {2 * feat, feat}, cout[2] = {feat, feat / 2};
    for (int v = 0; v < 2; ++v) {
        const float *X = v == 0 ? S.M : W.vY;
        const int ldx = v == 0 ? 6 * feat : feat * 3;
        if ((rc = vn_lin_launch(P, cin[v], cout[v], X, ldx, w->inv_wf[v], w->inv_wd[v], W.vP, W.vD, st))) return rc;
        if ((rc = vn_stat_launch(P, cout[v], W.vP, W.partial, st))) return rc;
        if ((rc = fin(6 + v, cout[v], 1, (double)P, nullptr, 0))) return rc;
        if (v == 0 && (rc = vn_apply_launch(P, cout[v], W.vP, W.vD, S.rec + (size_t)6 * REC * CMAX, W.vY, st))) return rc;
    }
    return 0;
}

int da_pcd_train_backward(const da_pcd_train_weights *w, int n_parts, int n_points, const float *points, int inv,
                          const float *grad_out, int ld_g, void *state, const da_pcd_train_grads *g, void *workspace,
                          size_t workspace_bytes, int chunk, void *stream) {
    if (int rc = check_weights(w, n_parts, n_points, inv)) return rc;
    const int P = n_parts, N = n_points, feat = w->feat_dim;
    if (chunk < 1) chunk = 1;
    if (chunk > P) chunk = P;
    DA_REQUIRE(points && grad_out && state && g && workspace, "da_pcd_train_backward: null argument");
    DA_REQUIRE(ld_g >= (inv ? 2 * feat : 6 * feat), "da_pcd_train_backward: ld_g too small");
    for (int l = 0; l < 6; ++l)
        DA_REQUIRE(g->wf[l] && g->wd[l] && g->gamma[l] && g->beta[l], "da_pcd_train_backward: gradient of layer %d missing", l);
    DA_REQUIRE(!inv || (g->linear0_w && g->linear0_b), "da_pcd_train_backward: linear0 gradients missing");
    DA_REQUIRE(workspace_bytes >= da_pcd_train_workspace_bytes(P, N, chunk, feat), "da_pcd_train_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const StateLayout S = state_layout(state, P, N, feat);
    const WsLayout W = ws_layout(workspace, P, N, chunk, feat);
    const long long pts = (long long)P * N;
    const int g6 = g6_ld(feat);
    float *rec = S.rec;
    int rc;
    // output -> gradient of the pooled map
    if ((rc = head_bwd_launch(P, grad_out, ld_g, inv, feat, w->linear0, W.dm, st))) return rc;
    if (inv && (rc = lin0_grad_launch(P, grad_out, ld_g, S.M, 6 * feat, feat, g->linear0_w, g->linear0_b, st))) return rc;
    // the chunks of a pass, each with its blocks' slots in W.partial (global block index: fixed summation order)
    auto chunks = [&](auto &&body) -> int {
        size_t boff = 0;
        for (int p0 = 0; p0 < P; p0 += chunk) {
            const int B = P - p0 < chunk ? P - p0 : chunk;
            const long long off = (long long)p0 * N, cp = (long long)B * N;
            const int nb = (int)((cp + 255) / 256);
            if (int rc2 = body(off, cp, nb, boff, B)) return rc2;
            boff += nb;
        }
        return 0;
    };
    const int nbt = (int)nblk_total(P, N, chunk);
    auto fin_bwd = [&](int l, int C, double count) -> int {
        return bn_fin_bwd_launch(W.partial, nbt, C, count, rec + (size_t)l * REC * CMAX, g->gamma[l], g->beta[l], st);
    };
    // conv6
    const float *rec6 = rec + (size_t)5 * REC * CMAX;
    if ((rc = chunks([&](long long off, long long cp, int, size_t boff, int) -> int {
             return c6_launch(C6_BWD1, S.X[0] + off * VROW, S.X[1] + off * VROW, S.X[2] + off * VROW, w->conv6, feat, N, cp, rec6,
                              W.dm + (off / N) * feat * 3, W.partial + boff * 2 * feat, nullptr, 0, nullptr, st);
         }))) return rc;
    if ((rc = fin_bwd(5, feat, (double)pts))) return rc;
    if ((rc = chunks([&](long long off, long long cp, int, size_t, int) -> int {
             int r2 = c6_launch(C6_BWD2, S.X[0] + off * VROW, S.X[1] + off * VROW, S.X[2] + off * VROW, w->conv6, feat, N, cp, rec6,
                                W.dm + (off / N) * feat * 3, nullptr, W.G6, g6, W.F, st);
             if (r2) return r2;
             const long long rows = cp * 3;
             if ((r2 = c6_dx_launch(W.G6, g6, w->conv6, feat, rows, W.dX[0] + off * 3 * VROW, W.dX[1] + off * 3 * VROW,
                                    W.dX[2] + off * 3 * VROW, st))) return r2;
             r2 = launch_gemm_tn((int)rows, feat, V3, W.G6, g6, W.F, VROW, g->wf[5], V3, W.gpart, st);
             return r2 ? r2 : launch_gemm_tn((int)rows, 1, V3, W.G6 + feat, g6, W.F, VROW, g->wd[5], V3, W.gpart, st);
         }))) return rc;
    // stages 3, 2, 1
    for (int s = 2; s >= 0; --s) {
        const float *xin = s == 0 ? points : S.X[s - 1];
        const int ldx = s == 0 ? 3 : VROW, C = s == 0 ? 1 : VC;
        const int la = 2 * s, lb = 2 * s + 1;
        const bool hb = s < 2;
        if ((rc = pcd_premap_launch(C, xin, ldx, w->premap[s], pts, W.T, st))) return rc;
        EdgeArgs a0{};
        a0.T = W.T; a0.idx = S.idx[s]; a0.N = N; a0.wb = hb ? w->conv_b[s] : nullptr;
        a0.recA = rec + (size_t)la * REC * CMAX; a0.recB = rec + (size_t)lb * REC * CMAX;
        a0.Gb = W.Gb; a0.Hb = W.Hb; a0.E = W.E;
        auto args = [&](long long off, long long cp, size_t boff) {
            EdgeArgs a = a0;
            a.T = W.T + off * 4 * VROW; a.idx = S.idx[s] + off * KNN; a.npts = cp; a.dX = W.dX[s] + off * 3 * VROW;
            a.partial = W.partial + boff * 2 * VC;
            return a;
        };
        // sums of the last layer's BatchNorm backward
        if ((rc = chunks([&](long long off, long long cp, int, size_t boff, int) -> int {
                 return edge_launch(M_BWD1, hb, args(off, cp, boff), st);
             }))) return rc;
        if ((rc = fin_bwd(hb ? lb : la, VC, (double)pts * KNN))) return rc;
        if (hb) {
            if ((rc = chunks([&](long long off, long long cp, int, size_t boff, int) -> int {
                     int r2 = edge_launch(M_BWD2, true, args(off, cp, boff), st);
                     if (r2) return r2;
                     const int rows = (int)(cp * KNN * 3);
                     r2 = launch_gemm_tn(rows, VC, VC, W.Gb, GB_LD, W.Hb, H_LD, g->wf[lb], VC, W.gpart, st);
                     return r2 ? r2 : launch_gemm_tn(rows, VC, VC, W.Gb + VC, GB_LD, W.Hb, H_LD, g->wd[lb], VC, W.gpart, st);
                 }))) return rc;
            if ((rc = fin_bwd(la, VC, (double)pts * KNN))) return rc;
        }
        DA_CHECK_HIP(hipMemsetAsync(W.dWm, 0, (size_t)4 * VC * C * 4, st));
        if ((rc = chunks([&](long long off, long long cp, int, size_t boff, int B) -> int {
                 const EdgeArgs a = args(off, cp, boff);
                 int r2 = edge_launch(M_BWD3, hb, a, st);
                 if (r2) return r2;
                 if ((r2 = rev_adj_launch(B, N, a.idx, W.cnt, W.ptr, W.cur, W.rev, st))) return r2;
                 float *dxp = s == 0 ? g->points : W.dX[s - 1] + off * 3 * VROW;
                 if (s == 0) {
                     if (dxp) dxp += off * 3;
                     else dxp = W.F;                       // point gradient not requested: a dead scratch target
                 }
                 if ((r2 = gather_launch(C, cp, W.E, W.ptr, W.cnt, W.rev, w->premap[s], xin + off * ldx, ldx, dxp, W.dTc, W.Xc, st))) return r2;
                 return launch_gemm_tn((int)(cp * 3), 4 * VC, C, W.dTc, DT_LD, W.Xc, XC_LD, W.dWm, C, W.gpart, st);
             }))) return rc;
        if ((rc = premap_wgrad_launch(C, W.dWm, g->wf[la], g->wd[la], st))) return rc;
    }
    return 0;
}

int da_pcd_train_pass(int pass, const da_pcd_pass_args *p, void *stream) {
    DA_REQUIRE(p, "da_pcd_train_pass: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int P = p->n_parts, N = p->n_points, feat = p->feat;
    const long long pts = (long long)P * N;
    auto sized = [&](bool lists) { return P >= 1 && N >= (lists ? KNN : 1) && pts * KNN * 3 <= 0x7fffffffLL; };
    auto feat_ok = [&]() { return feat >= 1 && feat <= 128; };
    switch (pass) {
    case DA_PCD_PASS_PREMAP:
        DA_REQUIRE(sized(false) && (p->cin == 1 || p->cin == VC) && p->x && p->w && p->T && p->ld_x >= 3 * p->cin, "da_pcd_train_pass: premap arguments");
        return pcd_premap_launch(p->cin, p->x, p->ld_x, p->w, pts, p->T, st);
    case DA_PCD_PASS_EDGE_STAT_A: case DA_PCD_PASS_EDGE_STAT_B: case DA_PCD_PASS_EDGE_BWD1: case DA_PCD_PASS_EDGE_BWD2:
    case DA_PCD_PASS_EDGE_BWD3: {
        const int mode = pass - DA_PCD_PASS_EDGE_STAT_A;      // M_STAT_A .. M_BWD3, same order
        const bool hb = p->has_b != 0, bwd = mode >= M_BWD1;
        DA_REQUIRE(sized(true) && p->T && p->idx, "da_pcd_train_pass: edge pass without T / idx");
        DA_REQUIRE(mode == M_BWD3 || p->partial, "da_pcd_train_pass: edge pass without partial");
        DA_REQUIRE(mode == M_STAT_A || p->rec_a, "da_pcd_train_pass: edge pass without rec_a");
        DA_REQUIRE(!hb || mode == M_STAT_A || p->w, "da_pcd_train_pass: edge pass without the conv_b blob");
        DA_REQUIRE(!bwd || (p->dX_in && (!hb || p->rec_b)), "da_pcd_train_pass: backward edge pass without dX_in / rec_b");
        DA_REQUIRE(mode != M_BWD2 || (p->Gb && p->Hb), "da_pcd_train_pass: BWD2 without Gb / Hb");
        DA_REQUIRE(mode != M_BWD3 || p->E, "da_pcd_train_pass: BWD3 without E");
        EdgeArgs a{};
        a.T = p->T; a.idx = p->idx; a.N = N; a.npts = pts; a.recA = p->rec_a; a.recB = p->rec_b; a.wb = hb ? p->w : nullptr;
        a.dX = p->dX_in; a.partial = p->partial; a.Gb = p->Gb; a.Hb = p->Hb; a.E = p->E;
        return edge_launch(mode, hb, a, st);
    }
    case DA_PCD_PASS_C6_STAT: case DA_PCD_PASS_C6_BWD1: case DA_PCD_PASS_C6_BWD2: {
        const int mode = pass - DA_PCD_PASS_C6_STAT;
        DA_REQUIRE(sized(false) && feat_ok() && p->X1 && p->X2 && p->X3 && p->w, "da_pcd_train_pass: conv6 arguments");
        DA_REQUIRE(mode == C6_BWD2 ? (p->G6 && p->F && p->ld_g >= feat + 1) : p->partial != nullptr, "da_pcd_train_pass: conv6 outputs");
        DA_REQUIRE(mode == C6_STAT || (p->rec_a && p->dm_in), "da_pcd_train_pass: conv6 backward without rec_a / dm_in");
        return c6_launch(mode, p->X1, p->X2, p->X3, p->w, feat, N, pts, p->rec_a, p->dm_in, p->partial, p->G6, p->ld_g, p->F, st);
    }
    case DA_PCD_PASS_C6_DX:
        DA_REQUIRE(sized(false) && feat_ok() && p->G6 && p->w && p->dX1 && p->dX2 && p->dX3 && p->ld_g >= feat + 1, "da_pcd_train_pass: c6_dx arguments");
        return c6_dx_launch(p->G6, p->ld_g, p->w, feat, pts * 3, p->dX1, p->dX2, p->dX3, st);
    case DA_PCD_PASS_BN_FIN_FWD:
        DA_REQUIRE(p->partial && p->nblk >= 1 && p->channels >= 1 && p->channels <= CMAX && p->count > 1.0 && p->gamma && p->beta &&
                       p->running_mean && p->running_var && p->rec_a && p->run_out && (!p->ss || p->ld_m >= p->channels),
                   "da_pcd_train_pass: bn_fin_fwd arguments");
        return bn_fin_fwd_launch(p->partial, p->nblk, p->channels, p->count, p->gamma, p->beta, p->momentum, p->eps, p->running_mean,
                                 p->running_var, p->rec_a, p->run_out, p->ss, p->ld_m, st);
    case DA_PCD_PASS_BN_FIN_BWD:
        DA_REQUIRE(p->partial && p->nblk >= 1 && p->channels >= 1 && p->channels <= CMAX && p->count >= 1.0 && p->rec_a && p->dgamma && p->dbeta,
                   "da_pcd_train_pass: bn_fin_bwd arguments");
        return bn_fin_bwd_launch(p->partial, p->nblk, p->channels, p->count, p->rec_a, p->dgamma, p->dbeta, st);
    case DA_PCD_PASS_REV_ADJ:
        DA_REQUIRE(sized(true) && p->idx && p->cnt && p->ptr && p->cur && p->rev, "da_pcd_train_pass: rev_adj arguments");
        return rev_adj_launch(P, N, p->idx, p->cnt, p->ptr, p->cur, p->rev, st);
    case DA_PCD_PASS_GATHER:
        DA_REQUIRE(sized(true) && (p->cin == 1 || p->cin == VC) && p->E && p->cnt && p->ptr && p->rev && p->w && p->x && p->ld_x >= 3 * p->cin &&
                       p->dXp && p->dTc && p->Xc, "da_pcd_train_pass: gather arguments");
        return gather_launch(p->cin, pts, p->E, p->ptr, p->cnt, p->rev, p->w, p->x, p->ld_x, p->dXp, p->dTc, p->Xc, st);
    case DA_PCD_PASS_PREMAP_WGRAD:
        DA_REQUIRE((p->cin == 1 || p->cin == VC) && p->dWm && p->dwf && p->dwd, "da_pcd_train_pass: premap_wgrad arguments");
        return premap_wgrad_launch(p->cin, p->dWm, p->dwf, p->dwd, st);
    case DA_PCD_PASS_HEAD_BWD:
        DA_REQUIRE(P >= 1 && feat_ok() && p->grad_out && p->dm && (!p->inv || p->w) && p->ld_g >= (p->inv ? 2 * feat : 6 * feat),
                   "da_pcd_train_pass: head_bwd arguments");
        return head_bwd_launch(P, p->grad_out, p->ld_g, p->inv, feat, p->w, p->dm, st);
    case DA_PCD_PASS_LIN0_GRAD:
        DA_REQUIRE(P >= 1 && feat_ok() && p->grad_out && p->x && p->dwf && p->dwd && p->ld_g >= 2 * feat && p->ld_x >= 3 * feat,
                   "da_pcd_train_pass: lin0_grad arguments");
        return lin0_grad_launch(P, p->grad_out, p->ld_g, p->x, p->ld_x, feat, p->dwf, p->dwd, st);
    case DA_PCD_PASS_VN_LIN:
        DA_REQUIRE(P >= 1 && p->vn_cin >= 1 && p->channels >= 1 && p->x && p->w && p->w2 && p->vP && p->vD && p->ld_x >= 3 * p->vn_cin,
                   "da_pcd_train_pass: vn_lin arguments");
        return vn_lin_launch(P, p->vn_cin, p->channels, p->x, p->ld_x, p->w, p->w2, p->vP, p->vD, st);
    case DA_PCD_PASS_VN_STAT:
        DA_REQUIRE(P >= 1 && p->channels >= 1 && p->vP && p->partial, "da_pcd_train_pass: vn_stat arguments");
        return vn_stat_launch(P, p->channels, p->vP, p->partial, st);
    case DA_PCD_PASS_VN_APPLY:
        DA_REQUIRE(P >= 1 && p->channels >= 1 && p->channels <= CMAX && p->vP && p->vD && p->rec_a && p->vY, "da_pcd_train_pass: vn_apply arguments");
        return vn_apply_launch(P, p->channels, p->vP, p->vD, p->rec_a, p->vY, st);
    default:
        DA_REQUIRE(false, "da_pcd_train_pass: unknown pass %d", pass);
    }
    return 0;
}

}  // extern "C"
