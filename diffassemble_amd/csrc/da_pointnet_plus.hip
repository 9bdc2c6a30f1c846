// PointNet++ fragment encoder (backbone="pointnet_plus"): the eval forward of the reference's PointNetPlus(normal_channel=False)
// (backbones/pointnet.py:200-256 and its helpers): two set-abstraction levels that pick centres by farthest point sampling,
// group the points of a ball around each centre, run a three-layer 1x1-conv stack over the grouped rows and keep the maximum
// per group; a third level over all 128 points of the second; a two-layer head.  fp32 throughout, BatchNorm folded on the host.
//
//   k_pnp_fps    one workgroup per fragment, the points and their running distances in registers (8 per lane of 256, N <= 2048)
//                and a copy of the points in LDS for the broadcast of the chosen one.  A pick is one pass over the lane's
//                points, a wave-level maximum of the 64-bit key (distance bits | ~index: the largest distance, the LOWEST index
//                among equals), one LDS exchange between the four waves and ONE barrier (the exchange slots alternate).
//   k_pnp_ball   one wave per centre walks the points in index order, 64 at a time: ballot + prefix popcount append the
//                members in ascending order, the walk stops at nsample, the first member fills the rest.
//   k_pnp_sa     one workgroup (8 waves) gathers a tile of grouped rows into LDS and takes it through the three layers on
//                v_mfma_f32_32x32x2_f32 (exact fp32 operands): the rows are the A operand (read from LDS 16 bytes at a time),
//                the folded weights the B operand (read from L2, one 16-byte load per lane feeds 4 x the tile's row blocks
//                MFMAs), activations ping-pong between two LDS buffers and never leave the CU; the last layer's result stays in
//                registers, where the maximum over a group's rows is an in-lane maximum and one exchange between lane halves.
//                The K axis of the rows is [features | xyz | zero padding to a multiple of 8]: the host permutes and pads the
//                weight columns the same way, so feature copies are aligned 16-byte moves.
//   k_pnp_head   maximum over the third level's four row tiles, then fc1 / fc2 (+ folded BatchNorm, ReLU): a wave per output
//                channel, four fragments per workgroup sharing every weight load.
// Both squared distances are formed by separately rounded fp32 operations (no contraction): the selections are discrete and
// must match the contract index for index.  No atomics anywhere; a fragment's result does not depend on its neighbours.
#include "da_internal.h"

namespace da {
namespace {

typedef __attribute__((ext_vector_type(4))) float pp_f4;
typedef __attribute__((ext_vector_type(16))) float pp_f16;

constexpr int PNP_NMAX = 2048;                       // points per fragment at most (8 per lane of the sampling workgroup)
constexpr int PNP_S1 = 512, PNP_K1 = 32;             // sa1: centres, samples per centre
constexpr int PNP_S2 = 128, PNP_K2 = 64;             // sa2
constexpr int PNP_C1 = 128, PNP_C2 = 256, PNP_C3 = 1024, PNP_OUT = 256;
constexpr int PNP_T3 = 4;                            // sa3: row tiles (of 32 points) per fragment
constexpr int PNP_CHUNK = 1024;                      // fragments per pass over the workspace
constexpr int PNP_NW = 8;                            // waves of a k_pnp_sa workgroup

// d2(p, q) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), d* = fl(p* - q*): every operation rounded on its own
__device__ __forceinline__ float pnp_d2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// ---- farthest point sampling ---------------------------------------------------------------------------------------
// the N points of fragment p: points[p * frag_stride + 3 m], m = sel ? sel[p * sel_stride + n] : n.  idx [P][npoint]
__global__ __launch_bounds__(256) void k_pnp_fps(int N, int npoint, const float *__restrict__ points, long long frag_stride,
                                                 const int32_t *__restrict__ sel, int sel_stride, const int32_t *__restrict__ start,
                                                 int32_t *__restrict__ idx) {
    __shared__ float sx[PNP_NMAX], sy[PNP_NMAX], sz[PNP_NMAX];
    __shared__ unsigned long long wbest[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, p = blockIdx.x;
    const float *pts = points + (size_t)p * frag_stride;
    const int32_t *s = sel ? sel + (size_t)p * sel_stride : nullptr;
    float x[8], y[8], z[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = tid + 256 * i;
        x[i] = y[i] = z[i] = 0.f;
        d[i] = 1e10f;
        if (n < N) {
            const int m = s ? s[n] : n;
            x[i] = pts[(size_t)m * 3]; y[i] = pts[(size_t)m * 3 + 1]; z[i] = pts[(size_t)m * 3 + 2];
            sx[n] = x[i]; sy[n] = y[i]; sz[n] = z[i];
        }
    }
    __syncthreads();
    int far = start[p];
    far = far < 0 ? 0 : (far >= N ? N - 1 : far);
    int32_t *out = idx + (size_t)p * npoint;
    for (int it = 0; it < npoint; ++it) {
        if (tid == 0) out[it] = far;
        const float fx = sx[far], fy = sy[far], fz = sz[far];
        unsigned long long best = 0ull;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = tid + 256 * i;
            if (n < N) {
                d[i] = fminf(d[i], pnp_d2(x[i], y[i], z[i], fx, fy, fz));
                const unsigned long long key = ((unsigned long long)__float_as_uint(d[i]) << 32) | (unsigned)(0xffffffffu - (unsigned)n);
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (lane == 0) wbest[it & 1][w] = best;
        __syncthreads();                               // the slots alternate: iteration it + 2 writes these behind the next barrier
        unsigned long long b = wbest[it & 1][0];
#pragma unroll
        for (int k = 1; k < 4; ++k) b = wbest[it & 1][k] > b ? wbest[it & 1][k] : b;
        far = (int)(0xffffffffu - (unsigned)(b & 0xffffffffull));
    }
}

// ---- ball query -----------------------------------------------------------------------------------------------------
// one wave per centre.  centre [P][S]: index n of the centre among the fragment's N points; grp [P][S][nsample]
__global__ __launch_bounds__(256) void k_pnp_ball(int N, int S, int nsample, float r2, long long total, const float *__restrict__ points,
                                                  long long frag_stride, const int32_t *__restrict__ sel, int sel_stride,
                                                  const int32_t *__restrict__ centre, int32_t *__restrict__ grp) {
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= total) return;
    const long long p = gw / S;
    const float *pts = points + (size_t)p * frag_stride;
    const int32_t *s = sel ? sel + (size_t)p * sel_stride : nullptr;
    int cn = centre[gw];
    cn = cn < 0 ? 0 : (cn >= N ? N - 1 : cn);
    const int cm = s ? s[cn] : cn;
    const float cx = pts[(size_t)cm * 3], cy = pts[(size_t)cm * 3 + 1], cz = pts[(size_t)cm * 3 + 2];
    int32_t *out = grp + (size_t)gw * nsample;
    int count = 0, first = -1;
    for (int n0 = 0; n0 < N && count < nsample; n0 += 64) {
        const int n = n0 + lane;
        bool in = false;
        if (n < N) {
            const int m = s ? s[n] : n;
            in = !(pnp_d2(cx, cy, cz, pts[(size_t)m * 3], pts[(size_t)m * 3 + 1], pts[(size_t)m * 3 + 2]) > r2);
        }
        const unsigned long long mask = __ballot(in);
        const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (in && at < nsample) out[at] = n;
        if (first < 0 && mask) first = n0 + __builtin_ctzll(mask);
        count += __popcll(mask);
    }
    if (first < 0) first = cn;                         // cannot happen for finite points: the centre is a member
    for (int j = (count < nsample ? count : nsample) + lane; j < nsample; j += 64) out[j] = first;
}

// ---- grouped three-layer stack ---------------------------------------------------------------------------------------
struct PnpSaW { const float *w[3], *b[3]; };

__device__ __forceinline__ pp_f16 pp_zero16() {
    pp_f16 z;
#pragma unroll
    for (int v = 0; v < 16; ++v) z[v] = 0.f;
    return z;
}

// how the NW waves share a [ROWS][C] result: C / 32 column blocks dealt round-robin when there are at least NW of them (every
// wave then owns all row blocks), otherwise the row blocks are split RS ways as well
template <int ROWS, int C> struct PnpShape {
    static constexpr int NCB = C / 32, NRBT = ROWS / 32;
    static constexpr int RS = NCB >= PNP_NW ? 1 : PNP_NW / NCB;
    static constexpr int NRB = NRBT / RS;              // row blocks per wave
    static constexpr int CBW = NCB >= PNP_NW ? NCB / PNP_NW : 1;   // column blocks per wave
    static_assert(C % 32 == 0 && ROWS % 32 == 0 && NRBT % RS == 0 && NRB >= 1, "tile shape");
    static_assert(NCB >= PNP_NW ? NCB % PNP_NW == 0 : PNP_NW % NCB == 0, "column blocks against waves");
};

// acc[b] += Xs[rows 32 (rb0 + b) .. + 31][0 .. KP) . W[col][0 .. KP)   (Wl: this lane's W + col * KP + 4 half)
template <int KP, int NRB, int LDI>
__device__ __forceinline__ void pnp_mma(const float *Xs, int rb0, const float *__restrict__ Wl, pp_f16 (&acc)[NRB], int r, int half) {
#pragma unroll 4
    for (int s = 0; s < KP / 8; ++s) {
        const pp_f4 wv = *(const pp_f4 *)(Wl + 8 * s);
#pragma unroll
        for (int b = 0; b < NRB; ++b) {
            const pp_f4 x = *(const pp_f4 *)(Xs + ((rb0 + b) * 32 + r) * LDI + 8 * s + 4 * half);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[e], wv[e], acc[b], 0, 0, 0);
        }
    }
}

// Ys = relu(Xs . W^T + b): Xs [ROWS][LDI] (KP columns used) -> Ys [ROWS][C + 4]
template <int ROWS, int KP, int C, int LDI>
__device__ __forceinline__ void pnp_layer(const float *Xs, float *Ys, const float *__restrict__ W, const float *__restrict__ B, int w, int lane) {
    typedef PnpShape<ROWS, C> S;
    constexpr int LDO = C + 4;
    const int r = lane & 31, half = lane >> 5;
    const int rs = S::RS == 1 ? 0 : w / S::NCB;
#pragma unroll 1
    for (int i = 0; i < S::CBW; ++i) {
        const int cb = S::RS == 1 ? w + PNP_NW * i : w % S::NCB, col = cb * 32 + r;
        pp_f16 acc[S::NRB];
#pragma unroll
        for (int b = 0; b < S::NRB; ++b) acc[b] = pp_zero16();
        pnp_mma<KP, S::NRB, LDI>(Xs, rs * S::NRB, W + (size_t)col * KP + 4 * half, acc, r, half);
        const float bias = B[col];
#pragma unroll
        for (int b = 0; b < S::NRB; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = (rs * S::NRB + b) * 32 + 8 * (v >> 2) + 4 * half + (v & 3);
                Ys[row * LDO + col] = fmaxf(acc[b][v] + bias, 0.f);
            }
    }
}

// LEVEL 1: tile = ROWS / 32 centres of sa1, row = [x_n - centre | x_n | 0 0]                      (KP = 8)
// LEVEL 2: tile = ROWS / 64 centres of sa2, row = [l1 feature (128) | l1_xyz_n - centre | 0 x 5]  (KP = 136)
// LEVEL 3: tile = 32 of a fragment's 128 l2 points, row = [l2 feature (256) | l2_xyz | 0 x 5]     (KP = 264); the output is the
//          tile's own maximum (PNP_T3 rows per fragment, reduced by the head)
// out [tiles * ROWS / GS][C3], GS = rows per group
template <int LEVEL, int ROWS, int KP, int C1, int C2, int C3, int GS>
__global__ __launch_bounds__(PNP_NW * 64) void k_pnp_sa(PnpSaW W, int N, const float *__restrict__ points, const int32_t *__restrict__ fps1,
                                                        const int32_t *__restrict__ fps2, const int32_t *__restrict__ grp,
                                                        const float *__restrict__ feat, float *__restrict__ out) {
    constexpr int LDI = KP + 4, LD1 = C1 + 4, LD2 = C2 + 4;
    constexpr int SZA = ROWS * (LDI > LD2 ? LDI : LD2);
    extern __shared__ __attribute__((aligned(16))) float pnp_lds[];
    float *A = pnp_lds, *Bf = pnp_lds + SZA;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long t = blockIdx.x;
    if (LEVEL == 1) {
        if (tid < ROWS) {
            const long long g = t * (ROWS / GS) + tid / GS, p = g / PNP_S1;
            const float *pts = points + (size_t)p * N * 3;
            const int n = grp[g * GS + tid % GS], c = fps1[g];
            const float x = pts[(size_t)n * 3], y = pts[(size_t)n * 3 + 1], z = pts[(size_t)n * 3 + 2];
            float *row = A + tid * LDI;
            *(pp_f4 *)row = (pp_f4){x - pts[(size_t)c * 3], y - pts[(size_t)c * 3 + 1], z - pts[(size_t)c * 3 + 2], x};
            *(pp_f4 *)(row + 4) = (pp_f4){y, z, 0.f, 0.f};
        }
    } else {
        constexpr int CF = KP - 8, V = CF / 4;         // feature columns, float4 per row
        for (int i = tid; i < ROWS * V; i += PNP_NW * 64) {
            const int rr = i / V, c4 = (i - rr * V) * 4;
            long long src;                             // the row of `feat`
            if (LEVEL == 2) {
                const long long g = t * (ROWS / GS) + rr / GS;
                src = (g / PNP_S2) * PNP_S1 + grp[g * GS + rr % GS];
            } else {
                src = t * ROWS + rr;
            }
            *(pp_f4 *)(A + rr * LDI + c4) = *(const pp_f4 *)(feat + (size_t)src * CF + c4);
        }
        if (tid < ROWS) {
            float *row = A + tid * LDI + CF;
            if (LEVEL == 2) {
                const long long g = t * (ROWS / GS) + tid / GS, p = g / PNP_S2;
                const float *pts = points + (size_t)p * N * 3;
                const int32_t *f1 = fps1 + p * PNP_S1;
                const int n = f1[grp[g * GS + tid % GS]], c = f1[fps2[g]];
                *(pp_f4 *)row = (pp_f4){pts[(size_t)n * 3] - pts[(size_t)c * 3], pts[(size_t)n * 3 + 1] - pts[(size_t)c * 3 + 1],
                                        pts[(size_t)n * 3 + 2] - pts[(size_t)c * 3 + 2], 0.f};
            } else {
                const long long g = t * ROWS + tid, p = g / PNP_S2;
                const float *pts = points + (size_t)p * N * 3;
                const int n = fps1[p * PNP_S1 + fps2[g]];
                *(pp_f4 *)row = (pp_f4){pts[(size_t)n * 3], pts[(size_t)n * 3 + 1], pts[(size_t)n * 3 + 2], 0.f};
            }
            *(pp_f4 *)(row + 4) = (pp_f4){0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    pnp_layer<ROWS, KP, C1, LDI>(A, Bf, W.w[0], W.b[0], w, lane);
    __syncthreads();
    pnp_layer<ROWS, C1, C2, LD1>(Bf, A, W.w[1], W.b[1], w, lane);
    __syncthreads();
    {
        typedef PnpShape<ROWS, C3> S;
        constexpr int G = GS / 32;                     // row blocks per group
        static_assert(GS % 32 == 0 && S::NRB % G == 0, "a group's rows belong to one wave");
        const int r = lane & 31, half = lane >> 5;
        const int rs = S::RS == 1 ? 0 : w / S::NCB;
#pragma unroll 1
        for (int i = 0; i < S::CBW; ++i) {
            const int cb = S::RS == 1 ? w + PNP_NW * i : w % S::NCB, col = cb * 32 + r;
            pp_f16 acc[S::NRB];
#pragma unroll
            for (int b = 0; b < S::NRB; ++b) acc[b] = pp_zero16();
            pnp_mma<C2, S::NRB, LD2>(A, rs * S::NRB, W.w[2] + (size_t)col * C2 + 4 * half, acc, r, half);
            const float bias = W.b[2][col];
#pragma unroll
            for (int g = 0; g < S::NRB / G; ++g) {
                float m = -INFINITY;
#pragma unroll
                for (int b = 0; b < G; ++b)
#pragma unroll
                    for (int v = 0; v < 16; ++v) m = fmaxf(m, acc[g * G + b][v]);
                m = fmaxf(m, __shfl_xor(m, 32));
                // relu and + bias are monotone: the maximum of the activated rows is the activated maximum, bit for bit
                if (half == 0) out[(size_t)(t * (ROWS / GS) + rs * (S::NRB / G) + g) * C3 + col] = fmaxf(m + bias, 0.f);
            }
        }
    }
}

template <int ROWS, int KP, int C1, int C2> constexpr size_t pnp_sa_lds() {
    return sizeof(float) * (size_t)ROWS * ((KP + 4 > C2 + 4 ? KP + 4 : C2 + 4) + C1 + 4);
}

// ---- head -------------------------------------------------------------------------------------------------------------
constexpr int PNP_HF = 4;                              // fragments per workgroup

// Y[f][o] = relu(X[f] . W[o] + b[o]) for the wave's outputs o = w, w + 4, ...
template <int K>
__device__ __forceinline__ void pnp_fc(const float (*X)[K], const float *__restrict__ W, const float *__restrict__ B, int n_out, int w, int lane,
                                       float *Y, int ldy, int valid) {
    for (int o = w; o < n_out; o += 4) {
        float acc[PNP_HF];
#pragma unroll
        for (int f = 0; f < PNP_HF; ++f) acc[f] = 0.f;
        for (int k = lane * 4; k < K; k += 256) {
            const pp_f4 wv = *(const pp_f4 *)(W + (size_t)o * K + k);
#pragma unroll
            for (int f = 0; f < PNP_HF; ++f) {
                const pp_f4 xv = *(const pp_f4 *)(&X[f][k]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[f] = fmaf(xv[e], wv[e], acc[f]);
            }
        }
#pragma unroll
        for (int f = 0; f < PNP_HF; ++f) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) acc[f] += __shfl_xor(acc[f], s);
        }
        if (lane == 0) {
            const float bias = B[o];
#pragma unroll
            for (int f = 0; f < PNP_HF; ++f)
                if (f < valid) Y[(size_t)f * ldy + o] = fmaxf(acc[f] + bias, 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void k_pnp_head(int P, const float *__restrict__ part, const float *__restrict__ W1, const float *__restrict__ B1,
                                                  const float *__restrict__ W2, const float *__restrict__ B2, float *__restrict__ out, int ld_out) {
    __shared__ __attribute__((aligned(16))) float xs[PNP_HF][PNP_C3];
    __shared__ __attribute__((aligned(16))) float hs[PNP_HF][512];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, p0 = blockIdx.x * PNP_HF;
    const int valid = P - p0 < PNP_HF ? P - p0 : PNP_HF;
    for (int i = tid; i < PNP_HF * PNP_C3; i += 256) {
        const int f = i / PNP_C3, c = i - f * PNP_C3;
        float v = 0.f;
        if (f < valid) {
            const float *q = part + ((size_t)(p0 + f) * PNP_T3) * PNP_C3 + c;
            v = q[0];
#pragma unroll
            for (int k = 1; k < PNP_T3; ++k) v = fmaxf(v, q[(size_t)k * PNP_C3]);
        }
        xs[f][c] = v;
    }
    __syncthreads();
    pnp_fc<PNP_C3>(xs, W1, B1, 512, w, lane, &hs[0][0], 512, PNP_HF);
    __syncthreads();
    pnp_fc<512>(hs, W2, B2, PNP_OUT, w, lane, out + (size_t)p0 * ld_out, ld_out, valid);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct PnpWork {
    int32_t *fps1, *grp1, *fps2, *grp2;
    float *l1, *l2, *part;
    size_t bytes;
};
PnpWork pnp_work(void *base, long long P) {
    PnpWork w;
    char *b = (char *)base;
    size_t o = 0;
    w.fps1 = (int32_t *)(b + o); o += align_up((size_t)P * PNP_S1 * sizeof(int32_t), 256);
    w.grp1 = (int32_t *)(b + o); o += align_up((size_t)P * PNP_S1 * PNP_K1 * sizeof(int32_t), 256);
    w.fps2 = (int32_t *)(b + o); o += align_up((size_t)P * PNP_S2 * sizeof(int32_t), 256);
    w.grp2 = (int32_t *)(b + o); o += align_up((size_t)P * PNP_S2 * PNP_K2 * sizeof(int32_t), 256);
    w.l1 = (float *)(b + o); o += align_up((size_t)P * PNP_S1 * PNP_C1 * sizeof(float), 256);
    w.l2 = (float *)(b + o); o += align_up((size_t)P * PNP_S2 * PNP_C2 * sizeof(float), 256);
    w.part = (float *)(b + o); o += align_up((size_t)P * PNP_T3 * PNP_C3 * sizeof(float), 256);
    w.bytes = o;
    return w;
}

bool pnp_aligned16(const void *p) { return ((size_t)p & 15) == 0; }

// the three levels' tile shapes: <LEVEL, ROWS, KP, C1, C2, C3, GS>.  Rows per tile of sa1 / sa2: -DPNP_R1=256 / -DPNP_R2=64 build the
// shapes these were measured against
#ifndef PNP_R1
#define PNP_R1 128
#endif
#ifndef PNP_R2
#define PNP_R2 128
#endif
#define PNP_SA1 1, PNP_R1, 8, 64, 64, PNP_C1, PNP_K1
#define PNP_SA2 2, PNP_R2, 136, 128, 128, PNP_C2, PNP_K2
#define PNP_SA3 3, 32, 264, 256, 512, PNP_C3, 32
constexpr size_t PNP_LDS1 = pnp_sa_lds<PNP_R1, 8, 64, 64>(), PNP_LDS2 = pnp_sa_lds<PNP_R2, 136, 128, 128>(), PNP_LDS3 = pnp_sa_lds<32, 264, 256, 512>();
static_assert(PNP_LDS1 <= 160 * 1024 && PNP_LDS2 <= 160 * 1024 && PNP_LDS3 <= 160 * 1024, "LDS of a CU");

enum { PNP_ST_FPS1 = 1, PNP_ST_BALL1 = 2, PNP_ST_SA1 = 4, PNP_ST_FPS2 = 8, PNP_ST_BALL2 = 16, PNP_ST_SA2 = 32, PNP_ST_SA3 = 64, PNP_ST_HEAD = 128 };

int pnp_run(const da_pointnet_plus_weights *w, int P, int N, const float *points, const int32_t *start1, const int32_t *start2, float *out,
            int ld_out, void *workspace, int stages, hipStream_t st) {
    static bool attr = false;
    if (!attr) {
        DA_CHECK_HIP(hipFuncSetAttribute((const void *)k_pnp_sa<PNP_SA1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PNP_LDS1));
        DA_CHECK_HIP(hipFuncSetAttribute((const void *)k_pnp_sa<PNP_SA2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PNP_LDS2));
        DA_CHECK_HIP(hipFuncSetAttribute((const void *)k_pnp_sa<PNP_SA3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PNP_LDS3));
        attr = true;
    }
    PnpSaW W[3];
    for (int l = 0; l < 9; ++l) { W[l / 3].w[l % 3] = w->w[l]; W[l / 3].b[l % 3] = w->b[l]; }
    const float r1 = (float)(0.2 * 0.2), r2 = (float)(0.4 * 0.4);      // float32(radius ** 2) of the reference's two levels
    const long long fs = (long long)N * 3;
    for (int p0 = 0; p0 < P; p0 += PNP_CHUNK) {
        const int pc = P - p0 < PNP_CHUNK ? P - p0 : PNP_CHUNK;
        const PnpWork k = pnp_work(workspace, P < PNP_CHUNK ? P : PNP_CHUNK);
        const float *pts = points + (size_t)p0 * fs;
        if (stages & PNP_ST_FPS1) k_pnp_fps<<<(unsigned)pc, 256, 0, st>>>(N, PNP_S1, pts, fs, nullptr, 0, start1 + p0, k.fps1);
        if (stages & PNP_ST_BALL1)
            k_pnp_ball<<<(unsigned)(pc * (PNP_S1 / 4)), 256, 0, st>>>(N, PNP_S1, PNP_K1, r1, (long long)pc * PNP_S1, pts, fs, nullptr, 0, k.fps1, k.grp1);
        if (stages & PNP_ST_SA1)
            k_pnp_sa<PNP_SA1><<<(unsigned)(pc * (PNP_S1 * PNP_K1 / PNP_R1)), PNP_NW * 64, PNP_LDS1, st>>>(W[0], N, pts, k.fps1, nullptr, k.grp1, nullptr, k.l1);
        if (stages & PNP_ST_FPS2) k_pnp_fps<<<(unsigned)pc, 256, 0, st>>>(PNP_S1, PNP_S2, pts, fs, k.fps1, PNP_S1, start2 + p0, k.fps2);
        if (stages & PNP_ST_BALL2)
            k_pnp_ball<<<(unsigned)(pc * (PNP_S2 / 4)), 256, 0, st>>>(PNP_S1, PNP_S2, PNP_K2, r2, (long long)pc * PNP_S2, pts, fs, k.fps1, PNP_S1, k.fps2,
                                                                      k.grp2);
        if (stages & PNP_ST_SA2)
            k_pnp_sa<PNP_SA2><<<(unsigned)(pc * (PNP_S2 * PNP_K2 / PNP_R2)), PNP_NW * 64, PNP_LDS2, st>>>(W[1], N, pts, k.fps1, k.fps2, k.grp2, k.l1, k.l2);
        if (stages & PNP_ST_SA3)
            k_pnp_sa<PNP_SA3><<<(unsigned)(pc * PNP_T3), PNP_NW * 64, PNP_LDS3, st>>>(W[2], N, pts, k.fps1, k.fps2, nullptr, k.l2, k.part);
        if (stages & PNP_ST_HEAD)
            k_pnp_head<<<(unsigned)((pc + PNP_HF - 1) / PNP_HF), 256, 0, st>>>(pc, k.part, w->w[9], w->b[9], w->w[10], w->b[10],
                                                                              out + (size_t)p0 * ld_out, ld_out);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

int pnp_args_ok(const da_pointnet_plus_weights *w, int n_parts, int n_points, const float *points, const int32_t *start1,
                const int32_t *start2, float *out, int ld_out, void *workspace, size_t workspace_bytes, const char *who) {
    DA_REQUIRE(w, "%s: null weights", who);
    DA_REQUIRE(n_parts >= 0, "%s: n_parts %d (need >= 0)", who, n_parts);
    DA_REQUIRE(n_points >= 1 && n_points <= PNP_NMAX, "%s: n_points %d: the sampling kernel holds a fragment in one workgroup's registers, 1 .. %d points",
               who, n_points, PNP_NMAX);
    if (n_parts == 0) return 0;
    DA_REQUIRE(points && start1 && start2 && out && ld_out >= PNP_OUT, "%s: null points / start1 / start2 / out, or ld_out %d < %d", who, ld_out,
               PNP_OUT);
    for (int l = 0; l < DA_PNP_LAYERS; ++l)
        DA_REQUIRE(w->w[l] && w->b[l] && pnp_aligned16(w->w[l]), "%s: layer %d: null or misaligned weights", who, l);
    const size_t need = pnp_work(nullptr, n_parts < PNP_CHUNK ? n_parts : PNP_CHUNK).bytes;
    DA_REQUIRE(workspace && pnp_aligned16(workspace) && workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who,
               workspace_bytes, need);
    return 0;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

int da_pnp_fps(int n_parts, int n_points, int npoint, const float *points, const int32_t *start, int32_t *idx, void *stream) {
    DA_REQUIRE(n_parts >= 0 && npoint >= 0, "da_pnp_fps: n_parts %d / npoint %d (need >= 0)", n_parts, npoint);
    DA_REQUIRE(n_points >= 1 && n_points <= PNP_NMAX, "da_pnp_fps: n_points %d: a fragment lives in one workgroup's registers, 1 .. %d points", n_points,
               PNP_NMAX);
    if (n_parts == 0 || npoint == 0) return 0;
    DA_REQUIRE(points && start && idx, "da_pnp_fps: null points / start / idx");
    k_pnp_fps<<<(unsigned)n_parts, 256, 0, (hipStream_t)stream>>>(n_points, npoint, points, (long long)n_points * 3, nullptr, 0, start, idx);
    DA_LAUNCH_CHECK();
    return 0;
}

int da_pnp_ball_query(int n_parts, int n_points, int n_centres, int nsample, double radius, const float *points, const int32_t *centre,
                      int32_t *grp, void *stream) {
    DA_REQUIRE(n_parts >= 0 && n_centres >= 0 && nsample >= 1, "da_pnp_ball_query: n_parts %d / n_centres %d / nsample %d", n_parts, n_centres, nsample);
    DA_REQUIRE(n_points >= 1 && n_points <= PNP_NMAX, "da_pnp_ball_query: n_points %d (need 1 .. %d)", n_points, PNP_NMAX);
    const long long total = (long long)n_parts * n_centres;
    if (total == 0) return 0;
    DA_REQUIRE(total < (1ll << 32), "da_pnp_ball_query: too many centres");
    DA_REQUIRE(points && centre && grp, "da_pnp_ball_query: null points / centre / grp");
    k_pnp_ball<<<(unsigned)((total + 3) / 4), 256, 0, (hipStream_t)stream>>>(n_points, n_centres, nsample, (float)(radius * radius), total, points,
                                                                            (long long)n_points * 3, nullptr, 0, centre, grp);
    DA_LAUNCH_CHECK();
    return 0;
}

size_t da_pointnet_plus_workspace_bytes(int n_parts, int n_points) {
    if (n_parts <= 0 || n_points <= 0) return 0;
    return pnp_work(nullptr, n_parts < PNP_CHUNK ? n_parts : PNP_CHUNK).bytes;
}

int da_pointnet_plus_workspace_offsets(int n_parts, size_t offsets[7]) {
    if (n_parts > 0 && offsets) {
        const PnpWork k = pnp_work(nullptr, n_parts < PNP_CHUNK ? n_parts : PNP_CHUNK);      // base 0: the pointers ARE the offsets
        const void *at[7] = {k.fps1, k.grp1, k.fps2, k.grp2, k.l1, k.l2, k.part};
        for (int i = 0; i < 7; ++i) offsets[i] = (size_t)at[i];
    }
    return PNP_CHUNK;
}

int da_pointnet_plus_forward(const da_pointnet_plus_weights *w, int n_parts, int n_points, const float *points, const int32_t *start1,
                             const int32_t *start2, float *out, int ld_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = pnp_args_ok(w, n_parts, n_points, points, start1, start2, out, ld_out, workspace, workspace_bytes, "da_pointnet_plus_forward")) return rc;
    if (n_parts == 0) return 0;
    return pnp_run(w, n_parts, n_points, points, start1, start2, out, ld_out, workspace, 255, (hipStream_t)stream);
}

int da_pointnet_plus_stages(const da_pointnet_plus_weights *w, int n_parts, int n_points, const float *points, const int32_t *start1,
                            const int32_t *start2, float *out, int ld_out, void *workspace, size_t workspace_bytes, int stages, void *stream) {
    if (int rc = pnp_args_ok(w, n_parts, n_points, points, start1, start2, out, ld_out, workspace, workspace_bytes, "da_pointnet_plus_stages")) return rc;
    if (n_parts == 0) return 0;
    return pnp_run(w, n_parts, n_points, points, start1, start2, out, ld_out, workspace, stages & 255, (hipStream_t)stream);
}

}  // extern "C"
