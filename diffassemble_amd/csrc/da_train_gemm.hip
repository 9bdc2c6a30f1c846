// Products and element-wise pieces of the training paths (the denoiser's, da_train.hip; the piece encoder's, the point-cloud
// encoders' and PointNet's call the dW products too, through da_internal.h).
//
// Linear layers: dX = dY @ W runs through the forward MFMA linear kernel with W transposed once per step (k_weight_prep,
// da_train.hip); dW = dY^T @ X is a dedicated MFMA kernel whose reduction runs over the node dimension, split over node chunks with
// a deterministic second-pass reduction -- three families: k_gemm_tn (fp32 operands, exact or rounded to bf16 in registers),
// k_gemm_tn_db (the bf16-operand mode: dW and db from one pass over dY), k_gemm_tn_bf16 (bf16 operands in memory: the encoder).
// Beside them: the bias gradient's column sums, the fp32 transpose, the bf16 cast and the GELU / LeakyReLU kernels.
#include <type_traits>

#include "da_train.h"

namespace da {

// dst = gelu(src); dst16 (optional): the same values rounded to bf16 -- the next projection's operand in the q16 mode (its own
// k_cast_h launch folded in; the rounding is of the fp32 value just stored, i.e. the same bits)
__global__ __launch_bounds__(256) void k_gelu_fwd(size_t n, const float *__restrict__ src, float *__restrict__ dst, bf16_t *__restrict__ dst16) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = gelu_erf(src[i]);
        dst[i] = v;
        if (dst16) dst16[i] = f2bf(v);
    }
}

// dx = dy * gelu'(pre)   (dx may alias dy)
__global__ __launch_bounds__(256) void k_gelu_bwd(size_t n, const float *__restrict__ pre, const float *dy, float *dx) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dx[i] = dy[i] * gelu_grad(pre[i]);
}

// dx = dy * (out > 0 ? 1 : 0.2): LeakyReLU(0.2) backward from the layer's OUTPUT (same sign as its input; 0 takes the slope like torch)
__global__ __launch_bounds__(256) void k_leaky_bwd(size_t n, const float *__restrict__ out, const float *dy, float *dx) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dx[i] = out[i] > 0.f ? dy[i] : 0.2f * dy[i];
}

// dst = bf16(src), 8 elements per thread and pass (n a multiple of 8; both 16-byte aligned)
__global__ __launch_bounds__(256) void k_cast_h(size_t n8, const float *__restrict__ src, bf16_t *__restrict__ dst) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = *(const f32x4 *)(src + 8 * i), b = *(const f32x4 *)(src + 8 * i + 4);
        typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_;
        const bf16x8_ v = {(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
        *(u32x4 *)(dst + 8 * i) = __builtin_bit_cast(u32x4, v);
    }
}
int cast_h(size_t n, const float *src, bf16_t *dst, hipStream_t st) {
    const size_t n8 = n / 8, blocks = (n8 + 255) / 256;
    k_cast_h<<<(unsigned)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks)), 256, 0, st>>>(n8, src, dst);
    DA_LAUNCH_CHECK();
    return 0;
}
// dst[c][r] = src[r][c]
__global__ __launch_bounds__(256) void k_transpose(int rows, int cols, const float *__restrict__ src, float *__restrict__ dst) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 8 * k][tx] = src[(size_t)r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (r < rows && c < cols) dst[(size_t)c * rows + r] = tile[tx][ty + 8 * k];
    }
}

// out[c] += sum_m A[m][c]      (bias gradients).  Two deterministic stages: grid (ceil(N/64), chunks)
// column sums over row chunks into `partial[chunk][N]`, then one pass adds the chunks into out.
__global__ __launch_bounds__(256) void k_colsum_partial(int M, int N, const float *__restrict__ A, int lda, int rows_per,
                                                        float *__restrict__ partial) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    const int m0 = blockIdx.y * rows_per, m1 = min(M, m0 + rows_per);
    float s = 0.f;
    if (c < N)
        for (int m = m0 + ty; m < m1; m += 4) s += A[(size_t)m * lda + c];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < N) partial[(size_t)blockIdx.y * N + c] = red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx];
}
// 64 columns per block, four threads per column: thread (tx, ty) adds the chunks ty, ty + 4, ... in ascending order, the four
// sub-sums are combined as (s0 + s1) + (s2 + s3) -- a fixed order (data-parallel replicas must produce identical bits), a
// quarter of the dependent loads per thread (one thread per column walked all chunks: 15 - 18 us per call, 8 calls per step)
__global__ __launch_bounds__(256) void k_colsum_finish(int chunks, int N, const float *__restrict__ partial, float *out) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    float s = 0.f;
    if (c < N)
        for (int k = ty; k < chunks; k += 4) s += partial[(size_t)k * N + c];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < N) out[c] += (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

// ---------------------------------------------------------------------------------------------
// dW kernel: C[n][k] (+)= sum_m A[m][n] * B[m][k]   (A = dY [M, N], B = X [M, K], both row-major:
// the reduction runs over ROWS, so both tiles are staged exactly as they lie in memory, [m][col], and
// the fp32 MFMA fragments (one float per lane: row = lane & 15 of the output tile, k = lane >> 4) are
// read with conflict-free 4-byte LDS reads -- no transposes anywhere).
// Tile 64 (n) x 64 (k), 16 rows of m per stage, 4 waves as 2 x 2, v_mfma_f32_16x16x4_f32.
// grid = (ceil(K/64), ceil(N/64), splits); split s reduces rows [s * Mc, (s + 1) * Mc).
__device__ __forceinline__ f32x4 load_row4(const float *base, int ld, int row, int col, int rows, int cols, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= rows) return v;
    const float *p = base + (size_t)row * ld + col;
    if (vec && col + 3 < cols) return *(const f32x4 *)p;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (col + r < cols) v[r] = p[r];
    return v;
}

// BFC: the fp32 tiles are rounded to bf16 in registers and multiplied with v_mfma_f32_16x16x16_bf16 (one MFMA per 16-row
// stage and tile pair instead of four exact-fp32 ones; training's DA_TRAIN_MMA_BF16 mode); lane group g = lane >> 4 takes the
// stage rows g, g + 4, g + 8, g + 12 (any assignment works as long as both operands use it: rows one apart keep the four
// groups on different banks)
template <bool BFC>
__global__ __launch_bounds__(256) void k_gemm_tn(int M, int N, int K, const float *__restrict__ A, int lda,
                                                 const float *__restrict__ B, int ldb, float *C, int ldc,
                                                 float *partial, int Mc) {
    constexpr int LS = 80;                                       // LDS row stride (floats): 4 rows -> banks 0,16,32,48
    __shared__ __attribute__((aligned(16))) float As[16 * LS];
    __shared__ __attribute__((aligned(16))) float Bs[16 * LS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    const int m_beg = blockIdx.z * Mc, m_end = min(M, m_beg + Mc);
    const int lrow = tid >> 4, lc4 = (tid & 15) * 4;
    const bool vecA = (lda % 4 == 0) && (((size_t)A & 15) == 0), vecB = (ldb % 4 == 0) && (((size_t)B & 15) == 0);
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 ra = load_row4(A, lda, m_beg + lrow, n0 + lc4, m_end, N, vecA);
    f32x4 rb = load_row4(B, ldb, m_beg + lrow, k0 + lc4, m_end, K, vecB);
    for (int m0 = m_beg; m0 < m_end; m0 += 16) {
        *(f32x4 *)(As + lrow * LS + lc4) = ra;
        *(f32x4 *)(Bs + lrow * LS + lc4) = rb;
        __syncthreads();
        if (m0 + 16 < m_end) {
            ra = load_row4(A, lda, m0 + 16 + lrow, n0 + lc4, m_end, N, vecA);
            rb = load_row4(B, ldb, m0 + 16 + lrow, k0 + lc4, m_end, K, vecB);
        }
        if (BFC) {
            typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_;
            typedef __attribute__((ext_vector_type(4))) short s16x4_;
            s16x4_ a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x4_ ta, tb;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ta[e] = (__bf16)As[(4 * e + (lane >> 4)) * LS + wr * 32 + i * 16 + (lane & 15)];
                    tb[e] = (__bf16)Bs[(4 * e + (lane >> 4)) * LS + wc * 32 + i * 16 + (lane & 15)];
                }
                a[i] = __builtin_bit_cast(s16x4_, ta);
                b[i] = __builtin_bit_cast(s16x4_, tb);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[i], b[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[(kk + (lane >> 4)) * LS + wr * 32 + i * 16 + (lane & 15)];
                b[i] = Bs[(kk + (lane >> 4)) * LS + wc * 32 + i * 16 + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        }
        __syncthreads();
    }
    float *dst = partial ? partial + (size_t)blockIdx.z * N * K : C;
    const int ldd = partial ? K : ldc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wr * 32 + i * 16 + 4 * (lane >> 4) + r, k = k0 + wc * 32 + j * 16 + (lane & 15);
                if (n < N && k < K) {
                    if (partial) dst[(size_t)n * ldd + k] = acc[i][j][r];
                    else dst[(size_t)n * ldd + k] += acc[i][j][r];
                }
            }
}

__global__ __launch_bounds__(256) void k_reduce_partial(int splits, int N, int K, const float *__restrict__ partial,
                                                        float *C, int ldc) {
    const size_t NK = (size_t)N * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < NK; i += (size_t)gridDim.x * blockDim.x) {
        // fixed summation order (deterministic), eight independent loads in flight: the split count reaches several
        // hundred for the encoder's weight gradients and one dependent load per iteration was latency-bound
        float s = 0.f;
        int k = 0;
        for (; k + 8 <= splits; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(k + u) * NK + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; k < splits; ++k) s += partial[(size_t)k * NK + i];
        const size_t n = i / K, kk = i - n * K;
        C[n * ldc + kk] += s;
    }
}

// k_reduce_partial and k_colsum_finish in one launch (launch_gemm_tn_db): items [0, N K) add the split partials into C (when
// partial != null), items [N K, N K + N) add the `splits` row-range sums of a dY column into db -- in k_colsum_finish's order
// ((s0 + s1) + (s2 + s3), s_q = chunks q, q + 4, ... ascending), so the bits are the ones the two-launch form produced.
__global__ __launch_bounds__(256) void k_tn_finish(int splits, int N, int K, const float *__restrict__ partial, float *C, int ldc,
                                                   const float *__restrict__ bpartial, float *db) {
    const size_t NK = partial ? (size_t)N * K : 0, items = NK + (bpartial ? (size_t)N : 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        if (i < NK) {
            const size_t NKs = (size_t)N * K;
            float s = 0.f;
            int k = 0;
            for (; k + 32 <= splits; k += 32) {               // (small outputs are cut into up to 144 row ranges: 32 loads in flight)
                float v[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) v[u] = partial[(size_t)(k + u) * NKs + i];
#pragma unroll
                for (int u = 0; u < 32; ++u) s += v[u];
            }
            for (; k + 8 <= splits; k += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(k + u) * NKs + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; k < splits; ++k) s += partial[(size_t)k * NKs + i];
            const size_t n = i / K, kk = i - n * K;
            C[n * ldc + kk] += s;
        } else {
            const size_t c = i - NK;
            float q[4] = {0.f, 0.f, 0.f, 0.f};
            int k = 0;
            for (; k + 32 <= splits; k += 32) {
                float v[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) v[u] = bpartial[(size_t)(k + u) * N + c];
#pragma unroll
                for (int u = 0; u < 32; ++u) q[u & 3] += v[u];
            }
            for (; k < splits; ++k) q[k & 3] += bpartial[(size_t)k * N + c];
            db[c] += (q[0] + q[1]) + (q[2] + q[3]);
        }
    }
}

// the split partials of a dW product into C, behind the product on its stream
static void reduce_partial(long splits, int N, int K, const float *partial, float *C, int ldc, hipStream_t st) {
    const size_t NK = (size_t)N * K;
    k_reduce_partial<<<(unsigned)((NK + 255) / 256 > 4096 ? 4096 : (NK + 255) / 256), 256, 0, st>>>((int)splits, N, K, partial, C, ldc);
}

int launch_gemm_tn(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                          float *partial, hipStream_t st, bool bfc) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int tn = (N + 63) / 64, tk = (K + 63) / 64;
    long splits = 2048 / ((long)tn * tk);
    const long by_rows = (M + 255) / 256, by_cap = (long)(PART_CAP / ((size_t)N * K));
    splits = splits > by_rows ? by_rows : splits;
    splits = splits > by_cap ? by_cap : splits;
    if (splits < 1) splits = 1;
    int Mc = (int)(((M + splits - 1) / splits + 15) / 16 * 16);
    splits = (M + Mc - 1) / Mc;
    const dim3 grid((unsigned)tk, (unsigned)tn, (unsigned)splits);
    if (splits == 1) {
        if (bfc) k_gemm_tn<true><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, nullptr, Mc);
        else k_gemm_tn<false><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, nullptr, Mc);
    } else {
        if (bfc) k_gemm_tn<true><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, partial, Mc);
        else k_gemm_tn<false><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, partial, Mc);
        reduce_partial(splits, N, K, partial, C, ldc, st);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// dW + db in ONE pass for the bf16-operand training mode (round 4): C[n][k] += sum_m A[m][n] B[m][k] and, if db,
// db[n] += sum_m A[m][n] (A = dY, B = X, fp32 row-major).  k_gemm_tn<true> above is bound by what its 64 x 64 tiles pull through
// the L2 (every dY column block is re-read K / 64 times, every X column block N / 64 times: 1.36 GB per call at BASELINE
// configuration 5's conv 3) and the bias gradient read dY once more in its own two kernels.  Here: 128 x 128 tiles (half the
// operand traffic), 64 rows of m per stage (one stage of register prefetch: the bytes in flight per workgroup are what hides the load latency at two to three workgroups per CU), the fp32 tiles rounded to bf16 on their way into LDS (row-major [m][col], 8-byte
// stores) and fetched as MFMA fragments by ds_read_b64_tr_b16 (one read per 16 x 16 operand block instead of four scalar reads +
// four conversions); the workgroups of the first k tile also add up their dY columns in fp32 (exact values, fixed order) while
// they stage them.  grid = (ceil(K/128), ceil(N/128), splits).
typedef __attribute__((ext_vector_type(4))) short tn_s16x4;
// 4 consecutive bf16 of a row-major matrix as fp32, zero beyond (rows, cols)
__device__ __forceinline__ f32x4 load_row4_h(const bf16_t *base, int ld, int row, int col, int rows, int cols, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= rows) return v;
    const bf16_t *p = base + (size_t)row * ld + col;
    if (vec && col + 3 < cols) {
        const u32x2 u = *(const u32x2 *)p;
        return (f32x4){bf2f((bf16_t)(u[0] & 0xffff)), bf2f((bf16_t)(u[0] >> 16)), bf2f((bf16_t)(u[1] & 0xffff)), bf2f((bf16_t)(u[1] >> 16))};
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (col + r < cols) v[r] = bf2f(p[r]);
    return v;
}
// A16: A (dY) is stored as bf16 (the q16 mode's projection gradient); B16: B (the layer's input X) comes as the bf16 image the forward
// kept of it (q16 mode: the projection's own operand) -- 8 instead of 16 bytes per piece on the kernel's dominant stream (a 128 x 128
// tile pulls 32 KB of fp32 X per 64-row stage against 16 KB of bf16 dY; the kernel moves ~0.5 GB through the L2 per call)
template <bool A16, bool B16 = false>
__global__ __launch_bounds__(256) void k_gemm_tn_db(int M, int N, int K, const void *__restrict__ Av, int lda,
                                                    const void *__restrict__ Bv, int ldb, float *C, int ldc,
                                                    float *partial, float *bpartial, int Mc, int xcd_tk) {
    constexpr int PT = 136;                                      // LDS row pitch (bf16 elements): 272 B
    constexpr int SR = 64, NU = SR / 8;                          // rows of m per stage; 8-byte / 16-byte pieces per thread, operand and stage
    __shared__ __attribute__((aligned(16))) unsigned short As[SR * PT];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[SR * PT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1, l15 = lane & 15, lg = lane >> 4;
    // xcd_tk > 0: 1-D grid with the row split = id % splits (splits a multiple of 8: workgroups are dealt round-robin over the
    // 8 XCDs, so ALL tiles of one row range run on one XCD, start together and walk the rows at the same pace -- the operand
    // rows one of them pulls in are L2 hits for the others; with the 3-D grid the tiles of a row range were spread over the XCDs
    // and every one of them fetched its operands from the fabric)
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (xcd_tk > 0) {
        const int splits = (M + Mc - 1) / Mc, tile = blockIdx.x / splits;
        bz = blockIdx.x - tile * splits;
        by = tile / xcd_tk;
        bx = tile - by * xcd_tk;
    }
    const int n0 = by * 128, k0 = bx * 128;
    const int m_beg = bz * Mc, m_end = min(M, m_beg + Mc);
    const int lrow = tid >> 5, lc4 = (tid & 31) * 4;             // stage rows lrow + 8 u, columns lc4 ..+3
    const bool vecA = (lda % 4 == 0) && (((size_t)Av & 15) == 0), vecB = (ldb % 4 == 0) && (((size_t)Bv & 15) == 0);
    auto pack = [](const f32x4 &v) {
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_;
        const bf16x4_ b = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        return __builtin_bit_cast(tn_s16x4, b);
    };
    // A pieces stay in the form they are stored in (bf16: the bits go to LDS untouched; fp32: rounded when they are written there)
    typedef typename std::conditional<A16, tn_s16x4, f32x4>::type RA;
    auto loadA = [&](int row) -> RA {
        if constexpr (A16) {
            const bf16_t *q = (const bf16_t *)Av + (size_t)row * lda + n0 + lc4;
            if (row < m_end && vecA && n0 + lc4 + 3 < N) return *(const tn_s16x4 *)q;
            return pack(load_row4_h((const bf16_t *)Av, lda, row, n0 + lc4, m_end, N, false));
        } else {
            return load_row4((const float *)Av, lda, row, n0 + lc4, m_end, N, vecA);
        }
    };
    typedef typename std::conditional<B16, tn_s16x4, f32x4>::type RB;
    auto loadB = [&](int row) -> RB {
        if constexpr (B16) {
            const bf16_t *q = (const bf16_t *)Bv + (size_t)row * ldb + k0 + lc4;
            if (row < m_end && vecB && k0 + lc4 + 3 < K) return *(const tn_s16x4 *)q;
            return pack(load_row4_h((const bf16_t *)Bv, ldb, row, k0 + lc4, m_end, K, false));
        } else {
            return load_row4((const float *)Bv, ldb, row, k0 + lc4, m_end, K, vecB);
        }
    };
    const bool want_db = bpartial != nullptr && bx == 0;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 csum = {0.f, 0.f, 0.f, 0.f};
    RA ra[NU];
    RB rb[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        ra[u] = loadA(m_beg + lrow + 8 * u);
        rb[u] = loadB(m_beg + lrow + 8 * u);
    }
    for (int m0 = m_beg; m0 < m_end; m0 += SR) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if constexpr (A16) {
                *(tn_s16x4 *)(As + (lrow + 8 * u) * PT + lc4) = ra[u];
                if (want_db) {
                    const unsigned lo = (unsigned)(unsigned short)ra[u][0] | ((unsigned)(unsigned short)ra[u][1] << 16);
                    const unsigned hi = (unsigned)(unsigned short)ra[u][2] | ((unsigned)(unsigned short)ra[u][3] << 16);
                    csum += (f32x4){__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                                    __uint_as_float(hi & 0xffff0000u)};
                }
            } else {
                *(tn_s16x4 *)(As + (lrow + 8 * u) * PT + lc4) = pack(ra[u]);
                csum += ra[u];
            }
            if constexpr (B16) *(tn_s16x4 *)(Bs + (lrow + 8 * u) * PT + lc4) = rb[u];
            else *(tn_s16x4 *)(Bs + (lrow + 8 * u) * PT + lc4) = pack(rb[u]);
        }
        __syncthreads();
        if (m0 + SR < m_end) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                ra[u] = loadA(m0 + SR + lrow + 8 * u);
                rb[u] = loadB(m0 + SR + lrow + 8 * u);
            }
        }
#pragma unroll
        for (int ks = 0; ks < SR / 16; ++ks) {
            tn_s16x4 a[4], b[4];
            // fragment (k = rows 16 ks + 4 lg ..+3, n = column c0 + l15): lane i' of a 16-lane group supplies the address of
            // row (i' >> 2), columns 4 (i' & 3) ..+3 and receives column i' of the four rows
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tn_s16x4 *)(
                    As + (16 * ks + 4 * lg + (l15 >> 2)) * PT + wr * 64 + i * 16 + 4 * (l15 & 3)));
                b[i] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tn_s16x4 *)(
                    Bs + (16 * ks + 4 * lg + (l15 >> 2)) * PT + wc * 64 + i * 16 + 4 * (l15 & 3)));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *dst = partial ? partial + (size_t)bz * N * K : C;
    const int ldd = partial ? K : ldc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wr * 64 + i * 16 + 4 * lg + r, k = k0 + wc * 64 + j * 16 + l15;
                if (n < N && k < K) {
                    if (partial) dst[(size_t)n * ldd + k] = acc[i][j][r];
                    else dst[(size_t)n * ldd + k] += acc[i][j][r];
                }
            }
    if (want_db) {                                              // the eight row groups' sums of each column, fixed order
        float *red = (float *)As;                               // [8][128] floats = 4 KB of the 17 KB tile
        *(f32x4 *)(red + lrow * 128 + lc4) = csum;
        __syncthreads();
        if (tid < 128 && n0 + tid < N) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += red[g * 128 + tid];
            bpartial[(size_t)bz * N + n0 + tid] = s;
        }
    }
}

// dW (+ db) of the bf16-operand mode.  bscratch: splits * N floats
int launch_gemm_tn_db(int M, int N, int K, const void *A, int lda, const void *B, int ldb, float *C, int ldc,
                      float *partial, float *db, float *bscratch, hipStream_t st, bool a16, bool b16) {
    DA_REQUIRE(!b16 || a16, "launch_gemm_tn_db: a bf16 X image is only instantiated beside a bf16 dY");
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int tn = (N + 127) / 128, tk = (K + 127) / 128;
    long splits = 640 / ((long)tn * tk);
    // (one- and two-tile outputs -- the head's, pos_mlp's, mlp.2's gradients: row ranges of ONE 64-row stage, so that the launch is
    //  one load round trip deep instead of four: 14 -> ~5 us each at 9 216 rows)
    const long by_rows = tn * tk <= 2 ? (M + 63) / 64 : (M + 255) / 256, by_cap = (long)(PART_CAP / ((size_t)N * K));
    splits = splits > by_rows ? by_rows : splits;
    splits = splits > by_cap ? by_cap : splits;
    if (splits < 1) splits = 1;
    const bool xcd_off = DA_XENV("DA_TN_NO_XCD_MAP", 0) != 0;
    // several tiles and enough rows: exactly 8 (or 16) row ranges, one (two) per XCD (see the kernel)
    const bool xcd = !xcd_off && tn * tk >= 8 && by_rows >= 8 && by_cap >= 8;
    if (xcd) splits = (tn * tk <= 12 && by_rows >= 32 && by_cap >= 32) ? 32 : (tn * tk <= 24 && by_rows >= 16 && by_cap >= 16) ? 16 : 8;
    int Mc = (int)(((M + splits - 1) / splits + 7) / 8 * 8);      // (a last partial stage is zero-filled: no multiple of the stage needed)
    const long want = splits;
    splits = (M + Mc - 1) / Mc;
    const bool xmap = xcd && splits == want;
    const dim3 grid = xmap ? dim3((unsigned)(tk * tn * splits)) : dim3((unsigned)tk, (unsigned)tn, (unsigned)splits);
    if (a16 && b16) k_gemm_tn_db<true, true><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, splits == 1 ? nullptr : partial, db ? bscratch : nullptr, Mc,
                                                                xmap ? tk : 0);
    else if (a16) k_gemm_tn_db<true><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, splits == 1 ? nullptr : partial, db ? bscratch : nullptr, Mc,
                                                   xmap ? tk : 0);
    else k_gemm_tn_db<false><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, splits == 1 ? nullptr : partial, db ? bscratch : nullptr, Mc,
                                                   xmap ? tk : 0);
    {       // one finishing launch: the split partials into dW and the row-range sums into db (two launches until round 5)
        const size_t NK = splits > 1 ? (size_t)N * K : 0, items = NK + (db ? (size_t)N : 0);
        if (items) k_tn_finish<<<(unsigned)((items + 255) / 256 > 4096 ? 4096 : (items + 255) / 256), 256, 0, st>>>((int)splits, N, K, NK ? partial : nullptr, C, ldc, db ? bscratch : nullptr, db);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// bf16 variant of the dW kernel (the encoder's bf16 training mode): C[n][k] (+)= sum_m A[m][n] B[m][k], A / B bf16
// row-major, fp32 accumulation and output.  v_mfma_f32_32x32x16_bf16 wants 8 CONSECUTIVE reduction indices per lane,
// and the reduction index m is the slow one in memory, so the tiles are transposed on their way into LDS: a thread loads
// 16 bytes (8 columns of one row) and writes them as eight 2-byte stores into the [column][m] image (row pitch 72 bytes:
// the two 8-byte fragment reads of a lane are conflict-free across the 32-lane groups, the 2-byte writes of the two
// column groups of a wave land on disjoint banks).  Tile 128 (n) x 128 (k), 32 rows of m per stage, 4 waves as 2 x 2.
// Arbitrary N, K (zero-filled loads, masked stores); lda / ldb multiples of 8, 16-byte aligned bases.
typedef __attribute__((ext_vector_type(16))) float f32x16;
__global__ __launch_bounds__(256) void k_gemm_tn_bf16(int M, int N, int K, const bf16_t *__restrict__ A, int lda,
                                                      const bf16_t *__restrict__ B, int ldb, float *C, int ldc,
                                                      float *partial, int Mc) {
    constexpr int PITCH = 72;
    __shared__ __attribute__((aligned(16))) unsigned char As[128 * PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[128 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    const int n0 = blockIdx.y * 128, k0 = blockIdx.x * 128;
    const int m_beg = blockIdx.z * Mc, m_end = min(M, m_beg + Mc);
    const int srow = tid & 31, sch = tid >> 5;                   // staging role: row of the stage, 8-column chunk (and + 8)
    auto ldchunk = [&](const bf16_t *P, int ld, int m, int col, int cols) -> u32x4 {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (m >= m_end || col >= cols) return v;
        const bf16_t *q = P + (size_t)m * ld + col;
        if (col + 8 <= cols) return *(const u32x4 *)q;
        unsigned short e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 8 && col + i < cols; ++i) e[i] = q[i];
        v[0] = e[0] | ((unsigned)e[1] << 16); v[1] = e[2] | ((unsigned)e[3] << 16);
        v[2] = e[4] | ((unsigned)e[5] << 16); v[3] = e[6] | ((unsigned)e[7] << 16);
        return v;
    };
    auto put = [&](unsigned char *S, int chunk, const u32x4 &v) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            *(unsigned short *)(S + (8 * chunk + e) * PITCH + srow * 2) = (unsigned short)(v[e >> 1] >> ((e & 1) * 16));
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    u32x4 ra[2], rb[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        ra[p] = ldchunk(A, lda, m_beg + srow, n0 + 8 * (sch + 8 * p), N);
        rb[p] = ldchunk(B, ldb, m_beg + srow, k0 + 8 * (sch + 8 * p), K);
    }
    for (int m0 = m_beg; m0 < m_end; m0 += 32) {
#pragma unroll
        for (int p = 0; p < 2; ++p) { put(As, sch + 8 * p, ra[p]); put(Bs, sch + 8 * p, rb[p]); }
        __syncthreads();
        if (m0 + 32 < m_end) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                ra[p] = ldchunk(A, lda, m0 + 32 + srow, n0 + 8 * (sch + 8 * p), N);
                rb[p] = ldchunk(B, ldb, m0 + 32 + srow, k0 + 8 * (sch + 8 * p), K);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned char *pa = As + (wr * 64 + i * 32 + (lane & 31)) * PITCH + ks * 32 + (lane >> 5) * 16;
                const unsigned char *pb = Bs + (wc * 64 + i * 32 + (lane & 31)) * PITCH + ks * 32 + (lane >> 5) * 16;
                const uint2 a0 = *(const uint2 *)pa, a1 = *(const uint2 *)(pa + 8), b0 = *(const uint2 *)pb, b1 = *(const uint2 *)(pb + 8);
                a[i] = (u32x4){a0.x, a0.y, a1.x, a1.y};
                b[i] = (u32x4){b0.x, b0.y, b1.x, b1.y};
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]), __builtin_bit_cast(bf16x8, b[j]),
                                                                       acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *dst = partial ? partial + (size_t)blockIdx.z * N * K : C;
    const int ldd = partial ? K : ldc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), k = k0 + wc * 64 + j * 32 + (lane & 31);
                if (n < N && k < K) {
                    if (partial) dst[(size_t)n * ldd + k] = acc[i][j][r];
                    else dst[(size_t)n * ldd + k] += acc[i][j][r];
                }
            }
}

int launch_gemm_tn_bf16(int M, int N, int K, const bf16_t *A, int lda, const bf16_t *B, int ldb, float *C, int ldc,
                        float *partial, hipStream_t st) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int tn = (N + 127) / 128, tk = (K + 127) / 128;
    long splits = 2048 / ((long)tn * tk);
    const long by_rows = (M + 511) / 512, by_cap = (long)(PART_CAP / ((size_t)N * K));
    splits = splits > by_rows ? by_rows : splits;
    splits = splits > by_cap ? by_cap : splits;
    if (splits < 1) splits = 1;
    int Mc = (int)(((M + splits - 1) / splits + 31) / 32 * 32);
    splits = (M + Mc - 1) / Mc;
    const dim3 grid((unsigned)tk, (unsigned)tn, (unsigned)splits);
    if (splits == 1) {
        k_gemm_tn_bf16<<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, nullptr, Mc);
    } else {
        k_gemm_tn_bf16<<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, partial, Mc);
        reduce_partial(splits, N, K, partial, C, ldc, st);
    }
    DA_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Launchers of the element-wise kernels at the top of the file, the transpose and the two-stage column sum
int gelu_fwd(size_t n, const float *src, float *dst, hipStream_t st, bf16_t *dst16) {
    k_gelu_fwd<<<grid_for(n), 256, 0, st>>>(n, src, dst, dst16);
    DA_LAUNCH_CHECK();
    return 0;
}
int gelu_bwd(size_t n, const float *pre, const float *dy, float *dx, hipStream_t st) {
    k_gelu_bwd<<<grid_for(n), 256, 0, st>>>(n, pre, dy, dx);
    DA_LAUNCH_CHECK();
    return 0;
}
int leaky_bwd(size_t n, const float *out, const float *dy, float *dx, hipStream_t st) {
    k_leaky_bwd<<<grid_for(n), 256, 0, st>>>(n, out, dy, dx);
    DA_LAUNCH_CHECK();
    return 0;
}
int launch_transpose_f32(int rows, int cols, const float *src, float *dst, hipStream_t st) {
    k_transpose<<<dim3((cols + 31) / 32, (rows + 31) / 32), 256, 0, st>>>(rows, cols, src, dst);
    DA_LAUNCH_CHECK();
    return 0;
}
int colsum_add(int M, int N, const float *A, int lda, float *out, float *scratch, hipStream_t st) {
    // at most ~32 row chunks (never more than the 128-row chunks the scratch is sized for): chunks * N floats of scratch
    const int rows_per = max(128, ((M + 31) / 32 + 3) / 4 * 4), chunks = (M + rows_per - 1) / rows_per;
    k_colsum_partial<<<dim3((N + 63) / 64, chunks), 256, 0, st>>>(M, N, A, lda, rows_per, scratch);
    k_colsum_finish<<<(N + 63) / 64, 256, 0, st>>>(chunks, N, scratch, out);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da
