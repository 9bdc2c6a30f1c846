// Puzzle and piece accuracy of a whole 2D Batch in one launch: the scoring that follows every sampling loop
// of validation_step / test_step, spatial_diffusion.py:775-856, 915-955 -- per puzzle two greedy_cost_assignment calls
// (ground truth -> grid, prediction -> grid), two sorts by row, the comparison of the assigned cells and, with rotation, a
// cosine test.
//
// k_score2d: one workgroup of 1024 threads per puzzle.  The puzzle's cell centres are staged in LDS once; waves 0-7 run the
// greedy assignment of the ground truth, waves 8-15 that of the prediction, in the same loop: both have min(n, m) steps, so
// they share every barrier.  Each half is k_greedy_assign (da_assign.hip) on 512 threads -- the same dist2, the same
// lexicographic (value, index) minima, whose result does not depend on how many lanes reduce them -- and instead of the
// (row, column, distance) list it fills a row -> column table in LDS: table[i] is what the reference reads after sorting its
// assignments by row.  The epilogue compares the two tables piece by piece, applies the cosine test and reduces the counts.
// No atomics, nothing crosses workgroups, every result leaves through plain stores.
#include <math.h>

#include "da_assign_common.h"      // dist2, lexmin

namespace da {
namespace {

constexpr int S2_THREADS = 1024;
constexpr int S2_HALF = S2_THREADS / 2;            // threads per assignment problem
constexpr int S2_HWAVES = S2_HALF / 64;            // waves per assignment problem
constexpr int S2_FIXED = 96;                       // words of LDS next to the arrays sized by the puzzle: redv 16, redi 16, bcast 8, cnt 48

// LDS floats of a puzzle of n pieces and m cells: the grid [m][2], then per half rmin [n], rarg [n], cell [n], cused [m]
__host__ __device__ inline size_t s2_lds_floats(int n, int m) { return (size_t)2 * m + 2 * ((size_t)3 * n + m) + S2_FIXED; }

// torch.cosine_similarity of two 2-vectors (each divided by its norm clamped at eps = 1e-8, then the dot product) against
// cos(pi / 4) as fp32; a NaN compares false
__device__ __forceinline__ bool rot_ok(const float *a, const float *b) {
#pragma clang fp contract(off)
    const float na = fmaxf(sqrtf(a[0] * a[0] + a[1] * a[1]), 1e-8f), nb = fmaxf(sqrtf(b[0] * b[0] + b[1] * b[1]), 1e-8f);
    const float c = (a[0] / na) * (b[0] / nb) + (a[1] / na) * (b[1] / nb);
    return c > (float)0.7071067811865476;
}

__global__ __launch_bounds__(S2_THREADS) void k_score2d(const float *__restrict__ pred, int ld_pred, const float *__restrict__ gt, int ld_gt,
                                                         const float *__restrict__ grid, int ld_grid,
                                                         const int32_t *__restrict__ ptr_piece, const int32_t *__restrict__ ptr_cell,
                                                         int max_n, int max_m, int rotation, int32_t *__restrict__ cell_pred,
                                                         int32_t *__restrict__ cell_gt, uint8_t *__restrict__ piece_ok,
                                                         int32_t *__restrict__ per_puzzle) {
    extern __shared__ float sm[];
    const int g = blockIdx.x;
    const int r0 = ptr_piece[g], n = ptr_piece[g + 1] - r0, c0 = ptr_cell[g], m = ptr_cell[g + 1] - c0;
    const int tid = threadIdx.x;
    // more pieces than cells (the reference compares two different row sets then), or sizes the launch reserved no LDS for:
    // the whole workgroup leaves before the first barrier
    if (n < 0 || m < 0 || n > m || n > max_n || m > max_m) {
        if (tid == 0) per_puzzle[(size_t)g * 4] = -1;
        return;
    }
    const int half = tid >> 9, ht = tid & (S2_HALF - 1), lane = tid & 63, hw = ht >> 6, wv = tid >> 6;
    float *p2 = sm;                                            // [m][2]
    float *hb = p2 + 2 * m + (size_t)half * (3 * n + m);       // this half's arrays
    float *rmin = hb;                                          // [n] smallest free distance of the row (+inf once retired)
    int *rarg = (int *)(rmin + n);                             // [n] its column
    int *cell = rarg + n;                                      // [n] row -> assigned column
    int *cused = cell + n;                                     // [m]
    int *fixed = (int *)(p2 + 2 * m + 2 * (size_t)(3 * n + m));
    float *redv = (float *)fixed + half * S2_HWAVES;           // [2][8]
    int *redi = fixed + 16 + half * S2_HWAVES;                 // [2][8]
    int *bcast = fixed + 32 + half;                            // [2]: the column each half retired
    int *cnt = fixed + 40;                                     // [3][16] the epilogue's counts per wave
    const float *pos = half ? pred : gt;                       // half 0: ground truth -> grid, half 1: prediction -> grid
    const int ld = half ? ld_pred : ld_gt;
    for (int j = tid; j < m; j += S2_THREADS) {
        p2[2 * j] = grid[(size_t)(c0 + j) * ld_grid];
        p2[2 * j + 1] = grid[(size_t)(c0 + j) * ld_grid + 1];
    }
    for (int j = ht; j < m; j += S2_HALF) cused[j] = 0;
    for (int i = ht; i < n; i += S2_HALF) cell[i] = 0;
    __syncthreads();
    auto rescan = [&](int i) {                                 // one wave: smallest free column of row i
        const float a[2] = {pos[(size_t)(r0 + i) * ld], pos[(size_t)(r0 + i) * ld + 1]};
        float v = INFINITY;
        int c = 0x7fffffff;
        for (int j = lane; j < m; j += 64)
            if (!cused[j]) lexmin(v, c, dist2(a, p2 + 2 * j), j);
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o);
            const int c2 = __shfl_xor(c, o);
            lexmin(v, c, v2, c2);
        }
        if (lane == 0) { rmin[i] = v; rarg[i] = c; }
    };
    for (int i = hw; i < n; i += S2_HWAVES) rescan(i);
    __syncthreads();
    for (int k = 0; k < n; ++k) {                              // n = min(n, m)
        // (a) argmin over rows, ties -> smallest row (its cached column is already the smallest of the row)
        float v = INFINITY;
        int i = 0x7fffffff;
        for (int r = ht; r < n; r += S2_HALF) lexmin(v, i, rmin[r], r);
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o);
            const int i2 = __shfl_xor(i, o);
            lexmin(v, i, v2, i2);
        }
        if (lane == 0) { redv[hw] = v; redi[hw] = i; }
        __syncthreads();
        if (ht == 0) {                                         // (b) retire the row and its column
            for (int w = 1; w < S2_HWAVES; ++w) lexmin(v, i, redv[w], redi[w]);
            if (i >= n) {                                      // cannot happen with finite rmin; never index past LDS
                i = 0;
                while (i < n - 1 && !(rmin[i] < INFINITY)) ++i;
            }
            int j = rarg[i];
            j = j < 0 ? 0 : (j >= m ? m - 1 : j);
            *bcast = j;
            cell[i] = j;
            rmin[i] = INFINITY;
            cused[j] = 1;
        }
        __syncthreads();
        // (c) rows that pointed at the retired column look again
        const int jr = *bcast;
        for (int r = hw; r < n; r += S2_HWAVES)
            if (rmin[r] < INFINITY && rarg[r] == jr) rescan(r);
        __syncthreads();
    }
    // epilogue: piece i sits on the same cell in both assignments (and points the same way)
    const int *cell_g = (const int *)(p2 + 2 * m) + 2 * n, *cell_p = cell_g + (3 * n + m);
    int n_ok = 0, n_pos = 0, n_rot = 0;
    for (int i = tid; i < n; i += S2_THREADS) {
        const int cg = cell_g[i], cp = cell_p[i];
        const bool pos_ok = cg == cp;
        const bool r_ok = !rotation || rot_ok(pred + (size_t)(r0 + i) * ld_pred + 2, gt + (size_t)(r0 + i) * ld_gt + 2);
        if (cell_gt) cell_gt[r0 + i] = cg;
        if (cell_pred) cell_pred[r0 + i] = cp;
        piece_ok[r0 + i] = (uint8_t)(pos_ok && r_ok);
        n_pos += pos_ok;
        n_rot += r_ok;
        n_ok += pos_ok && r_ok;
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_ok += __shfl_xor(n_ok, o);
        n_pos += __shfl_xor(n_pos, o);
        n_rot += __shfl_xor(n_rot, o);
    }
    if (lane == 0) { cnt[wv] = n_ok; cnt[16 + wv] = n_pos; cnt[32 + wv] = n_rot; }
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0, c = 0;
        for (int w = 0; w < S2_THREADS / 64; ++w) { a += cnt[w]; b += cnt[16 + w]; c += cnt[32 + w]; }
        int32_t *o = per_puzzle + (size_t)g * 4;
        o[0] = a == n; o[1] = a; o[2] = b; o[3] = c;
    }
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" int da_score2d(int n_puzzles, const float *pred, int ld_pred, const float *gt, int ld_gt, const float *grid, int ld_grid,
                          const int32_t *ptr_piece, const int32_t *ptr_cell, int max_n, int max_m, int rotation,
                          int32_t *cell_pred, int32_t *cell_gt, uint8_t *piece_ok, int32_t *per_puzzle, void *stream) {
    DA_REQUIRE(pred && gt && grid && ptr_piece && ptr_cell && piece_ok && per_puzzle, "da_score2d: null argument");
    const int cols = rotation ? 4 : 2;
    DA_REQUIRE(n_puzzles > 0 && max_n > 0 && max_m > 0 && ld_pred >= cols && ld_gt >= cols && ld_grid >= 2,
               "da_score2d: bad sizes (%d puzzles, max %d x %d, ld %d / %d / %d, rotation %d)", n_puzzles, max_n, max_m, ld_pred, ld_gt,
               ld_grid, rotation);
    DA_REQUIRE(max_n <= max_m, "da_score2d: more pieces than cells (%d > %d): the reference compares different row sets there", max_n, max_m);
    const size_t lds = s2_lds_floats(max_n, max_m) * 4;
    DA_REQUIRE(lds <= 160 * 1024, "da_score2d: puzzle too large for one workgroup (%d x %d needs %zu bytes of LDS)", max_n, max_m, lds);
    static bool attr_done[16] = {};           // per device: the attribute belongs to the device's copy of the function
    int dev = 0;
    DA_CHECK_HIP(hipGetDevice(&dev));
    if (lds > 48 * 1024 && !attr_done[dev & 15]) {
        DA_CHECK_HIP(hipFuncSetAttribute((const void *)k_score2d, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_done[dev & 15] = true;
    }
    k_score2d<<<n_puzzles, S2_THREADS, lds, (hipStream_t)stream>>>(pred, ld_pred, gt, ld_gt, grid, ld_grid, ptr_piece, ptr_cell, max_n, max_m,
                                                                   rotation, cell_pred, cell_gt, piece_ok, per_puzzle);
    DA_LAUNCH_CHECK();
    return 0;
}
