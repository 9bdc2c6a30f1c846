// The assembled puzzles of a 2D Batch as RGBA pictures, every requested (step, puzzle) frame in one launch:
// the compositing of create_image_from_patches, spatial_diffusion.py:1204-1234 -- per piece a 32x32 crop turned into
// bytes, padded to 46x46 with transparent pixels, rotated about (23, 23) by PIL's nearest-neighbour rule and pasted with its
// own alpha as the mask, later pieces over earlier ones.
//
// k_render2d: one workgroup of 256 threads per 32x32 tile of one frame's canvas (the canvas is 32 rows x 32 cols pixels, so
// the tiles are the puzzle's cells).  The workgroup walks its puzzle's pieces from the LAST index down in chunks of 256: every
// thread places one piece (the position arithmetic of the reference in fp32, uncontracted), the pieces whose 46x46 box meets
// the tile are compacted into LDS in that descending order (ballot + prefix, no atomics), and every thread then walks the
// list for its four pixels: canvas pixel -> pixel of the rotated tile -> pixel of the padded tile through the 16.16 fixed-point
// inverse map PIL uses (six ints per (frame, piece), made on the host: they are fp64 trigonometry rounded to 15 decimals),
// first opaque hit wins.  A chunk never overflows the list (at most 256 candidates), so all pieces on one spot are just more
// chunks; the walk stops as soon as every pixel of the tile is covered.  Each thread writes its four pixels with one 16-byte
// store; nothing crosses workgroups, the bytes are the same on every run.
#include <math.h>

#include "da_common.h"

namespace da {
namespace {

constexpr int R2_THREADS = 256;
constexpr int R2_PATCH = 32;                       // crop and canvas-tile edge
constexpr int R2_PAD = 7;                          // transparent border of the padded tile
constexpr int R2_BOX = R2_PATCH + 2 * R2_PAD;      // 46
constexpr int R2_HALF = R2_BOX / 2;                // 23: the paste offset and the centre of rotation
constexpr int R2_PUZ = 8;                          // ints per puzzle: first piece, pieces, rows, cols, x scale, y scale (float bits), byte offset lo, hi

// int((v + 1) * extent / 2) - 23 with the reference's operation order; false: the pose is not finite (or beyond any canvas)
__device__ __forceinline__ bool place(float pos, float scale, int extent, int &out) {
#pragma clang fp contract(off)
    const float v = pos * scale;
    const float t = (v + 1.0f) * (float)extent / 2.0f;
    if (!(fabsf(t) < 1.0e9f)) return false;        // NaN, inf, or further out than an int holds: nothing of it is on the canvas
    out = (int)t - R2_HALF;                        // truncation toward zero, as int() of the reference
    return true;
}

__device__ __forceinline__ unsigned to_byte(float v) {
#pragma clang fp contract(off)
    return (unsigned)(int)(v * 255.0f) & 255u;
}

__global__ __launch_bounds__(R2_THREADS) void k_render2d(int n_puzzles, int n_pieces, int max_tiles, const float *__restrict__ patches,
                                                          const float *__restrict__ poses, int ld_pose, long long step_stride,
                                                          const int32_t *__restrict__ coef, const int32_t *__restrict__ puzzles,
                                                          long long step_bytes, uint8_t *__restrict__ out) {
    __shared__ int cand[R2_THREADS][9];            // piece, x_pos, y_pos, a0 .. a5 (9 ints: odd stride, no bank conflicts)
    __shared__ int wave_hits[R2_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long frame = blockIdx.x / max_tiles;
    const int tile = (int)(blockIdx.x % max_tiles);
    const int k = (int)(frame / n_puzzles), g = (int)(frame % n_puzzles);
    const int32_t *pz = puzzles + (size_t)g * R2_PUZ;
    const int r0 = pz[0], n = pz[1], rows = pz[2], cols = pz[3];
    const float sx = __int_as_float(pz[4]), sy = __int_as_float(pz[5]);
    const long long off = (long long)(((unsigned long long)(unsigned)pz[7] << 32) | (unsigned)pz[6]);
    // uniform per workgroup, before the first barrier: tiles this puzzle does not have, and tables that point outside the buffers
    if (rows < 1 || cols < 1 || tile >= rows * cols) return;
    const int W = R2_PATCH * cols, H = R2_PATCH * rows;
    if (r0 < 0 || n < 0 || (long long)r0 + n > n_pieces || off < 0 || (off & 15) || off + (long long)W * H * 4 > step_bytes) return;
    const int X0 = (tile % cols) * R2_PATCH, Y0 = (tile / cols) * R2_PATCH;
    const int px = X0 + (tid & 7) * 4, py = Y0 + (tid >> 3);         // this thread's four pixels: (px .. px + 3, py)
    const float *pose_k = poses + (size_t)k * step_stride;
    const int32_t *coef_k = coef ? coef + (size_t)k * n_pieces * 6 : nullptr;
    unsigned rgba[4] = {0u, 0u, 0u, 0u};
    unsigned open = 15u;                                             // pixels not covered yet
    for (int hi = n; hi > 0; hi -= R2_THREADS) {
        // place piece hi - 1 - tid; keep it when its box meets the tile
        const int i = hi - 1 - tid;
        int xp = 0, yp = 0;
        bool hit = false;
        if (i >= 0) {
            const float *row = pose_k + (size_t)(r0 + i) * ld_pose;
            hit = place(row[0], sx, W, xp) && place(row[1], sy, H, yp);
            hit = hit && xp < X0 + R2_PATCH && xp + R2_BOX > X0 && yp < Y0 + R2_PATCH && yp + R2_BOX > Y0;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wave_hits[wv] = __popcll(b);
        __syncthreads();
        int slot = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < R2_THREADS / 64; ++w) {
            if (w < wv) slot += wave_hits[w];
            total += wave_hits[w];
        }
        if (hit) {
            int *c = cand[slot];
            c[0] = r0 + i; c[1] = xp; c[2] = yp;
            if (coef_k) {
                const int32_t *a = coef_k + (size_t)(r0 + i) * 6;
                for (int q = 0; q < 6; ++q) c[3 + q] = a[q];
            } else {                                                 // no rotation: the identity map, sampled at pixel centres
                c[3] = 65536; c[4] = 0; c[5] = 32768; c[6] = 0; c[7] = 65536; c[8] = 32768;
            }
        }
        __syncthreads();
        for (int e = 0; e < total && open; ++e) {                    // descending piece index: the first opaque hit is on top
            const int *c = cand[e];
            const int dy = py - c[2];
            if (dy < 0 || dy >= R2_BOX) continue;
            for (int q = 0; q < 4; ++q) {
                if (!(open & (1u << q))) continue;
                const int dx = px + q - c[1];
                if (dx < 0 || dx >= R2_BOX) continue;
                const int xin = (c[5] + c[3] * dx + c[4] * dy) >> 16, yin = (c[8] + c[6] * dx + c[7] * dy) >> 16;
                const int u = xin - R2_PAD, v = yin - R2_PAD;         // inside the crop <=> opaque
                if (u < 0 || u >= R2_PATCH || v < 0 || v >= R2_PATCH) continue;
                const float *src = patches + (size_t)c[0] * (3 * R2_PATCH * R2_PATCH) + v * R2_PATCH + u;
                rgba[q] = to_byte(src[0]) | (to_byte(src[R2_PATCH * R2_PATCH]) << 8) | (to_byte(src[2 * R2_PATCH * R2_PATCH]) << 16) | 0xff000000u;
                open &= ~(1u << q);
            }
        }
        if (__syncthreads_count(open != 0u) == 0) break;             // the tile is covered (also the barrier before cand is refilled)
    }
    uint4 *dst = (uint4 *)(out + (size_t)k * step_bytes + off + ((size_t)py * W + px) * 4);
    *dst = make_uint4(rgba[0], rgba[1], rgba[2], rgba[3]);
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" long long da_render2d_frame_bytes(int rows, int cols) {
    if (rows < 1 || cols < 1) return 0;
    return (long long)R2_PATCH * rows * R2_PATCH * cols * 4;
}

extern "C" int da_render2d(int n_steps, int n_puzzles, int n_pieces, int max_tiles, const float *patches, const float *poses, int ld_pose,
                           long long step_stride, const int32_t *coef, const int32_t *puzzles, long long step_bytes, uint8_t *out,
                           void *stream) {
    DA_REQUIRE(patches && poses && puzzles && out, "da_render2d: null argument");
    DA_REQUIRE(n_steps > 0 && n_puzzles > 0 && n_pieces > 0 && max_tiles > 0 && ld_pose >= 2 && step_stride >= 0 && step_bytes > 0,
               "da_render2d: bad sizes (%d steps, %d puzzles, %d pieces, %d tiles, ld %d, step stride %lld, %lld bytes per step)", n_steps,
               n_puzzles, n_pieces, max_tiles, ld_pose, step_stride, step_bytes);
    DA_REQUIRE((step_bytes & 15) == 0 && ((uintptr_t)out & 15) == 0, "da_render2d: the frame buffer and its steps are 16-byte aligned");
    const long long blocks = (long long)n_steps * n_puzzles * max_tiles;
    // a launch holds fewer than 2^32 threads
    DA_REQUIRE(blocks * R2_THREADS <= 0xffffffffLL, "da_render2d: %lld tiles in one launch (at most 2^24 - 1): pass fewer steps", blocks);
    k_render2d<<<(unsigned)blocks, R2_THREADS, 0, (hipStream_t)stream>>>(n_puzzles, n_pieces, max_tiles, patches, poses, ld_pose, step_stride,
                                                                         coef, puzzles, step_bytes, out);
    DA_LAUNCH_CHECK();
    return 0;
}
