// Resize a Batch's pictures: PIL.Image.resize(size, resample, box) for 8-bit RGB, byte for byte, for every picture of
// a Batch in one launch -- the img.resize((32 cols, 32 rows)) at the head of every get() of the reference's
// dataset/puzzle_dataset.py (:266, :344, :413, :517 bicubic, :590 Lanczos) and the RandomHorizontalFlip /
// RandomCropAndResizedToOriginal pair of its `hard` augmentation (:155-172).  PIL's method is two separable integer passes:
// horizontally, then vertically, each output byte = clamp((2^21 + sum of byte * coefficient) >> 22, 0, 255) in int32 with 22-bit
// coefficients, the horizontal result rounded to uint8 before the vertical pass reads it.  The coefficient and bound tables are
// made on the host in fp64 (diffassemble_amd/resize2d.py); nothing here is floating point.  A pass PIL skips arrives as the
// identity table (one coefficient 2^22 per output: (2^21 + v * 2^22) >> 22 = v).
//
// k_resize_fused: one workgroup of 256 threads per 64-row x 32-column tile of one picture's OUTPUT.
//   window  the source rows the tile's vertical pass reads: [bounds_v[Y0].first, bounds_v[Y1 - 1].first + .count) (the bounds
//           do not decrease with the output index); at most RS_WINDOW = 256 rows, else the host takes the two-pass route.
//   h pass  thread i takes pixel (row i / 32 of the window, column i % 32 of the tile): three int32 sums over the source row
//           in global memory (the taps' 3 n bytes are contiguous and are read as words, see h_pixel), rounded, clamped and
//           written as three bytes of the LDS tile T[row][3 c + ch], 96 bytes a row.
//           With `flip` column c of the tile holds result column out_w - 1 - (X0 + c): the mirror is applied to the stage's
//           OUTPUT, as RandomHorizontalFlip after the resize does, never to the source.
//   v pass  thread i takes 16 bytes of an output row (row i / 6, segment i % 6): per tap one ds_read_b128 of T and one
//           coefficient, sixteen int32 sums, then ONE 16-byte store where the row is 16-byte aligned (out_w * 3 a multiple of
//           16, as with puzzle-sized pictures: rows of 96 cols bytes) and byte stores otherwise.
//   LDS     24 KB of bytes, integer only.  Rows lie 96 bytes apart, unpadded: the 16-byte reads want 16-byte aligned rows, and
//           the 6 segments of a row are 6 distinct 16-byte slots of the 256-byte bank row; rows 8 apart (768 = 3 x 256 bytes)
//           share slots.  Scaling up, neighbouring output rows read the same window rows (one address: a broadcast).  The
//           conflicts were not counted (no SQ_LDS_BANK_CONFLICT run); the kernel's time is in its loads, DESIGN 3s.
// k_resize_h / k_resize_v: the two-pass route, PIL's own order, for windows that do not fit: one thread per pixel, the
// horizontal result of the rows [row0, row0 + rows) the vertical pass needs in a caller-provided uint8 workspace.
// Both routes run the same sums in the same order on the same bytes.  No atomics, nothing crosses workgroups.
#include "da_common.h"

namespace da {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TW = 32;                          // tile columns
constexpr int RS_TH = 64;                          // tile rows
constexpr int RS_ROW = 3 * RS_TW;                  // 96: bytes of one row of the LDS tile
constexpr int RS_WINDOW = 256;                     // source rows one tile may need (24 KB of LDS)
constexpr int RS_PIC = 24;                         // ints per picture, see include/diffassemble_hip.h
constexpr int RS_HALF = 1 << 21, RS_BITS = 22;
// byte * coefficient is a 24-bit multiply (v_mad_i32_i24, full rate; a 32-bit integer multiply runs at a quarter of it): the host
// makes no table with a coefficient of 2^23 or more in magnitude (the largest weight PIL's filters reach is about 1.3 * 2^22).

struct Picture {
    long long src, dst, ws;
    int in_h, in_w, out_h, out_w, flip, hb, hc, hk, vb, vc, vk, tile0, tiles_x, hblock0, vblock0, row0, rows;
};

__device__ inline long long word64(int lo, int hi) { return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo); }

__device__ inline Picture load_picture(const int32_t *p) {
    Picture q;
    q.src = word64(p[0], p[1]); q.in_h = p[2]; q.in_w = p[3];
    q.dst = word64(p[4], p[5]); q.out_h = p[6]; q.out_w = p[7];
    q.flip = p[8]; q.hb = p[9]; q.hc = p[10]; q.hk = p[11]; q.vb = p[12]; q.vc = p[13]; q.vk = p[14];
    q.tile0 = p[15]; q.tiles_x = p[16]; q.hblock0 = p[17]; q.vblock0 = p[18]; q.row0 = p[19]; q.rows = p[20];
    q.ws = word64(p[21], p[22]);
    return q;
}

// everything a table entry could point outside of: uniform per workgroup, a picture that fails writes nothing
__device__ inline bool picture_ok(const Picture &q, long long src_bytes, long long dst_bytes, long long n_table) {
    if (q.in_h < 1 || q.in_w < 1 || q.out_h < 1 || q.out_w < 1 || q.in_h > (1 << 24) || q.in_w > (1 << 24) || q.out_h > (1 << 24) ||
        q.out_w > (1 << 24))
        return false;
    if (q.src < 0 || q.src + 3LL * q.in_h * q.in_w > src_bytes || q.dst < 0 || q.dst + 3LL * q.out_h * q.out_w > dst_bytes) return false;
    if (q.hk < 1 || q.vk < 1 || q.hb < 0 || q.hc < 0 || q.vb < 0 || q.vc < 0) return false;
    if (q.hb + 2LL * q.out_w > n_table || q.hc + (long long)q.hk * q.out_w > n_table) return false;
    if (q.vb + 2LL * q.out_h > n_table || q.vc + (long long)q.vk * q.out_h > n_table) return false;
    return true;
}

// the last picture whose first block (int `field` of its descriptor) is <= b
__device__ inline int find_picture(const int32_t *pictures, int n_pictures, int field, int b) {
    int lo = 0, hi = n_pictures - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pictures[(size_t)mid * RS_PIC + field] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// clamp((v >> 22), 0, 255), written as a clamp of v followed by the shift.  Not `v >>= 22` followed by the clamp: hipcc (ROCm 7)
// turns two of those that are packed into one word into v_ashr_pk_u8_i32, whose result it takes to be zero above bit 15, while
// the MI355X leaves the destination's old bits 16 .. 31 in place -- bytes 2 of a packed word came back OR-ed with stale values.
__device__ inline int clip8(int v) {
    v = v < 0 ? 0 : v;
    v = v > (256 << RS_BITS) - 1 ? (256 << RS_BITS) - 1 : v;
    return (int)((unsigned)v >> RS_BITS);
}

// `bytes` (1 .. 4) source bytes at p as one word, low byte first.  memcpy of the exact size: the compiler turns it into one load of
// that size where the device reads unaligned words (it does), and nothing beyond the picture's last byte is touched.
template <int bytes> __device__ inline unsigned load_bytes(const uint8_t *p) {
    unsigned v = 0;
    if (bytes == 3) {
        unsigned short lo;
        __builtin_memcpy(&lo, p, 2);
        return (unsigned)lo | ((unsigned)p[2] << 16);
    }
    __builtin_memcpy(&v, p, bytes);
    return v;
}

__device__ inline int byte_of(unsigned w, int i) { return (int)((w >> (8 * i)) & 255u); }

// the three sums of result pixel (source row `row`, result column xx) of the horizontal pass, as 3 bytes in one int.  The taps'
// 3 n source bytes are contiguous: four taps are read as three words, two as a word and a half, one as a half and a byte (a
// byte load per channel and tap made the kernel wait on its load instructions, not on memory); the sums run in tap order.
__device__ inline unsigned h_pixel(const Picture &q, const uint8_t *__restrict__ src, const int32_t *__restrict__ tables, int row, int xx) {
    int xmin = tables[q.hb + 2 * xx], n = tables[q.hb + 2 * xx + 1];
    if (xmin < 0 || n < 0 || n > q.hk || xmin + n > q.in_w) n = 0;
    const int32_t *k = tables + q.hc + (size_t)xx * q.hk;
    const uint8_t *s = src + q.src + ((long long)row * q.in_w + xmin) * 3;
    int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF;
    int x = 0;
    for (; x + 4 <= n; x += 4, s += 12) {
        const unsigned w0 = load_bytes<4>(s), w1 = load_bytes<4>(s + 4), w2 = load_bytes<4>(s + 8);
        const int c0 = k[x], c1 = k[x + 1], c2 = k[x + 2], c3 = k[x + 3];
        a0 += __mul24(byte_of(w0, 0), c0); a1 += __mul24(byte_of(w0, 1), c0); a2 += __mul24(byte_of(w0, 2), c0);
        a0 += __mul24(byte_of(w0, 3), c1); a1 += __mul24(byte_of(w1, 0), c1); a2 += __mul24(byte_of(w1, 1), c1);
        a0 += __mul24(byte_of(w1, 2), c2); a1 += __mul24(byte_of(w1, 3), c2); a2 += __mul24(byte_of(w2, 0), c2);
        a0 += __mul24(byte_of(w2, 1), c3); a1 += __mul24(byte_of(w2, 2), c3); a2 += __mul24(byte_of(w2, 3), c3);
    }
    if (x + 2 <= n) {
        const unsigned w0 = load_bytes<4>(s), w1 = load_bytes<2>(s + 4);
        const int c0 = k[x], c1 = k[x + 1];
        a0 += __mul24(byte_of(w0, 0), c0); a1 += __mul24(byte_of(w0, 1), c0); a2 += __mul24(byte_of(w0, 2), c0);
        a0 += __mul24(byte_of(w0, 3), c1); a1 += __mul24(byte_of(w1, 0), c1); a2 += __mul24(byte_of(w1, 1), c1);
        x += 2;
        s += 6;
    }
    if (x < n) {
        const unsigned w0 = load_bytes<3>(s);
        const int c0 = k[x];
        a0 += __mul24(byte_of(w0, 0), c0); a1 += __mul24(byte_of(w0, 1), c0); a2 += __mul24(byte_of(w0, 2), c0);
    }
    return (unsigned)clip8(a0) | ((unsigned)clip8(a1) << 8) | ((unsigned)clip8(a2) << 16);
}

__global__ __launch_bounds__(RS_THREADS) void k_resize_fused(int n_pictures, const uint8_t *__restrict__ src, long long src_bytes,
                                                              const int32_t *__restrict__ pictures, const int32_t *__restrict__ tables,
                                                              long long n_table, uint8_t *__restrict__ dst, long long dst_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t T[RS_WINDOW * RS_ROW];
    const int tid = threadIdx.x;
    const int g = find_picture(pictures, n_pictures, 15, (int)blockIdx.x);
    const Picture q = load_picture(pictures + (size_t)g * RS_PIC);
    if (!picture_ok(q, src_bytes, dst_bytes, n_table)) return;
    const int t = (int)blockIdx.x - q.tile0;
    if (t < 0 || q.tiles_x != (q.out_w + RS_TW - 1) / RS_TW) return;
    const int ty = t / q.tiles_x, tx = t % q.tiles_x;
    const int Y0 = ty * RS_TH, X0 = tx * RS_TW;
    if (Y0 >= q.out_h) return;
    const int Y1 = min(Y0 + RS_TH, q.out_h), cols = min(RS_TW, q.out_w - X0);
    const int r0 = tables[q.vb + 2 * Y0];
    const int r1 = tables[q.vb + 2 * (Y1 - 1)] + tables[q.vb + 2 * (Y1 - 1) + 1];
    const int nrows = r1 - r0;
    if (r0 < 0 || r1 > q.in_h || nrows < 1 || nrows > RS_WINDOW) return;

    for (int i = tid; i < nrows * RS_TW; i += RS_THREADS) {
        const int r = i / RS_TW, c = i % RS_TW;
        unsigned v = 0;
        if (c < cols) {
            const int X = X0 + c;
            v = h_pixel(q, src, tables, r0 + r, q.flip ? q.out_w - 1 - X : X);
        }
        uint8_t *o = T + r * RS_ROW + 3 * c;
        o[0] = (uint8_t)v;
        o[1] = (uint8_t)(v >> 8);
        o[2] = (uint8_t)(v >> 16);
    }
    __syncthreads();

    const int row_bytes = 3 * cols;
    const long long out_ld = 3LL * q.out_w;
    const bool aligned = (((uintptr_t)dst | (unsigned long long)q.dst | (unsigned long long)out_ld) & 15) == 0;
    for (int i = tid; i < (Y1 - Y0) * 6; i += RS_THREADS) {
        const int y = Y0 + i / 6, s = i % 6;
        if (16 * s >= row_bytes) continue;
        int ymin = tables[q.vb + 2 * y], n = tables[q.vb + 2 * y + 1];
        if (ymin < r0 || n < 0 || n > q.vk || ymin + n > r1) n = 0;
        const int32_t *k = tables + q.vc + (size_t)y * q.vk;
        const uint8_t *col = T + (ymin - r0) * RS_ROW + 16 * s;
        int acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = RS_HALF;
        for (int x = 0; x < n; ++x) {
            const int c = k[x];
            const uint4 v = *(const uint4 *)(col + x * RS_ROW);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += __mul24((int)((w[j >> 2] >> (8 * (j & 3))) & 255u), c);
        }
        unsigned o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
            o[d] = (unsigned)clip8(acc[4 * d]) | ((unsigned)clip8(acc[4 * d + 1]) << 8) | ((unsigned)clip8(acc[4 * d + 2]) << 16) |
                   ((unsigned)clip8(acc[4 * d + 3]) << 24);
        uint8_t *out = dst + q.dst + (long long)y * out_ld + 3LL * X0 + 16 * s;
        if (aligned && 16 * s + 16 <= row_bytes) {
            *(uint4 *)out = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            const int left = min(16, row_bytes - 16 * s);
            for (int j = 0; j < left; ++j) out[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// two-pass route, horizontal: the workspace of a picture is [rows][out_w][3] uint8, source rows row0 .. row0 + rows - 1
__global__ __launch_bounds__(RS_THREADS) void k_resize_h(int n_pictures, const uint8_t *__restrict__ src, long long src_bytes,
                                                          const int32_t *__restrict__ pictures, const int32_t *__restrict__ tables,
                                                          long long n_table, long long dst_bytes, uint8_t *__restrict__ ws, long long ws_bytes) {
    const int g = find_picture(pictures, n_pictures, 17, (int)blockIdx.x);
    const Picture q = load_picture(pictures + (size_t)g * RS_PIC);
    if (!picture_ok(q, src_bytes, dst_bytes, n_table)) return;
    if (q.row0 < 0 || q.rows < 1 || q.row0 + q.rows > q.in_h || q.ws < 0 || q.ws + 3LL * q.rows * q.out_w > ws_bytes) return;
    const long long i = ((long long)blockIdx.x - q.hblock0) * RS_THREADS + threadIdx.x;
    if (i < 0 || i >= (long long)q.rows * q.out_w) return;
    const int r = (int)(i / q.out_w), X = (int)(i % q.out_w);
    const unsigned v = h_pixel(q, src, tables, q.row0 + r, q.flip ? q.out_w - 1 - X : X);
    uint8_t *o = ws + q.ws + 3 * i;
    o[0] = (uint8_t)v;
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)(v >> 16);
}

__global__ __launch_bounds__(RS_THREADS) void k_resize_v(int n_pictures, long long src_bytes, const int32_t *__restrict__ pictures,
                                                          const int32_t *__restrict__ tables, long long n_table, uint8_t *__restrict__ dst,
                                                          long long dst_bytes, const uint8_t *__restrict__ ws, long long ws_bytes) {
    const int g = find_picture(pictures, n_pictures, 18, (int)blockIdx.x);
    const Picture q = load_picture(pictures + (size_t)g * RS_PIC);
    if (!picture_ok(q, src_bytes, dst_bytes, n_table)) return;
    if (q.row0 < 0 || q.rows < 1 || q.row0 + q.rows > q.in_h || q.ws < 0 || q.ws + 3LL * q.rows * q.out_w > ws_bytes) return;
    const long long i = ((long long)blockIdx.x - q.vblock0) * RS_THREADS + threadIdx.x;
    if (i < 0 || i >= (long long)q.out_h * q.out_w) return;
    const int y = (int)(i / q.out_w), X = (int)(i % q.out_w);
    int ymin = tables[q.vb + 2 * y], n = tables[q.vb + 2 * y + 1];
    if (ymin < q.row0 || n < 0 || n > q.vk || ymin + n > q.row0 + q.rows) n = 0;
    const int32_t *k = tables + q.vc + (size_t)y * q.vk;
    const uint8_t *s = ws + q.ws + ((long long)(ymin - q.row0) * q.out_w + X) * 3;
    const long long ld = 3LL * q.out_w;
    int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF;
    for (int x = 0; x < n; ++x) {
        const int c = k[x];
        a0 += __mul24((int)s[x * ld], c);
        a1 += __mul24((int)s[x * ld + 1], c);
        a2 += __mul24((int)s[x * ld + 2], c);
    }
    uint8_t *o = dst + q.dst + 3 * i;
    o[0] = (uint8_t)clip8(a0);
    o[1] = (uint8_t)clip8(a1);
    o[2] = (uint8_t)clip8(a2);
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" int da_resize2d_window_rows(void) { return RS_WINDOW; }

extern "C" size_t da_resize2d_workspace_bytes(int n_pictures, const int32_t *pictures_host) {
    if (!pictures_host || n_pictures < 1) return 0;
    size_t total = 0;
    for (int g = 0; g < n_pictures; ++g) {
        const int32_t *p = pictures_host + (size_t)g * RS_PIC;
        if (p[20] < 1 || p[7] < 1) return 0;
        total += align_up((size_t)3 * (size_t)p[20] * (size_t)p[7], 16);
    }
    return total;
}

extern "C" int da_resize2d(int n_pictures, const uint8_t *src, long long src_bytes, const int32_t *pictures, const int32_t *tables,
                           long long n_table, uint8_t *dst, long long dst_bytes, uint8_t *workspace, size_t workspace_bytes, int route,
                           long long n_tiles, long long n_hblocks, long long n_vblocks, void *stream) {
    DA_REQUIRE(src && pictures && tables && dst, "da_resize2d: null argument");
    DA_REQUIRE(n_pictures > 0 && src_bytes > 0 && n_table > 0 && dst_bytes > 0,
               "da_resize2d: bad sizes (%d pictures, %lld source bytes, %lld table entries, %lld output bytes)", n_pictures, src_bytes, n_table,
               dst_bytes);
    DA_REQUIRE(route == DA_RESIZE_FUSED || route == DA_RESIZE_TWO_PASS, "da_resize2d: route is 0 (fused) or 1 (two-pass) (got %d)", route);
    hipStream_t st = (hipStream_t)stream;
    if (route == DA_RESIZE_FUSED) {
        DA_REQUIRE(n_tiles > 0 && n_tiles <= 0x7fffffffLL, "da_resize2d: %lld tiles in one launch (1 .. 2^31 - 1)", n_tiles);
        k_resize_fused<<<(unsigned)n_tiles, RS_THREADS, 0, st>>>(n_pictures, src, src_bytes, pictures, tables, n_table, dst, dst_bytes);
        DA_LAUNCH_CHECK();
        return 0;
    }
    DA_REQUIRE(workspace && workspace_bytes > 0, "da_resize2d: the two-pass route needs a workspace (da_resize2d_workspace_bytes)");
    DA_REQUIRE(n_hblocks > 0 && n_hblocks <= 0x7fffffffLL && n_vblocks > 0 && n_vblocks <= 0x7fffffffLL,
               "da_resize2d: %lld and %lld blocks in one launch (1 .. 2^31 - 1)", n_hblocks, n_vblocks);
    k_resize_h<<<(unsigned)n_hblocks, RS_THREADS, 0, st>>>(n_pictures, src, src_bytes, pictures, tables, n_table, dst_bytes, workspace,
                                                          (long long)workspace_bytes);
    DA_LAUNCH_CHECK();
    k_resize_v<<<(unsigned)n_vblocks, RS_THREADS, 0, st>>>(n_pictures, src_bytes, pictures, tables, n_table, dst, dst_bytes, workspace,
                                                          (long long)workspace_bytes);
    DA_LAUNCH_CHECK();
    return 0;
}
