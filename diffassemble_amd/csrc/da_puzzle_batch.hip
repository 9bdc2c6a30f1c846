// A 2D Batch from whole images: every per-piece tensor the reference's dataset/puzzle_dataset.py builds on the
// host -- divide_images_into_patches :175-190 and the get() of Puzzle_Dataset :257-300, Puzzle_Dataset_Pad :326-379,
// Puzzle_Dataset_ROT_MP :403-485, Puzzle_Dataset_MP :507-544 and Puzzle_Dataset_ROT :580-700 (one Image.fromarray, one .rotate and
// one np.array per piece) -- in one launch, and the complete graphs' edge_index in a second.  The work is a byte shuffle: a quarter
// turn is a transpose, a colour is table[v] with the 256 values of uint8 / 255 made by torch on the host, so the result is
// bit-equal to the reference's.  Every random draw (turns, kept cells) is made on the host and arrives in the piece table.
//
// k_puzzle_batch: one workgroup of 256 threads per OUTPUT piece.
//   load   threads 0 .. 191 take the 32 rows x 96 bytes of the source cell with one 16-byte load each (96 = 6 x 16; the row
//          starts at base + (32 i + y) * 96 cols + 96 j, 16-byte aligned as the image base is), look the 16 bytes up in the LDS
//          copy of the table and write 16 floats into the LDS tile F[y][3 x + c], row stride 97 floats.
//   views  view k is the tile turned by t = (r + k) % 4 quarter turns counter-clockwise (np.rot90(tile, t), which is what
//          PIL.Image.rotate(90 t) does to a square tile).  The 12 KB of a view are contiguous; thread i of every pass writes
//          out[c][y][4 q .. 4 q + 3] (i = 256 c + 8 y + q) with one 16-byte store after four LDS reads:
//              t = 0  F[y][3 (4q+e) + c]      t = 1  F[4q+e][3 (31-y) + c]      t = 2  F[31-y][3 (31-4q-e) + c]      t = 3  F[31-4q-e][3 y + c]
//          and zeroes what lies in the `padding`-pixel border.
//   small  thread 0 writes the piece's row of x, rot, rot_index, indexes and batch.
// Bank conflicts (cdna_hip_programming.md 2: ds_read_b32 / ds_write_b32 are served per 32-lane half, bank = dword address % 32).
// A half covers 4 values of y and the 8 values of q.  With the row stride 97 = 1 (mod 32):
//   t = 0, 2   bank = +-(y + 12 q) + const: 12 q mod 32 = {0, 12, 24, 4, 16, 28, 8, 20}, all multiples of 4, y fills the gaps:
//              32 distinct banks, 0 conflicts;
//   t = 1, 3   the column-wise reads: bank = +-(4 q - 3 y) + const; 4 q + 3 b with b = 0 .. 3 takes 32 distinct values mod 32
//              (28 + 3 b wraps to {28, 31, 2, 5}, none of which another (q, b) reaches): 0 conflicts.  (With the natural stride
//              96 = 0 (mod 32) the eight q of a half would share one bank: 8-way.)
//   the fill   thread (y, s) writes F[y][16 s + e]: bank = y + 16 s + e, so the segments s = 0, 2, 4 (and 1, 3, 5) of one row
//              meet: 3-way, 2 extra cycles on each of the 16 writes of the three loading waves, 96 extra LDS cycles per piece
//              against the 768 .. 3072 16-byte stores that follow; the table reads before them depend on the pixels.
// tests/test_puzzle_batch_host.py reproduces the read-side counts by enumerating the addresses of every half for every (t, e, c).
// No atomics, nothing crosses workgroups, the bytes are the same on every run.
//
// k_complete_edges: one thread per edge of the block-diagonal complete graph with self loops, in the order of
// dense_to_sparse(torch.ones(n, n)) per puzzle: source-major.  The puzzle of an edge is found by bisection of the edge offsets.
#include "da_common.h"

namespace da {
namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_PATCH = 32;
constexpr int PB_ROW = 3 * PB_PATCH;               // 96: bytes of one tile row in the image, floats of one row of F
constexpr int PB_LD = PB_ROW + 1;                  // 97: the padded row stride of F (see the header)
constexpr int PB_VIEW = 3 * PB_PATCH * PB_PATCH;   // floats of one view
constexpr int PB_PUZ = 8;                          // ints per puzzle: byte offset lo, hi, rows, cols, first output piece, pieces present,
                                                   // start of the x table (linspace(-1, 1, cols)) and of the y table (rows) in `lin`
constexpr int PB_PIECE = 4;                        // ints per output piece: puzzle, source cell i * cols + j, quarter turns r, 0

__global__ __launch_bounds__(PB_THREADS) void k_puzzle_batch(int n_puzzles, int n_pieces, const uint8_t *__restrict__ images,
                                                              long long image_bytes, const int32_t *__restrict__ puzzles,
                                                              const int32_t *__restrict__ pieces, const float *__restrict__ lin, int n_lin,
                                                              const float *__restrict__ unit, int padding, int views, int x_cols,
                                                              float *__restrict__ patches, float *__restrict__ x, long long *__restrict__ rot,
                                                              long long *__restrict__ rot_index, long long *__restrict__ indexes,
                                                              long long *__restrict__ batch) {
    __shared__ float F[PB_PATCH * PB_LD];
    __shared__ float table[256];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int4 pc = *(const int4 *)(pieces + (size_t)p * PB_PIECE);
    const int g = pc.x, cell = pc.y, r = pc.z;
    // uniform per workgroup, before the first barrier: tables that point outside the buffers write nothing
    if (g < 0 || g >= n_puzzles || r < 0 || r > 3) return;
    const int32_t *pz = puzzles + (size_t)g * PB_PUZ;
    const long long off = (long long)(((unsigned long long)(unsigned)pz[1] << 32) | (unsigned)pz[0]);
    const int rows = pz[2], cols = pz[3], first = pz[4], present = pz[5], lx = pz[6], ly = pz[7];
    if (rows < 1 || cols < 1 || rows > 32768 / cols || cell < 0 || cell >= rows * cols) return;
    if (off < 0 || (off & 15) || off + (long long)rows * cols * (PB_ROW * PB_PATCH) > image_bytes) return;
    if (first < 0 || present < 1 || p < first || p >= first + present || lx < 0 || ly < 0 || lx + cols > n_lin || ly + rows > n_lin) return;
    const int ci = cell / cols, cj = cell % cols;

    table[tid] = unit[tid];
    __syncthreads();
    if (tid < PB_PATCH * 6) {
        const int y = tid / 6, s = tid % 6;
        const uint4 v = *(const uint4 *)(images + off + ((long long)(PB_PATCH * ci + y) * cols + cj) * PB_ROW + 16 * s);
        float *dst = F + y * PB_LD + 16 * s;
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int b = 0; b < 4; ++b) dst[4 * k + b] = table[(w[k] >> (8 * b)) & 255u];
        }
    }
    __syncthreads();

    const int q4 = (tid & 7) * 4, y = tid >> 3;
    const bool row_in = y >= padding && y < PB_PATCH - padding;
    float *out = patches + (size_t)p * views * PB_VIEW + (size_t)y * PB_PATCH + q4;
    for (int k = 0; k < views; ++k) {
        const int t = (r + k) & 3;
        // F index of out[c][y][q4 + e] = base + e * step + c
        int base, step;
        if (t == 0) { base = y * PB_LD + 3 * q4; step = 3; }
        else if (t == 1) { base = q4 * PB_LD + 3 * (PB_PATCH - 1 - y); step = PB_LD; }
        else if (t == 2) { base = (PB_PATCH - 1 - y) * PB_LD + 3 * (PB_PATCH - 1 - q4); step = -3; }
        else { base = (PB_PATCH - 1 - q4) * PB_LD + 3 * y; step = -PB_LD; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 v;
            v.x = F[base + c];
            v.y = F[base + step + c];
            v.z = F[base + 2 * step + c];
            v.w = F[base + 3 * step + c];
            if (!row_in) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q4 + 0 < padding || q4 + 0 >= PB_PATCH - padding) v.x = 0.f;
            if (q4 + 1 < padding || q4 + 1 >= PB_PATCH - padding) v.y = 0.f;
            if (q4 + 2 < padding || q4 + 2 >= PB_PATCH - padding) v.z = 0.f;
            if (q4 + 3 < padding || q4 + 3 >= PB_PATCH - padding) v.w = 0.f;
            *(float4 *)(out + (size_t)k * PB_VIEW + c * (PB_PATCH * PB_PATCH)) = v;
        }
    }
    if (tid == 0) {
        const int cs[4] = {1, 0, -1, 0}, sn[4] = {0, 1, 0, -1};      // one_hot(r) @ [[1, 0], [0, 1], [-1, 0], [0, -1]]
        float *xr = x + (size_t)p * x_cols;
        xr[0] = lin[lx + cj];
        xr[1] = lin[ly + ci];
        if (x_cols == 4) {
            xr[2] = (float)cs[r];
            xr[3] = (float)sn[r];
        }
        rot[2 * (size_t)p] = cs[r];
        rot[2 * (size_t)p + 1] = sn[r];
        rot_index[p] = r;
        indexes[p] = cell;
        batch[p] = g;
    }
}

constexpr int CE_THREADS = 256;

// table [n_puzzles][3] int64: first edge, first piece, pieces present
__global__ __launch_bounds__(CE_THREADS) void k_complete_edges(int n_puzzles, const long long *__restrict__ table, long long n_edges,
                                                                long long *__restrict__ edge_index) {
    const long long e = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    int lo = 0, hi = n_puzzles - 1;                 // the last puzzle whose first edge is <= e
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[3 * (size_t)mid] <= e) lo = mid; else hi = mid - 1;
    }
    const long long e0 = table[3 * (size_t)lo], first = table[3 * (size_t)lo + 1], n = table[3 * (size_t)lo + 2];
    const long long k = e - e0;
    if (n < 1 || k < 0 || k >= n * n) return;       // a table that does not tile [0, n_edges): nothing is written
    edge_index[e] = first + k / n;
    edge_index[n_edges + e] = first + k % n;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" int da_puzzle_batch(int n_puzzles, int n_pieces, const uint8_t *images, long long image_bytes, const int32_t *puzzles,
                               const int32_t *pieces, const float *lin, int n_lin, const float *unit, int padding, int views, int x_cols,
                               float *patches, float *x, long long *rot, long long *rot_index, long long *indexes, long long *batch,
                               void *stream) {
    DA_REQUIRE(images && puzzles && pieces && lin && unit && patches && x && rot && rot_index && indexes && batch,
               "da_puzzle_batch: null argument");
    DA_REQUIRE(n_puzzles > 0 && n_pieces > 0 && image_bytes > 0 && n_lin > 0,
               "da_puzzle_batch: bad sizes (%d puzzles, %d pieces, %lld image bytes, %d table entries)", n_puzzles, n_pieces, image_bytes, n_lin);
    DA_REQUIRE(views == 1 || views == 4, "da_puzzle_batch: views is 1 or 4 (got %d)", views);
    DA_REQUIRE(x_cols == 2 || x_cols == 4, "da_puzzle_batch: x has 2 or 4 columns (got %d)", x_cols);
    DA_REQUIRE(padding >= 0 && padding <= PB_PATCH / 2, "da_puzzle_batch: padding is 0 .. 16 (got %d)", padding);
    DA_REQUIRE(((uintptr_t)images & 15) == 0 && ((uintptr_t)patches & 15) == 0 && ((uintptr_t)pieces & 15) == 0,
               "da_puzzle_batch: images, patches and the piece table are 16-byte aligned");
    DA_REQUIRE((long long)n_pieces * PB_THREADS <= 0xffffffffLL, "da_puzzle_batch: %d pieces in one launch (at most 2^24 - 1)", n_pieces);
    k_puzzle_batch<<<(unsigned)n_pieces, PB_THREADS, 0, (hipStream_t)stream>>>(n_puzzles, n_pieces, images, image_bytes, puzzles, pieces, lin,
                                                                               n_lin, unit, padding, views, x_cols, patches, x, rot,
                                                                               rot_index, indexes, batch);
    DA_LAUNCH_CHECK();
    return 0;
}

extern "C" int da_complete_edges(int n_puzzles, const long long *table, long long n_edges, long long *edge_index, void *stream) {
    DA_REQUIRE(table && edge_index, "da_complete_edges: null argument");
    DA_REQUIRE(n_puzzles > 0 && n_edges > 0, "da_complete_edges: bad sizes (%d puzzles, %lld edges)", n_puzzles, n_edges);
    const long long blocks = (n_edges + CE_THREADS - 1) / CE_THREADS;
    DA_REQUIRE(blocks * CE_THREADS <= 0xffffffffLL, "da_complete_edges: %lld edges in one launch (fewer than 2^32)", n_edges);
    k_complete_edges<<<(unsigned)blocks, CE_THREADS, 0, (hipStream_t)stream>>>(n_puzzles, table, n_edges, edge_index);
    DA_LAUNCH_CHECK();
    return 0;
}
