// EfficientNet-B0 piece encoder (model="efficientnet_b0", the reference's default 2D backbone): the eval feature forward of timm's
// efficientnet_b0 under features_only=True, restricted to what Eff_GAT.visual_features keeps -- stem, blocks.0 .. blocks.4, feature
// maps 2 (blocks.2.1, 40 x 4 x 4) and 3 (blocks.4.2, 112 x 2 x 2) flattened in NCHW order into one 1088-wide row per 32 x 32 crop.
// fp32 throughout, every eval BatchNorm folded into the convolution in front of it on the host.  Activations are NHWC with the channel
// count padded to a multiple of 16 (24 -> 32, 40 -> 48; the padding channels are exact zeros: their folded weights and biases are zero),
// so that a 1x1 convolution is a row-major product with M = crops * H * W.
//
//   k_eff_stem   one workgroup per crop, one lane per output pixel: (x - mean) / std on the way in (the convolution pads the NORMALISED
//                image with zeros), the crop read through 0..3 clockwise quarter turns, 3x3 stride 2, + bias, SiLU -> [256][32].
//   k_eff_pw     the 1x1 convolutions on v_mfma_f32_16x16x4_f32 (exact fp32 operands): a wave owns 32 rows x 64 columns (2 x 4
//                accumulator blocks), reads its A rows and the weights' rows from L1 / L2 16 bytes per lane (one load feeds four k
//                steps), applies the squeeze-excite gate [crop][channel] to the A operand as it loads it, and folded bias, SiLU and the
//                residual in the epilogue.  The k order of an output is fixed by the shape alone.
//   k_eff_dw     depthwise k x k (3 / 5, stride 1 / 2) + bias + SiLU, one workgroup per crop, lanes over channels (coalesced NHWC),
//                the taps' weights in registers; the same workgroup then forms the squeeze-excite mean by a fixed-order sum (per output
//                row, then over rows), the reduce product + SiLU and the expand product + sigmoid: the gate [crop][channel] leaves it.
//   k_eff_nchw   NHWC (padded) -> NCHW: the two maps of the output row, and the block taps of da_effnet_forward_taps.
// No atomics; a crop's row does not depend on its neighbours or on the batch size (the batch is walked in chunks of EFF_CHUNK crops over
// one bounded workspace).
#include "da_internal.h"

namespace da {
namespace {

typedef __attribute__((ext_vector_type(4))) float ef_f4;

constexpr int EFF_CHUNK = 512;                       // crops per pass over the workspace
constexpr int EFF_PW_ROWS = 128;                     // rows of a k_eff_pw workgroup (4 waves x 32)
constexpr int EFF_PW_COLS = 64;                      // columns of a k_eff_pw workgroup
constexpr int EFF_CMAX = 672, EFF_RMAX = 32;         // widest depthwise map, widest squeeze (28) rounded up
constexpr int EFF_PART = 1344;                       // Ho * C at most (2 x 672)

struct EffBlock { int cin, mid, cout, k, s, r, h, skip; };   // h: spatial size of the block's input
constexpr EffBlock EFF_BLOCKS[DA_EFFNET_BLOCKS] = {
    {32, 32, 16, 3, 1, 8, 16, 0},                    // blocks.0.0: depthwise-separable (no expansion)
    {16, 96, 24, 3, 2, 4, 16, 0},   {24, 144, 24, 3, 1, 6, 8, 1},
    {24, 144, 40, 5, 2, 6, 8, 0},   {40, 240, 40, 5, 1, 10, 4, 1},      // blocks.2.1 = map 2
    {40, 240, 80, 3, 2, 10, 4, 0},  {80, 480, 80, 3, 1, 20, 2, 1},   {80, 480, 80, 3, 1, 20, 2, 1},
    {80, 480, 112, 5, 1, 20, 2, 0}, {112, 672, 112, 5, 1, 28, 2, 1}, {112, 672, 112, 5, 1, 28, 2, 1},   // blocks.4.2 = map 3
};
constexpr int EFF_MAP2 = 4, EFF_MAP3 = 10, EFF_MAP2_LEN = 40 * 16;
constexpr int p16(int c) { return (c + 15) / 16 * 16; }

__device__ __forceinline__ float eff_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float eff_silu(float x) { return x / (1.f + __expf(-x)); }

// ---- stem -------------------------------------------------------------------------------------------------------------------
// pixel (i, j) of the crop turned by `turns` clockwise quarter turns = pixel (si, sj) of the crop (torch.rot90(x, -turns, (2, 3)))
__device__ __forceinline__ void eff_turn(int turns, int i, int j, int &si, int &sj) {
    si = turns == 0 ? i : turns == 1 ? 31 - j : turns == 2 ? 31 - i : j;
    sj = turns == 0 ? j : turns == 1 ? i : turns == 2 ? 31 - j : 31 - i;
}

// W [32][27] (c * 9 + ky * 3 + kx), Y [n][16 * 16][32]
__global__ __launch_bounds__(256) void k_eff_stem(int turns, const float *__restrict__ crops, const float *__restrict__ W,
                                                  const float *__restrict__ B, float *__restrict__ Y) {
    const float mean[3] = {0.4850f, 0.4560f, 0.4060f}, sd[3] = {0.2290f, 0.2240f, 0.2250f};
    const int tid = threadIdx.x, oh = tid >> 4, ow = tid & 15;
    const float *crop = crops + (size_t)blockIdx.x * 3 * 1024;
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ih = 2 * oh - 1 + ky, iw = 2 * ow - 1 + kx;
                float v = 0.f;                         // the convolution pads the NORMALISED image with zeros
                if (ih >= 0 && ih < 32 && iw >= 0 && iw < 32) {
                    int si, sj;
                    eff_turn(turns, ih, iw, si, sj);
                    v = (crop[c * 1024 + si * 32 + sj] - mean[c]) / sd[c];
                }
                in[c * 9 + ky * 3 + kx] = v;
            }
    float *y = Y + ((size_t)blockIdx.x * 256 + tid) * 32;
#pragma unroll 1
    for (int o4 = 0; o4 < 32; o4 += 4) {
        ef_f4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *w = W + (o4 + e) * 27;        // uniform over the wave
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < 27; ++t) acc = fmaf(in[t], w[t], acc);
            r[e] = eff_silu(acc + B[o4 + e]);
        }
        *(ef_f4 *)(y + o4) = r;
    }
}

// ---- 1x1 convolution ----------------------------------------------------------------------------------------------------------
// Y[m][c] = act(sum_k A[m][k] (* gate[m >> hw_shift][k]) W[c][k] + B[c]) (+ res[m][c]); K and Cout multiples of 16, A / gate row
// stride K, Y / res row stride Cout.  Lane (r = lane & 15, q = lane >> 4) holds A[row r][s + 4 q + e] and W[col r][s + 4 q + e],
// e = 0..3, of a 16-wide k slice: MFMA e of the slice sums the four k = s + 4 q + e, so the slice's k are covered once each.
template <int ACT, bool GATE, bool RES>
__global__ __launch_bounds__(256) void k_eff_pw(long long M, int K, int Cout, int hw_shift, const float *__restrict__ A,
                                                const float *__restrict__ gate, const float *__restrict__ W, const float *__restrict__ B,
                                                const float *__restrict__ res, float *__restrict__ Y) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * 32;
    if (row0 >= M) return;                             // wave-uniform; the kernel has no barrier
    const int c0 = blockIdx.y * EFF_PW_COLS;
    const int nb = (Cout - c0) >> 4 < 4 ? (Cout - c0) >> 4 : 4;      // column blocks of this workgroup that exist
    const float *a[2], *g[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        long long row = row0 + 16 * b + r;
        row = row < M ? row : M - 1;                   // tail rows read the last row; their results are not stored
        a[b] = A + (size_t)row * K + 4 * q;
        g[b] = GATE ? gate + (size_t)(row >> hw_shift) * K + 4 * q : nullptr;
    }
    const float *wl = W + (size_t)(c0 + r) * K + 4 * q;
    ef_f4 acc[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[b][j] = (ef_f4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < K; s += 16) {
        ef_f4 x[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            x[b] = *(const ef_f4 *)(a[b] + s);
            if (GATE) x[b] *= *(const ef_f4 *)(g[b] + s);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nb) {
                const ef_f4 wv = *(const ef_f4 *)(wl + (size_t)j * 16 * K + s);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[b][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[b][e], wv[e], acc[b][j], 0, 0, 0);
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nb) {
            const int col = c0 + 16 * j + r;
            const float bias = B[col];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const long long row = row0 + 16 * b + 4 * q + v;
                    if (row < M) {
                        float y = acc[b][j][v] + bias;
                        if (ACT) y = eff_silu(y);
                        if (RES) y += res[(size_t)row * Cout + col];
                        Y[(size_t)row * Cout + col] = y;
                    }
                }
        }
}

// ---- depthwise convolution + squeeze-excite gate ------------------------------------------------------------------------------
// X [n][H * H][C] -> Y [n][Ho * Ho][C], Ho = H / S, padding KS / 2; Wd [KS * KS][C], Wr / We [R][C]; gate [n][C]
template <int KS, int S>
__global__ __launch_bounds__(256) void k_eff_dw(int H, int C, int R, const float *__restrict__ X, const float *__restrict__ Wd,
                                                const float *__restrict__ Bd, const float *__restrict__ Wr, const float *__restrict__ Br,
                                                const float *__restrict__ We, const float *__restrict__ Be, float *__restrict__ Y,
                                                float *__restrict__ gate) {
    constexpr int P = KS / 2;
    __shared__ float part[EFF_PART], smean[EFF_CMAX], sr[EFF_RMAX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, Ho = H / S;
    const float *x = X + (size_t)blockIdx.x * H * H * C;
    float *y = Y + (size_t)blockIdx.x * Ho * Ho * C;
    for (int i = tid; i < Ho * C; i += 256) {
        const int oh = i / C, c = i - oh * C;
        float wt[KS * KS];
#pragma unroll
        for (int t = 0; t < KS * KS; ++t) wt[t] = Wd[t * C + c];
        const float bias = Bd[c];
        float sum = 0.f;
        for (int ow = 0; ow < Ho; ++ow) {
            float acc = 0.f;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                const int ih = oh * S - P + ky;
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const int iw = ow * S - P + kx;
                    if (ih >= 0 && ih < H && iw >= 0 && iw < H) acc = fmaf(x[(size_t)(ih * H + iw) * C + c], wt[ky * KS + kx], acc);
                }
            }
            const float v = eff_silu(acc + bias);
            y[(size_t)(oh * Ho + ow) * C + c] = v;
            sum += v;
        }
        part[i] = sum;
    }
    __syncthreads();
    const float inv = 1.f / (float)(Ho * Ho);
    for (int c = tid; c < C; c += 256) {
        float s = 0.f;
        for (int oh = 0; oh < Ho; ++oh) s += part[oh * C + c];
        smean[c] = s * inv;
    }
    __syncthreads();
    for (int j = w; j < R; j += 4) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc = fmaf(Wr[(size_t)j * C + c], smean[c], acc);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) sr[j] = eff_silu(acc + Br[j]);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float acc = Be[c];
        for (int j = 0; j < R; ++j) acc = fmaf(We[(size_t)j * C + c], sr[j], acc);
        gate[(size_t)blockIdx.x * C + c] = eff_sigmoid(acc);
    }
}

// ---- NHWC (CP channels per pixel) -> NCHW (C channels): dst[n * dst_stride + c * HW + p] ------------------------------------------
__global__ __launch_bounds__(256) void k_eff_nchw(long long total, int HW, int CP, int C, const float *__restrict__ src,
                                                  float *__restrict__ dst, long long dst_stride) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int per = C * HW;
    const long long n = i / per;
    const int rem = (int)(i - n * per), c = rem / HW, p = rem - c * HW;
    dst[n * dst_stride + rem] = src[((size_t)n * HW + p) * CP + c];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct EffWork {
    float *x0, *x1, *e, *d, *g;
    size_t bytes;
};
EffWork eff_work(void *base, long long n) {
    EffWork w;
    char *b = (char *)base;
    size_t o = 0;
    w.x0 = (float *)(b + o); o += align_up((size_t)n * 256 * 32 * sizeof(float), 256);        // stem output; every second block's output
    w.x1 = (float *)(b + o); o += align_up((size_t)n * 256 * 16 * sizeof(float), 256);        // the other blocks' outputs (blocks.0.0 the largest)
    w.e = (float *)(b + o); o += align_up((size_t)n * 256 * 96 * sizeof(float), 256);         // expansion (blocks.1.0 the largest)
    w.d = (float *)(b + o); o += align_up((size_t)n * 64 * 144 * sizeof(float), 256);         // depthwise output (blocks.1.1 the largest)
    w.g = (float *)(b + o); o += align_up((size_t)n * EFF_CMAX * sizeof(float), 256);         // squeeze-excite gates
    w.bytes = o;
    return w;
}

bool eff_aligned16(const void *p) { return ((size_t)p & 15) == 0; }
int eff_log2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

template <int ACT, bool GATE, bool RES>
void eff_pw(long long M, int K, int Cout, int hw, const float *A, const float *gate, const float *W, const float *B, const float *res, float *Y,
            hipStream_t st) {
    const dim3 grid((unsigned)((M + EFF_PW_ROWS - 1) / EFF_PW_ROWS), (unsigned)((Cout + EFF_PW_COLS - 1) / EFF_PW_COLS));
    k_eff_pw<ACT, GATE, RES><<<grid, 256, 0, st>>>(M, K, Cout, eff_log2(hw), A, gate, W, B, res, Y);
}

void eff_nchw(int n, int HW, int C, const float *src, float *dst, long long dst_stride, hipStream_t st) {
    const long long total = (long long)n * C * HW;
    k_eff_nchw<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(total, HW, p16(C), C, src, dst, dst_stride);
}

enum { EFF_ST_STEM = 1, EFF_ST_BLOCK0 = 2, EFF_ST_OUT = 1 << 12, EFF_ST_ALL = (1 << 13) - 1 };

int eff_run(const da_effnet_weights *w, int n, const float *crops, int turns, float *out, int ld_out, void *workspace, float *const *taps,
            int stages, hipStream_t st) {
    const EffWork k = eff_work(workspace, n < EFF_CHUNK ? n : EFF_CHUNK);
    for (int n0 = 0; n0 < n; n0 += EFF_CHUNK) {
        const int nc = n - n0 < EFF_CHUNK ? n - n0 : EFF_CHUNK;
        if (stages & EFF_ST_STEM) k_eff_stem<<<(unsigned)nc, 256, 0, st>>>(turns, crops + (size_t)n0 * 3 * 1024, w->stem_w, w->stem_b, k.x0);
        float *cur = k.x0, *nxt = k.x1;
        for (int b = 0; b < DA_EFFNET_BLOCKS; ++b) {
            const EffBlock &B = EFF_BLOCKS[b];
            const int ho = B.h / B.s, cin = p16(B.cin), mid = p16(B.mid), cout = p16(B.cout);
            if (stages & (EFF_ST_BLOCK0 << b)) {
                const float *dwin = cur;
                if (b > 0) {
                    eff_pw<1, false, false>((long long)nc * B.h * B.h, cin, mid, 1, cur, nullptr, w->exp_w[b], w->exp_b[b], nullptr, k.e, st);
                    dwin = k.e;
                }
#define EFF_DW(KS, S) k_eff_dw<KS, S><<<(unsigned)nc, 256, 0, st>>>(B.h, mid, B.r, dwin, w->dw_w[b], w->dw_b[b], w->se_rw[b], w->se_rb[b], \
                                                                  w->se_ew[b], w->se_eb[b], k.d, k.g)
                if (B.k == 3 && B.s == 1) EFF_DW(3, 1);
                else if (B.k == 3) EFF_DW(3, 2);
                else if (B.s == 1) EFF_DW(5, 1);
                else EFF_DW(5, 2);
#undef EFF_DW
                const long long M = (long long)nc * ho * ho;
                if (B.skip) eff_pw<0, true, true>(M, mid, cout, ho * ho, k.d, k.g, w->prj_w[b], w->prj_b[b], cur, nxt, st);
                else eff_pw<0, true, false>(M, mid, cout, ho * ho, k.d, k.g, w->prj_w[b], w->prj_b[b], nullptr, nxt, st);
            }
            float *t = cur; cur = nxt; nxt = t;
            if (taps && (stages & (EFF_ST_BLOCK0 << b)))
                eff_nchw(nc, ho * ho, B.cout, cur, taps[b] + (size_t)n0 * B.cout * ho * ho, (long long)B.cout * ho * ho, st);
            if ((stages & EFF_ST_OUT) && b == EFF_MAP2) eff_nchw(nc, ho * ho, B.cout, cur, out + (size_t)n0 * ld_out, ld_out, st);
            if ((stages & EFF_ST_OUT) && b == EFF_MAP3) eff_nchw(nc, ho * ho, B.cout, cur, out + (size_t)n0 * ld_out + EFF_MAP2_LEN, ld_out, st);
        }
    }
    DA_LAUNCH_CHECK();
    return 0;
}

int eff_args_ok(const da_effnet_weights *w, int n, const float *crops, int turns, float *out, int ld_out, void *workspace, size_t workspace_bytes,
                const char *who) {
    DA_REQUIRE(w, "%s: null weights", who);
    DA_REQUIRE(n >= 0, "%s: n_crops %d (need >= 0)", who, n);
    DA_REQUIRE(turns >= 0 && turns <= 3, "%s: quarter_turns %d (need 0 .. 3)", who, turns);
    if (n == 0) return 0;
    DA_REQUIRE(crops && out && ld_out >= DA_EFFNET_OUT, "%s: null crops / out, or ld_out %d < %d", who, ld_out, DA_EFFNET_OUT);
    DA_REQUIRE(w->stem_w && w->stem_b, "%s: null stem weights", who);
    for (int b = 0; b < DA_EFFNET_BLOCKS; ++b) {
        DA_REQUIRE(b == 0 || (w->exp_w[b] && w->exp_b[b] && eff_aligned16(w->exp_w[b])), "%s: block %d: null or misaligned expansion weights", who, b);
        DA_REQUIRE(w->dw_w[b] && w->dw_b[b] && w->se_rw[b] && w->se_rb[b] && w->se_ew[b] && w->se_eb[b], "%s: block %d: null depthwise / gate weights",
                   who, b);
        DA_REQUIRE(w->prj_w[b] && w->prj_b[b] && eff_aligned16(w->prj_w[b]), "%s: block %d: null or misaligned projection weights", who, b);
    }
    const size_t need = eff_work(nullptr, n < EFF_CHUNK ? n : EFF_CHUNK).bytes;
    DA_REQUIRE(workspace && eff_aligned16(workspace) && workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu (16-byte aligned)", who,
               workspace_bytes, need);
    return 0;
}

}  // namespace
}  // namespace da

using namespace da;

extern "C" {

int da_effnet_constant(int which) {
    return which == DA_EFFNET_CHUNK ? EFF_CHUNK : which == DA_EFFNET_PW_ROWS ? EFF_PW_ROWS : which == DA_EFFNET_PW_COLS ? EFF_PW_COLS : -1;
}

size_t da_effnet_workspace_bytes(int n_crops) {
    if (n_crops <= 0) return 0;
    return eff_work(nullptr, n_crops < EFF_CHUNK ? n_crops : EFF_CHUNK).bytes;
}

int da_effnet_forward(const da_effnet_weights *w, int n_crops, const float *crops, int quarter_turns, float *out, int ld_out, void *workspace,
                      size_t workspace_bytes, void *stream) {
    if (int rc = eff_args_ok(w, n_crops, crops, quarter_turns, out, ld_out, workspace, workspace_bytes, "da_effnet_forward")) return rc;
    if (n_crops == 0) return 0;
    return eff_run(w, n_crops, crops, quarter_turns, out, ld_out, workspace, nullptr, EFF_ST_ALL, (hipStream_t)stream);
}

int da_effnet_forward_taps(const da_effnet_weights *w, int n_crops, const float *crops, int quarter_turns, float *out, int ld_out,
                           void *workspace, size_t workspace_bytes, float *const *taps, int stages, void *stream) {
    if (int rc = eff_args_ok(w, n_crops, crops, quarter_turns, out, ld_out, workspace, workspace_bytes, "da_effnet_forward_taps")) return rc;
    if (n_crops == 0) return 0;
    if (taps)
        for (int b = 0; b < DA_EFFNET_BLOCKS; ++b) DA_REQUIRE(taps[b], "da_effnet_forward_taps: null tap %d", b);
    return eff_run(w, n_crops, crops, quarter_turns, out, ld_out, workspace, taps, stages & EFF_ST_ALL, (hipStream_t)stream);
}

}  // extern "C"
