// GCN backbone (backbones/gcn.py:5-22): the normalised aggregation of PyG's GCNConv with default settings,
// restated (PyG 2.1-2.3, the version pytorch==1.12.1 implies; PyG is not vendored by the reference):
//   add_remaining_self_loops -- every existing self loop dropped, one loop of weight 1 added per node;
//   deg[i] = incoming edges of i counted at the TARGET (edge_index[1]), loop included, duplicates counted;
//   out_i = sum_{j -> i} deg[j]^-1/2 deg[i]^-1/2 (x W^T)_j + b.
// The projection runs on the library's linear kernels; these kernels only aggregate (width W = 256, the GCN's hidden
// width: layer 0 projects first, layer 1 aggregates first, so both aggregations run at 256 columns), with the bias
// and the activation fused into the epilogue.  Three plan kinds:
//   dense   (complete graphs, with or without self loops): A_hat = J / n_g -- a per-graph column mean, broadcast;
//   band    (closed-form Exphander plan, duplicate-free): A_hat = (A + I) / (d + 1) -- a cyclic window sum over the
//           circulant band in slot space, no edge list;
//   csr     (anything else): gather over the CSR by destination with dinv[] from da_gcn_dinv.
#include "da_common.h"
#include "da_internal.h"

namespace da {

// dinv[i] = (1 + #{incoming edges of i that are not self loops})^-1/2   (one thread per node)
__global__ void k_gcn_dinv(int n, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_src, float *__restrict__ dinv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int cnt = 1;
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) cnt += col_src[e] != i;
    dinv[i] = 1.0f / sqrtf((float)cnt);
}

template <typename T> struct Vec4;
template <> struct Vec4<float> {
    static __device__ inline void load(const float *p, float v[4]) {
        const float4 q = *(const float4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    static __device__ inline void store(float *p, const float v[4]) { *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Vec4<bf16_t> {
    static __device__ inline void load(const bf16_t *p, float v[4]) {
        const uint2 q = *(const uint2 *)p;
        v[0] = bf2f((bf16_t)(q.x & 0xffffu)); v[1] = bf2f((bf16_t)(q.x >> 16));
        v[2] = bf2f((bf16_t)(q.y & 0xffffu)); v[3] = bf2f((bf16_t)(q.y >> 16));
    }
    static __device__ inline void store(bf16_t *p, const float v[4]) {
        uint2 q;
        q.x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
        q.y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
        *(uint2 *)p = q;
    }
};

template <typename T>
__device__ inline void gcn_epilogue(float v[4], float scale, const float *bias, int c, int act) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float y = v[k] * scale;
        if (bias) y += bias[c + k];
        v[k] = apply_act(y, act);
    }
}

// CSR gather: one wave per destination row, four columns per lane, W / 256 passes.
template <typename T>
__global__ void __launch_bounds__(256) k_gcn_agg_csr(int n, int W, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_src,
                                                      const float *__restrict__ dinv, const T *__restrict__ X, const float *__restrict__ bias,
                                                      int act, T *__restrict__ out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
    const float di = dinv[i];
    for (int c = lane * 4; c < W; c += 256) {
        float acc[4], v[4];
        Vec4<T>::load(X + (size_t)i * W + c, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = di * v[k];            // the one self loop
        for (int e = e0; e < e1; ++e) {
            const int j = col_src[e];
            if (j == i) continue;                                  // existing self loops are dropped
            const float dj = dinv[j];
            Vec4<T>::load(X + (size_t)j * W + c, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(dj, v[k], acc[k]);
        }
        gcn_epilogue<T>(acc, di, bias, c, act);
        Vec4<T>::store(out + (size_t)i * W + c, acc);
    }
}

// Complete graphs: A_hat = J / n_g.  Workgroup (graph g, 64 columns): four row groups sum the graph's rows, then the
// same workgroup writes act(mean + b) to every row of the graph.  n_g (n + 64) W element reads/writes, no n^2 term.
template <typename T>
__global__ void __launch_bounds__(256) k_gcn_agg_dense(int W, const int32_t *__restrict__ graph_ptr, const T *__restrict__ X,
                                                        const float *__restrict__ bias, int act, T *__restrict__ out) {
    __shared__ float part[4][64];
    const int g = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rg = threadIdx.x >> 6;
    const int r0 = graph_ptr[g], r1 = graph_ptr[g + 1];
    float s = 0.f;
    if (c < W)
        for (int r = r0 + rg; r < r1; r += 4) s += ldf(X + (size_t)r * W + c);
    part[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (c >= W) return;
    const float tot = (part[0][threadIdx.x & 63] + part[1][threadIdx.x & 63]) + (part[2][threadIdx.x & 63] + part[3][threadIdx.x & 63]);
    const float dn = 1.0f / sqrtf((float)(r1 - r0));
    float v = tot * (dn * dn);
    if (bias) v += bias[c];
    v = apply_act(v, act);
    for (int r = r0 + rg; r < r1; r += 4) stf(out + (size_t)r * W + c, v);
}

// Closed-form Exphander plan (graph_plan.expander_plan, banded layout): the node at slot s of graph g neighbours the
// slots s +- 1 .. s +- h (mod n), h = d / 2, and for odd d the antipodal slot s + n / 2.  With the self loop every
// node has d + 1 incoming edges, so out(s) = (sum over the window s - h .. s + h [+ antipode]) / (d + 1).
// Lane = column, wave = a run of RUN consecutive slots: the first slot's window is summed directly, the following ones
// slide it (one row in, one row out), so the work per output row is ~(2h + 1) / RUN + 3 row reads, not 2h + 1.
constexpr int GCN_BAND_RUN = 64;
template <typename T>
__global__ void __launch_bounds__(256) k_gcn_agg_band(int n, int degree, int W, const int32_t *__restrict__ pad_ptr,
                                                       const int32_t *__restrict__ slot_node, const T *__restrict__ X,
                                                       const float *__restrict__ bias, int act, T *__restrict__ out) {
    const int g = blockIdx.z;
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    const int s0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * GCN_BAND_RUN;
    if (s0 >= n || c >= W) return;
    const int32_t *sn = slot_node + pad_ptr[g];
    const int h = degree / 2;
    const bool anti = degree & 1;
    auto row = [&](int s) -> float {                 // X at slot s (cyclic) of column c
        s %= n;
        if (s < 0) s += n;
        return ldf(X + (size_t)sn[s] * W + c);
    };
    float win = 0.f;
    for (int k = -h; k <= h; ++k) win += row(s0 + k);
    const float dn = 1.0f / sqrtf((float)(degree + 1));
    const float bc = bias ? bias[c] : 0.f;
    const int s1 = min(s0 + GCN_BAND_RUN, n);
    for (int s = s0; s < s1; ++s) {
        if (s > s0) win += row(s + h) - row(s - h - 1);
        float v = win;
        if (anti) v += row(s + n / 2);
        v = apply_act(v * (dn * dn) + bc, act);
        stf(out + (size_t)sn[s] * W + c, v);
    }
}

// How a GCN layer aggregates over this plan: 0 = dense, 1 = band, 2 = csr, -1 = no path (hybrid plan without the band)
int gcn_plan_kind(const da_graph *g) {
    if (g->dense && g->graph_ptr) return 0;
    if (g->hybrid && g->band_degree > 0 && g->slot_node && g->pad_ptr && g->n_nodes == g->n_real) return 1;
    if (g->row_ptr && (g->col_src || g->n_edges == 0)) return 2;
    return -1;
}

int launch_gcn_dinv(const da_graph *g, float *dinv, hipStream_t st) {
    if (gcn_plan_kind(g) != 2) return 0;             // dense / band plans: closed form inside the aggregation kernels
    k_gcn_dinv<<<(g->n_nodes + 255) / 256, 256, 0, st>>>(g->n_nodes, g->row_ptr, g->col_src, dinv);
    DA_LAUNCH_CHECK();
    return 0;
}

// out[n_nodes, W] = act(A_hat X + bias) (bias may be NULL), X / out in the act dtype, W % 4 == 0
int launch_gcn_aggregate(int prec, const da_graph *g, int W, const float *dinv, const void *X, const float *bias, int act, void *out,
                         hipStream_t st) {
    DA_REQUIRE(W > 0 && W % 4 == 0, "gcn aggregate: width %d must be a positive multiple of 4", W);
    const int kind = gcn_plan_kind(g);
    const bool b16 = prec == DA_PREC_BF16;
    if (kind == 0) {
        const dim3 grid((W + 63) / 64, g->n_graphs);
        if (b16) k_gcn_agg_dense<bf16_t><<<grid, 256, 0, st>>>(W, g->graph_ptr, (const bf16_t *)X, bias, act, (bf16_t *)out);
        else k_gcn_agg_dense<float><<<grid, 256, 0, st>>>(W, g->graph_ptr, (const float *)X, bias, act, (float *)out);
    } else if (kind == 1) {
        const int n = g->max_graph_nodes;           // every graph of a banded plan has n nodes
        DA_REQUIRE(n > 0 && (long long)n * g->n_graphs == g->n_real, "gcn aggregate: banded plan with unequal graphs");
        DA_REQUIRE(g->band_degree < n, "gcn aggregate: band degree %d >= n = %d", g->band_degree, n);
        const dim3 grid((n + 4 * GCN_BAND_RUN - 1) / (4 * GCN_BAND_RUN), (W + 63) / 64, g->n_graphs);
        if (b16) k_gcn_agg_band<bf16_t><<<grid, 256, 0, st>>>(n, g->band_degree, W, g->pad_ptr, g->slot_node, (const bf16_t *)X, bias, act, (bf16_t *)out);
        else k_gcn_agg_band<float><<<grid, 256, 0, st>>>(n, g->band_degree, W, g->pad_ptr, g->slot_node, (const float *)X, bias, act, (float *)out);
    } else if (kind == 2) {
        DA_REQUIRE(dinv, "gcn aggregate: CSR plan without dinv");
        if (g->n_nodes == 0) return 0;
        const unsigned grid = (unsigned)((g->n_nodes + 3) / 4);
        if (b16) k_gcn_agg_csr<bf16_t><<<grid, 256, 0, st>>>(g->n_nodes, W, g->row_ptr, g->col_src, dinv, (const bf16_t *)X, bias, act, (bf16_t *)out);
        else k_gcn_agg_csr<float><<<grid, 256, 0, st>>>(g->n_nodes, W, g->row_ptr, g->col_src, dinv, (const float *)X, bias, act, (float *)out);
    } else {
        set_error("gcn aggregate: the plan is hybrid without the banded Exphander layout (plan GCN Batches with hybrid='off')");
        return 1;
    }
    DA_LAUNCH_CHECK();
    return 0;
}

// The transposed aggregation (the backward's dX = A_hat^T dY): complete graphs and the Exphander band are symmetric, so the
// forward kernels apply as they are; over a CSR plan the same gather walks the by-SOURCE CSR (out_ptr / out_dst) with the
// forward's target-side dinv: out_j = dinv_j (dinv_j y_j + sum_{j -> i, i != j} dinv_i y_i) = sum_i norm_ji y_i.
int launch_gcn_aggregate_t(int prec, const da_graph *g, int W, const float *dinv, const void *X, void *out, hipStream_t st) {
    if (gcn_plan_kind(g) != 2) return launch_gcn_aggregate(prec, g, W, dinv, X, nullptr, DA_ACT_NONE, out, st);
    DA_REQUIRE(g->out_ptr && (g->out_dst || g->n_edges == 0), "gcn backward: the CSR plan needs its by-source orientation (out_ptr / out_dst)");
    da_graph gt = *g;
    gt.row_ptr = g->out_ptr;
    gt.col_src = g->out_dst;
    return launch_gcn_aggregate(prec, &gt, W, dinv, X, nullptr, DA_ACT_NONE, out, st);
}

// out = gelu(pre) + res   (fp32; conv 1's activation and the residual feats + combined_feats of the training forward)
__global__ void __launch_bounds__(256) k_gcn_gelu_res(size_t n, const float *__restrict__ pre, const float *__restrict__ res,
                                                       float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gelu_erf(pre[i]) + res[i];
}
int launch_gcn_gelu_res(size_t n, const float *pre, const float *res, float *out, hipStream_t st) {
    if (!n) return 0;
    k_gcn_gelu_res<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, pre, res, out);
    DA_LAUNCH_CHECK();
    return 0;
}

}  // namespace da

extern "C" int da_gcn_aggregate(int prec, const da_graph *g, int W, const float *dinv, const void *X, const float *bias, int act, void *out,
                                void *stream) {
    DA_REQUIRE(g && X && out, "da_gcn_aggregate: null argument");
    DA_REQUIRE(prec == DA_PREC_F32 || prec == DA_PREC_BF16, "bad precision %d", prec);
    return da::launch_gcn_aggregate(prec, g, W, dinv, X, bias, act, out, (hipStream_t)stream);
}

extern "C" int da_gcn_dinv(const da_graph *g, float *dinv, void *stream) {
    DA_REQUIRE(g && dinv, "da_gcn_dinv: null argument");
    return da::launch_gcn_dinv(g, dinv, (hipStream_t)stream);
}
