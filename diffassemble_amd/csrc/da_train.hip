// Training path of the denoiser: forward with saved activations + backward of every live parameter.
//
// Replaces torch autograd through Eff_GAT.forward_with_feats (efficient_gat.py:121-146) and the PyG
// TransformerConv message/aggregate of Transformer_GNN.py:29-46 / exophormer_gnn.py:161-215, for the 2D, 3D, discrete and discrete
// rot models over the transformer, exophormer and GCN backbones.
//
// Storage is fp32; da_train_*_ex's mma_precision picks the matrix cores' operands: DA_TRAIN_MMA_FP32, the parity mode (the gradient
// fixtures of the reference are fp32), or DA_TRAIN_MMA_BF16, operands rounded to bf16 inside the kernels -- on small complete
// graphs with the projection buffers themselves stored as bf16 (Dims::q16).  Every sum runs in a fixed order (data-parallel replicas
// must produce identical bits) with ONE exception: k_time_scatter adds the rows of time_emb's gradient with atomicAdd.
//
// This file: the entry points, the shapes and the workspace (dims_of, carve_train), the step's weight images (weight_prep) and the two
// paths as stages over a TrainCtx.  The products live in da_train_gemm.hip, the attention in da_train_dense.hip (matrix cores) and
// da_train_attn.hip (edge list); da_train.h is what the four share.
#include <mutex>
#include <vector>

#include "da_train.h"

namespace da {

// ---------------------------------------------------------------------------------------------
// Small pieces around the embedding
// a[r][o] = b0[o] + sum_k W0[o][k] x[r][k]  (pos_mlp.0 pre-activation), p1 = gelu(a)
__global__ __launch_bounds__(256) void k_pos_hidden(int n, int c_in, const float *__restrict__ x, const float *__restrict__ w0,
                                                    const float *__restrict__ b0, float *__restrict__ a, float *__restrict__ p1) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * 16) return;
    const int r = idx >> 4, o = idx & 15;
    float v = b0[o];
    for (int k = 0; k < c_in; ++k) v += w0[o * c_in + k] * x[(size_t)r * c_in + k];
    a[idx] = v;
    p1[idx] = gelu_erf(v);
}

// time_emb.grad[t[r]][c] += dcomb[r][F + 32 + c]
__global__ __launch_bounds__(256) void k_time_scatter(int n, int D, int F, int steps, const int64_t *__restrict__ t,
                                                      const float *__restrict__ dcomb, float *grad) {
    // a thread takes one channel of 16 consecutive rows and adds them up while the timestep stays the same (the nodes of a
    // puzzle share theirs): one atomic per run instead of one per row -- 144 rows hammering one address took 21 us
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, chunk = idx >> 5, c = idx & 31;
    const int r0 = chunk * 16, r1 = min(n, r0 + 16);
    if (r0 >= n) return;
    int64_t cur = -1;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) {
        int64_t ti = t[r];
        ti = ti < 0 ? 0 : (ti >= steps ? steps - 1 : ti);
        if (ti != cur) {
            if (cur >= 0) atomicAdd(grad + cur * 32 + c, s);
            cur = ti;
            s = 0.f;
        }
        s += dcomb[(size_t)r * D + F + 32 + c];
    }
    if (cur >= 0) atomicAdd(grad + cur * 32 + c, s);
}

__global__ __launch_bounds__(256) void k_copy_cols(int n, int cols, const float *__restrict__ src, int lds, float *__restrict__ dst) {
    const size_t total = (size_t)n * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / cols, c = i - r * cols;
        dst[i] = src[r * lds + c];
    }
}

// virt_node_embedding.grad[v][c] += sum_g dh[(g * V + v)][c]   (rows appended as arange(V).repeat(G))
__global__ __launch_bounds__(256) void k_virt_grad(int rows, int V, int D, const float *__restrict__ dh, float *grad) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= V * D) return;
    const int v = idx / D, c = idx - v * D;
    float s = 0.f;
    for (int r = v; r < rows; r += V) s += dh[(size_t)r * D + c];
    grad[idx] += s;
}

// Every weight image the step needs beside the fp32 parameters, in ONE launch at the top of the forward (round 5; they were 13
// cast and transpose launches spread over the forward and the backward, ~5 us of dependent-launch time
// each): job j of the table = one matrix, mode 0: dst[c][r] = src[r][c] (fp32 W^T for a dX product), 1: the same rounded to bf16
// (q16 mode), 2: dst[r][c] = bf16(src[r][c]) (the bf16 forward operand of the q16 mode).  grid = (tiles of the largest job, jobs).
struct WPrepJob { const float *src; void *dst; int rows, cols, mode, pad; };
struct WPrepTable { WPrepJob job[6 + 2 * DA_MAX_LAYERS]; int n; };
__global__ __launch_bounds__(256) void k_weight_prep(WPrepTable tab) {
    __shared__ float tile[32][33];
    const WPrepJob jb = tab.job[blockIdx.y];
    const int tcols = (jb.cols + 31) / 32, trows = (jb.rows + 31) / 32;
    if ((int)blockIdx.x >= tcols * trows) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    const int r0 = ((int)blockIdx.x / tcols) * 32, c0 = ((int)blockIdx.x % tcols) * 32;
    if (jb.mode == 2) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + ty + 8 * k, c = c0 + tx;
            if (r < jb.rows && c < jb.cols) ((bf16_t *)jb.dst)[(size_t)r * jb.cols + c] = f2bf(jb.src[(size_t)r * jb.cols + c]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        if (r < jb.rows && c < jb.cols) tile[ty + 8 * k][tx] = jb.src[(size_t)r * jb.cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (r < jb.rows && c < jb.cols) {
            if (jb.mode == 1) ((bf16_t *)jb.dst)[(size_t)c * jb.rows + r] = f2bf(tile[tx][ty + 8 * k]);
            else ((float *)jb.dst)[(size_t)c * jb.rows + r] = tile[tx][ty + 8 * k];
        }
    }
}

// ---------------------------------------------------------------------------------------------
static bool train_dense_disabled() { return cfg().train_attn == 0; }          // da_config.train_attn (DA_TRAIN_ATTN=0): the edge-list kernels only

static int dims_of(const da_weights *w, const da_graph *g, Dims &d, int mma = DA_TRAIN_MMA_FP32) {
    d.bfc = mma == DA_TRAIN_MMA_BF16;
    DA_REQUIRE(w && g, "training: null argument");
    DA_REQUIRE(w->variant == DA_VARIANT_2D || w->variant == DA_VARIANT_3D || w->variant == DA_VARIANT_DISCRETE || w->variant == DA_VARIANT_DISCRETE_ROT,
               "training: unknown variant %d", w->variant);
    d.v3d = w->variant == DA_VARIANT_3D;
    d.rot = w->variant == DA_VARIANT_DISCRETE_ROT;
    d.disc = w->variant == DA_VARIANT_DISCRETE || d.rot;
    if (d.disc) {
        DA_REQUIRE(w->arch == DA_ARCH_TRANSFORMER, "training (discrete variant): the transformer architecture only, as in inference");
        DA_REQUIRE(w->c_out >= 2 && w->c_out <= 1024, "training (discrete variant): K = c_out = %d outside [2, 1024]", w->c_out);
        DA_REQUIRE(w->c_in == 1 && w->pos_w1, "training (discrete variant): c_in must be 1 and pos_w1 = pos_mlp.weight [K, 32]");
    }
    d.hh = d.v3d ? 512 : (d.rot ? 64 : 32);
    DA_REQUIRE(!d.v3d || w->c_in == 7 || w->c_in == 13,
               "training (3D): c_in must be 7 (quaternion wxyz | translation) or 13 (use_6dof: | a1 | a2), not %d", w->c_in);
    DA_REQUIRE(d.v3d || (w->c_in >= 1 && w->c_in <= 8), "training: c_in %d outside 1 .. 8", w->c_in);
    d.tch = d.v3d ? w->c_in - 4 : 0;
    d.gcn = w->arch == DA_ARCH_GCN;
    DA_REQUIRE(!d.gcn || w->n_layers == 2, "training: gcn arch needs n_layers = 2 (backbones/gcn.py:9-14)");
    DA_REQUIRE(w->heads == 8 && w->n_layers >= 2 && w->n_layers <= DA_MAX_LAYERS, "training: bad heads / n_layers");
    d.nr = g->n_real; d.n = g->n_nodes; d.F = w->feat_dim; d.D = w->feat_dim + 64; d.hid = w->hidden; d.H = w->heads;
    d.L = w->n_layers; d.V = w->arch == DA_ARCH_EXOPHORMER ? w->virt_nodes : 0; d.c_in = w->c_in; d.c_out = d.v3d ? w->c_in : w->c_out;
    d.gelu_between = w->arch == DA_ARCH_TRANSFORMER || d.gcn;
    d.G = g->n_graphs;
    DA_REQUIRE(d.D % d.H == 0 && (d.D / d.H) % 8 == 0, "training: D / heads must be a multiple of 8");
    for (int l = 0; l < d.L; ++l) {
        d.din[l] = l == 0 ? d.D : 32 * d.H;
        d.C[l] = l == d.L - 1 ? d.D / d.H : 32;
        d.hc[l] = d.C[l] * d.H;
        if (d.gcn) { d.hc[l] = l == 0 ? 256 : d.D; d.din[l] = l == 0 ? d.D : 256; d.C[l] = 0; }     // GCNConv(D, 256), GCNConv(256, D)
    }
    if (d.gcn) {          // aggregation in closed form (complete graphs, banded Exphander plans) or over the CSR (da_gcn.hip)
        d.dense = d.hybrid = false;
        d.q16 = false;
        d.pair_floats = 0;
        DA_REQUIRE(gcn_plan_kind(g) >= 0, "training (gcn): plan the Batch without the hybrid split (build_plan(..., hybrid='off'))");
        return 0;
    }
    DA_REQUIRE(g->n_real > 0 && g->n_nodes >= g->n_real, "training: bad graph");
    DA_REQUIRE(d.V == 0 || g->n_nodes == g->n_real + d.V * g->n_graphs, "training: exophormer expects n_nodes = n_real + V*G");
    d.dense = !train_dense_disabled() && g->dense != 0 && g->graph_ptr && d.V == 0 && g->max_graph_nodes > 0;
    d.hybrid = !d.dense && !train_dense_disabled() && g->hybrid && g->mask && g->mask_ptr && g->irr_row_ptr && g->graph_ptr &&
               g->pad_ptr && g->max_graph_nodes > 0;
    // the hybrid training kernels index the adjacency bits by NODE (row i = node - graph_ptr[g]); a plan in the banded slot layout
    // (graph_plan.expander_plan: bits in SLOT space, slot_node != NULL) would be read in the wrong order -- refuse it loudly
    DA_REQUIRE(!(d.hybrid && g->slot_node), "training: hybrid graph in the banded slot layout (slot_node set); train on a natural-layout plan: build_plan(edge_index, batch), expander_plan(..., banded=False) or DA_EXPANDER_LAYOUT=natural");
    DA_REQUIRE(d.dense || d.hybrid || g->row_ptr, "training: this graph walks the edge list but the CSR arrays are missing");
    // hybrid graphs in the bf16-operand mode run flash-style (da_train_dense.hip: k_hyb_*): no pair matrix is ever allocated
    bool flash = d.hybrid && d.bfc;
    for (int l = 0; l < d.L && flash; ++l) flash = hybrid_flash_ok(g, d.C[l], d.bfc);
    d.pair_floats = (d.dense || (d.hybrid && !flash)) ? dense_pair_floats(g, d.H) : 0;
    const bool q16_off = DA_XENV("DA_TRAIN_Q16", 1) == 0 || DA_XENV("DA_TRAIN_TN_DB", 1) == 0;
    d.q16 = d.bfc && d.dense && !q16_off;
    for (int l = 0; l < d.L && d.q16; ++l) d.q16 = attn_small_ok(g, d.C[l], true) && d.din[l] % 32 == 0 && d.C[l] % 8 == 0;
    return 0;
}

// The workspace of a step: order and sizes are what da_train_workspace_bytes reports, so they stay as they are -- the `wt` block
// included, which nothing reads any more (every W^T image has a slot of its own, wt_*).
static TrainWs carve_train(const Dims &d, void *base) {
    char *p = (char *)base;
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *q = p ? (float *)(p + off) : nullptr;
        off += align_up(floats * 4, 256);
        return q;
    };
    const size_t n = (size_t)d.n + 64, nr = (size_t)d.nr + 64;
    TrainWs w;
    w.comb_in = take(nr * d.D);
    w.m1pre = take(nr * d.hid);
    w.m1 = take(nr * d.hid);
    w.h0 = take(n * d.D);
    int hcmax = 0;
    size_t wmax = (size_t)d.D * d.hid;
    for (int l = 0; l < d.L; ++l) {
        w.qkvs[l] = take(n * 4 * d.hc[l]);
        w.o[l] = take(n * d.hc[l]);
        w.hact[l] = ((l < d.L - 1 && d.gelu_between) || d.gcn) ? take(n * d.hc[l]) : nullptr;      // (gcn, last layer: z = gelu(pre) + h0)
        w.stats[l] = take(n * d.H * 2);
        hcmax = d.hc[l] > hcmax ? d.hc[l] : hcmax;
        const size_t ws = (size_t)4 * d.hc[l] * d.din[l];
        wmax = ws > wmax ? ws : wmax;
    }
    w.f1pre = take(nr * d.hh);
    w.f1 = take(nr * d.hh);
    w.dz = take(n * d.D);
    w.dh0 = take(n * d.D);
    w.dY4 = take(n * 4 * hcmax);
    w.dxa = take(n * d.D);
    w.dxb = take(n * d.D);
    w.Dd = take(n * d.H);
    w.dm1 = take(nr * d.hid);
    w.df1 = take(nr * d.hh);
    w.dcomb = take(nr * d.D);
    w.wt = take(wmax + 1024);           // unused (kept: removing it changes da_train_workspace_bytes)
    w.partial = take(PART_CAP);
    w.csum = take(((size_t)d.n / 128 + 2) * 4 * (size_t)hcmax);
    w.pa = take(nr * 16);
    w.p1 = take(nr * 16);
    w.dp1 = take(nr * 16);
    for (int l = 0; l < DA_MAX_LAYERS; ++l) w.P[l] = nullptr;
    w.dP = nullptr; w.poff = nullptr; w.node_graph = nullptr;
    if (d.dense || d.hybrid) {
        for (int l = 0; l < d.L; ++l) w.P[l] = take(d.pair_floats);
        w.dP = take(d.pair_floats);
        w.poff = (long long *)take(2 * ((size_t)d.G + 2));
        w.node_graph = (int32_t *)take(n);
    }
    for (int l = 0; l < DA_MAX_LAYERS; ++l) { w.wt_conv[l] = nullptr; w.wh_conv[l] = nullptr; w.x16[l] = nullptr; }
    for (int l = 0; l < d.L; ++l) {
        const size_t we = (size_t)4 * d.hc[l] * d.din[l];
        w.wt_conv[l] = take(d.q16 ? (we + 1) / 2 : we);
        w.wh_conv[l] = d.q16 ? (bf16_t *)take((we + 1) / 2) : nullptr;
        w.x16[l] = d.q16 ? (bf16_t *)take((n * d.din[l] + 1) / 2) : nullptr;
    }
    w.partial2 = take(PART_CAP);
    w.dY4b = take(n * 4 * hcmax);
    w.wt_head1 = take(d.v3d ? (size_t)d.tch * 256 : (size_t)d.c_out * 32);
    w.wt_head0 = take((size_t)d.hh * d.D);
    w.wt_mlp1 = take((size_t)d.D * d.hid);
    w.wt_mlp0 = take((size_t)d.hid * d.D);
    w.wt_pos1 = take((size_t)32 * 16);
    w.wt_head_r1 = w.pre6 = w.dpre6 = nullptr;
    if (d.v3d) {
        w.wt_head_r1 = take((size_t)3 * 256);
        w.pre6 = take(nr * (3 + d.tch));
        w.dpre6 = take(nr * (3 + d.tch));
    } else if (d.rot) {
        w.wt_head_r1 = take((size_t)4 * 32);
    }
    w.total = off;
    return w;
}

static int check_fused(const da_weights *w, const Dims &d, const char *what) {
    if (d.v3d) {
        DA_REQUIRE(w->head_w0 && w->head_b0 && w->head_w1 && w->head_b1, "%s: 3D head pointers (mlp_t) missing", what);
        DA_REQUIRE(w->head_r_w0 && w->head_r_b0 && w->head_r_w1 && w->head_r_b1, "%s: 3D head_r_* pointers (mlp_r) missing", what);
        DA_REQUIRE(w->head_r_w0 == w->head_w0 + (size_t)256 * d.D && w->head_r_b0 == w->head_b0 + 256,
                   "%s: the 3D heads need mlp_t.0 | mlp_r.0 contiguous in that order, weights and biases (flat parameter buffer)", what);
    }
    if (d.rot) {
        DA_REQUIRE(w->head_w0 && w->head_b0 && w->head_w1 && w->head_b1, "%s: discrete rot head pointers (final_mlp) missing", what);
        DA_REQUIRE(w->head_r_w0 && w->head_r_b0 && w->head_r_w1 && w->head_r_b1, "%s: discrete rot head_r_* pointers (final_mlp_rot) missing", what);
        DA_REQUIRE(w->head_r_w0 == w->head_w0 + (size_t)32 * d.D && w->head_r_b0 == w->head_b0 + 32,
                   "%s: the two heads need final_mlp.0 | final_mlp_rot.0 contiguous in that order, weights and biases (flat parameter buffer)", what);
    }
    for (int l = 0; l < d.L && d.gcn; ++l)
        DA_REQUIRE(w->conv_wq[l] && w->conv_bq[l], "%s: gcn conv %d pointers (lin.weight, bias) missing", what, l);
    for (int l = 0; l < d.L && !d.gcn; ++l) {
        const size_t blk = (size_t)d.hc[l] * d.din[l];
        DA_REQUIRE(w->conv_wq[l] && w->conv_bq[l], "%s: conv %d pointers missing", what, l);
        DA_REQUIRE(w->conv_wk[l] == w->conv_wq[l] + blk && w->conv_wv[l] == w->conv_wq[l] + 2 * blk &&
                       w->conv_ws[l] == w->conv_wq[l] + 3 * blk && w->conv_bk[l] == w->conv_bq[l] + d.hc[l] &&
                       w->conv_bv[l] == w->conv_bq[l] + 2 * d.hc[l] && w->conv_bs[l] == w->conv_bq[l] + 3 * d.hc[l],
                   "%s: conv %d needs lin_query|key|value|skip contiguous in that order (flat parameter buffer)", what, l);
    }
    return 0;
}

static bool q16_cast_on() { return DA_XENV("DA_TRAIN_Q16_CAST", 1) != 0; }

static int weight_prep(const da_weights *w, const Dims &d, TrainWs &ws, hipStream_t st) {
    WPrepTable tab;
    tab.n = 0;
    int maxt = 1;
    auto add = [&](const float *src, void *dst, int rows, int cols, int mode) {
        WPrepJob &j = tab.job[tab.n++];
        j.src = src; j.dst = dst; j.rows = rows; j.cols = cols; j.mode = mode; j.pad = 0;
        const int tiles = ((rows + 31) / 32) * ((cols + 31) / 32);
        maxt = tiles > maxt ? tiles : maxt;
    };
    static_assert(sizeof(WPrepTable) <= 2048, "the job table travels as a kernel argument");
    if (d.v3d) {
        add(w->head_w1, ws.wt_head1, d.tch, 256, 0);
        add(w->head_r_w1, ws.wt_head_r1, 3, 256, 0);
    } else {
        add(w->head_w1, ws.wt_head1, d.c_out, 32, 0);
        if (d.rot) add(w->head_r_w1, ws.wt_head_r1, 4, 32, 0);
    }
    add(w->head_w0, ws.wt_head0, d.hh, d.D, 0);
    add(w->mlp_w1, ws.wt_mlp1, d.D, d.hid, 0);
    add(w->mlp_w0, ws.wt_mlp0, d.hid, d.D, 0);
    if (!d.disc) add(w->pos_w1, ws.wt_pos1, 32, 16, 0);        // (discrete: pos_w1 is the [K, 32] embedding table, no product)
    for (int l = 0; l < d.L && d.gcn; ++l) add(w->conv_wq[l], ws.wt_conv[l], d.hc[l], d.din[l], 0);       // GCNConv lin.weight^T
    for (int l = 0; l < d.L && !d.gcn; ++l) {
        add(w->conv_wq[l], ws.wt_conv[l], 4 * d.hc[l], d.din[l], d.q16 ? 1 : 0);
        if (d.q16) add(w->conv_wq[l], ws.wh_conv[l], 4 * d.hc[l], d.din[l], 2);
    }
    k_weight_prep<<<dim3((unsigned)maxt, (unsigned)tab.n), 256, 0, st>>>(tab);
    DA_LAUNCH_CHECK();
    return 0;
}

// The weight-gradient products run BESIDE the backward's critical path (round 5).  Only dX feeds the next layer; dW = dY^T X and db
// are leaves.  At BASELINE configuration 5 (9 216 nodes per GPU) every kernel of the step is a few hundred workgroups deep in
// dependent load -> LDS -> MFMA stages and leaves most of the chip idle, so the leaves are issued on a side stream of the library
// (fork: an event on the caller's stream once dY is final; join: at the end of every da_train_backward_stage call, i.e. before the
// caller can read a gradient or start an exchange) and overlap with the dX product, the GELU backward and the next layer's attention
// backward.  What the two streams share is kept apart: the side stream has its own split-partial scratch (partial2; csum is only
// ever used by dW products), and the convs' projection gradient dY4 alternates between two buffers -- layer l's attention backward
// may only overwrite the buffer of layer l + 2 after that layer's dW product has read it (done[l + 2]).  DA_TRAIN_SIDE_DW=0: everything
// on the caller's stream, launch for launch the round-4 order.
// one context per (device, caller stream): two engines driven on different streams of one process must not share events
SideDw *side_dw(hipStream_t caller) {
    if (!(cfg().train_side_streams & 1)) return nullptr;          // da_config.train_side_streams bit 0
    struct Slot { int dev; hipStream_t caller; SideDw ctx; };
    static std::mutex mu;
    static std::vector<Slot *> slots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    for (Slot *sl : slots)
        if (sl->dev == dev && sl->caller == caller) return &sl->ctx;
    if (slots.size() >= 64) return nullptr;                 // (a process that cycles through streams: fall back to the one-stream order)
    Slot *sl = new Slot{dev, caller, SideDw()};
    SideDw &c = sl->ctx;
    bool good = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking) == hipSuccess;
    good = good && hipEventCreateWithFlags(&c.fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c.join, hipEventDisableTiming) == hipSuccess;
    for (int l = 0; l < DA_MAX_LAYERS && good; ++l) good = hipEventCreateWithFlags(&c.done[l], hipEventDisableTiming) == hipSuccess;
    if (!good) { delete sl; return nullptr; }
    slots.push_back(sl);
    return &sl->ctx;
}

// ---------------------------------------------------------------------------------------------
// The arguments of an entry point, by name (what an entry does not take stays null / default)
struct TrainCall {
    const da_weights *w = nullptr, *grads = nullptr;        // grads: same struct, written by the library (backward)
    const da_graph *g = nullptr;
    const float *x = nullptr;                               // float poses [n_real, c_in] (2D, 3D), or
    const int32_t *idx = nullptr;                           // position indices [n_real] (discrete) -- exactly one of the two
    const int64_t *t = nullptr;
    const float *feats = nullptr;                           // forward
    float *out = nullptr, *out_rot = nullptr;
    const float *d_out = nullptr, *d_out_rot = nullptr;     // backward
    float *d_feats = nullptr;
    void *workspace = nullptr;
    size_t workspace_bytes = 0;
    int mma_precision = DA_TRAIN_MMA_FP32, stage = DA_TRAIN_BWD_ALL;
    void *stream = nullptr;
    bool rot_entry = false;     // the call came through da_train_forward_rot / da_train_backward_rot (out_rot / d_out_rot: the second head)
};

// A Linear's backward.  Shape: dY [M, N], X [M, K], W [N, K].  The first block is what every call names; the second is named where
// it is used and absent where not.
struct LinBwd {
    int M, N, K;
    const float *dY; int ldy;          // (bf16 bits when dy16)
    const float *X; int ldx;
    const void *WT;                    // the forward's image of W^T (k_weight_prep: fp32, or bf16 when dy16); only read with dX
    float *dW, *db;                    // dW += dY^T X, db += colsum(dY) (db null: no bias gradient here)

    float *dX = nullptr; int lddx = 0; // dX = dY @ W (+ res)
    const float *res = nullptr;
    bool dy16 = false;                 // q16 mode: dY is bf16 (written by k_attn_small_bwd)
    const bf16_t *X16 = nullptr;       // with dy16: the bf16 image of X the forward's projection multiplied (dense, leading dimension K)
    const float *act_ref = nullptr;    // the activation in front of this Linear (dense [M, K] like dX): dX *= act'(act_ref).  act = DA_ACT_GELU:
    int act = DA_ACT_GELU;             // act_ref is its pre-image; DA_ACT_LEAKY02: act_ref is its OUTPUT (= X), dX *= (X > 0 ? 1 : 0.2)
    hipEvent_t done = nullptr;         // recorded behind the dW / db launches when they run on the side stream
};

// A Linear's forward.  A [M, K], W [Nout, K].
struct LinFw {
    int M, K, Nout;
    const float *A; int lda;
    const float *W, *bias;
    float *out; int ldo;

    float *act_out = nullptr;          // dense [M, Nout]: act(out)
    int act = DA_ACT_GELU;             // DA_ACT_LEAKY02 (the 3D mlp): act_out straight from the product's epilogue, `out` is not written (the
};                                     // backward takes the sign from the output)

// the conv layers' running input in the forward
struct LayerIn {
    const float *x; int ld;
    bool x16_ready;                    // x16[l] already holds the bf16 image of x (written by the GELU launch of the layer before)
};

static float *G(const float *p) { return (float *)p; }       // a field of `grads`

// One call of the training path: what its stages share.  Lives on the entry point's stack and allocates nothing -- unlike the
// captured sampling loop, a training step is enqueued by the host every time, so host cost is on the clock.
struct TrainCtx {
    const da_weights *w = nullptr, *grads = nullptr;
    const da_graph *g = nullptr;
    Dims d;
    TrainWs ws;
    hipStream_t st = nullptr;
    SideDw *sd = nullptr;               // null (DA_TRAIN_SIDE_DW=0): everything on the caller's stream
    StreamJoin side_guard;              // every exit joins the side stream (the error exits through its destructor)
    bool do_early = true, do_late = true;       // the stages of a backward call
    int PL = DA_PREC_F32;               // precision code of the linear layers (storage is fp32 either way)
    static constexpr int P = DA_PREC_F32;

    bool dh0_copy() const { return d.n > d.nr; }        // virtual rows: dh0 is materialised (see head_bwd)

    // The argument checks of both directions, in the one order they have always had, then the shapes, the workspace and the streams.
    int open(const TrainCall &a, bool bwd) {
        const char *dir = bwd ? "backward" : "forward", *pose_entry = bwd ? "backward_stage" : "forward_ex";
        int rc;
        DA_REQUIRE(a.mma_precision == DA_TRAIN_MMA_FP32 || a.mma_precision == DA_TRAIN_MMA_BF16, "da_train_%s: unknown mma_precision %d", dir,
                   a.mma_precision);
        if ((rc = dims_of(a.w, a.g, d, a.mma_precision))) return rc;
        DA_REQUIRE(a.rot_entry || !d.rot, "da_train_%s: a discrete rot denoiser has two heads (da_train_forward_rot / da_train_backward_rot)", dir);
        DA_REQUIRE(!a.rot_entry || d.rot, "da_train_%s_rot: not a discrete rot denoiser (variant %d; da_train_%s_idx / da_train_%s)", dir,
                   a.w->variant, dir, pose_entry);
        DA_REQUIRE(bwd || !a.rot_entry || a.out_rot, "da_train_forward_rot: null argument");
        DA_REQUIRE(a.idx || !d.disc, "da_train_%s: a discrete denoiser takes position indices (da_train_%s_idx)", dir, dir);
        DA_REQUIRE(!a.idx || d.disc, "da_train_%s_idx: not a discrete denoiser (da_train_%s takes poses)", dir, pose_entry);
        const bool own = bwd ? a.grads && (a.rot_entry ? a.d_out_rot : a.d_out) : a.feats && a.out;
        DA_REQUIRE(own && (a.x || a.idx) && a.t && a.workspace, "da_train_%s: null argument", dir);
        if (bwd) {
            DA_REQUIRE(!d.disc || (a.grads->variant == a.w->variant && a.grads->c_out == a.w->c_out && a.grads->pos_w1),
                       "da_train_backward_idx: grads must mirror the discrete weights");
            DA_REQUIRE(d.dense || (d.gcn && gcn_plan_kind(a.g) != 2) || (a.g->out_ptr && (a.g->out_dst || d.hybrid)),
                       "da_train_backward: the graph needs the by-source CSR (out_ptr / "
                       "out_dst; of the remainder edges for hybrid graphs, where out_dst may be empty)");
        }
        if ((rc = check_fused(a.w, d, bwd ? "da_train_backward(weights)" : "da_train_forward"))) return rc;
        if (bwd && (rc = check_fused(a.grads, d, "da_train_backward(grads)"))) return rc;
        ws = carve_train(d, a.workspace);
        DA_REQUIRE(a.workspace_bytes >= ws.total, "training workspace too small: %zu < %zu", a.workspace_bytes, ws.total);
        w = a.w; grads = a.grads; g = a.g;
        st = (hipStream_t)a.stream;
        PL = d.bfc ? DA_PREC_F32_BF16MMA : DA_PREC_F32;
        sd = side_dw(st);
        return 0;
    }

    // ---- the two Linear helpers
    // forward: the bf16-operand mode tries the reduction-split launch first (skinny outputs with a long reduction: mlp.0 and the head's
    // first layer leave most CUs idle otherwise); act_out = gelu(out) comes from the split product's second kernel, or from a launch of its own
    int linear_fw(const LinFw &p) {
        if (p.act == DA_ACT_LEAKY02)
            return linear(PL, p.M, p.K, p.Nout, p.A, p.lda, p.W, p.bias, DA_ACT_LEAKY02, nullptr, p.act_out, p.Nout, st);
        if (d.bfc) {
            const int rc = launch_gemm_mfma_splitk(p.M, p.K, p.Nout, p.A, p.lda, p.W, p.bias, nullptr, p.out, p.ldo, ws.partial, PART_CAP, st, false,
                                                   nullptr, p.act_out);
            if (rc >= 0) return rc;             // (-1: shape not taken)
        }
        const int rc = linear(PL, p.M, p.K, p.Nout, p.A, p.lda, p.W, p.bias, DA_ACT_NONE, nullptr, p.out, p.ldo, st);
        if (rc || !p.act_out) return rc;
        return gelu_fwd((size_t)p.M * p.Nout, p.out, p.act_out, st);
    }

    // backward: the activation's derivative is applied inside the reduction-split product's second kernel where that route is taken (GELU
    // only), as a launch of its own otherwise.  With a side stream the dW / db launches go there, behind an event that says dY is final
    int linear_bwd(const LinBwd &p) {
        int rc;
        const float *gelu_pre = p.act == DA_ACT_GELU ? p.act_ref : nullptr;      // (the split product's second kernel fuses the GELU derivative only)
        // the activation tail walks dX as a dense [M, K] image: a strided dX (the 3D heads' halves, lddx = 512) must not ask for one
        DA_REQUIRE(!p.act_ref || !p.dX || p.lddx == p.K, "linear_bwd: an activation reference needs a dense dX (lddx %d != K %d)", p.lddx, p.K);
        auto act_tail = [&]() -> int {
            if (!p.act_ref) return 0;
            const size_t n = (size_t)p.M * p.K;
            return p.act == DA_ACT_LEAKY02 ? leaky_bwd(n, p.act_ref, p.dX, p.dX, st) : gelu_bwd(n, p.act_ref, p.dX, p.dX, st);
        };
        auto split_done = [&](int r) -> int { return (r || gelu_pre == p.act_ref) ? r : act_tail(); };      // the split route fused nothing: apply it now
        hipStream_t sw = st;                                    // stream and split scratch of the dW / db launches
        float *part = ws.partial;
        if (sd) {
            DA_CHECK_HIP(hipEventRecord(sd->fork, st));
            DA_CHECK_HIP(hipStreamWaitEvent(sd->s, sd->fork, 0));
            sw = sd->s;
            part = ws.partial2;
        }
        const bool tn_db = DA_XENV("DA_TRAIN_TN_DB", 1) != 0;
        if (p.dy16) {
            // X16: the same bits the fp32 route rounds to inside the kernel
            if ((rc = p.X16 ? launch_gemm_tn_db(p.M, p.N, p.K, p.dY, p.ldy, p.X16, p.K, p.dW, p.K, part, p.db, ws.csum, sw, true, true)
                            : launch_gemm_tn_db(p.M, p.N, p.K, p.dY, p.ldy, p.X, p.ldx, p.dW, p.K, part, p.db, ws.csum, sw, true))) return rc;
        } else if (d.bfc && tn_db) {                            // dW and db from one pass over dY (k_gemm_tn_db)
            if ((rc = launch_gemm_tn_db(p.M, p.N, p.K, p.dY, p.ldy, p.X, p.ldx, p.dW, p.K, part, p.db, ws.csum, sw))) return rc;
        } else {
            if ((rc = launch_gemm_tn(p.M, p.N, p.K, p.dY, p.ldy, p.X, p.ldx, p.dW, p.K, part, sw, d.bfc))) return rc;
            if (p.db && (rc = colsum_add(p.M, p.N, p.dY, p.ldy, p.db, ws.csum, sw))) return rc;
        }
        if (sd && p.done) DA_CHECK_HIP(hipEventRecord(p.done, sd->s));
        if (!p.dX) return 0;
        if (p.dy16) {
            rc = launch_gemm_mfma_splitk(p.M, p.N, p.K, p.dY, p.ldy, p.WT, nullptr, p.res, p.dX, p.lddx, ws.partial, PART_CAP, st, true, gelu_pre);
            if (rc >= 0) return split_done(rc);                 // (-1: shape not taken)
            rc = launch_gemm_mfma_mixed(true, false, p.M, p.N, p.K, p.dY, p.ldy, p.WT, nullptr, p.res, p.dX, p.lddx, st);
            if (rc < 0) { set_error("training (q16): dX product %d x %d x %d not covered", p.M, p.N, p.K); return 1; }
            return rc ? rc : act_tail();
        }
        if (d.bfc) {                                            // skinny dX with a long reduction: split over the reduction (one launch + a fixed-order sum)
            rc = launch_gemm_mfma_splitk(p.M, p.N, p.K, p.dY, p.ldy, p.WT, nullptr, p.res, p.dX, p.lddx, ws.partial, PART_CAP, st, false, gelu_pre);
            if (rc >= 0) return split_done(rc);
        }
        if ((rc = linear(PL, p.M, p.N, p.K, p.dY, p.ldy, (const float *)p.WT, nullptr, DA_ACT_NONE, p.res, p.dX, p.lddx, st))) return rc;
        return act_tail();
    }

    // ---- forward stages
    // W^T / bf16 images of the step (the backward of this forward reads them too): on the library's side stream, beside the
    // feature copy, the embedding and the mlp -- the first reader is conv 0's projection
    int fork_weight_images() {
        int rc;
        if (sd) {
            DA_CHECK_HIP(hipEventRecord(sd->fork, st));         // (behind the optimizer step / whatever last wrote the weights on the caller's stream)
            DA_CHECK_HIP(hipStreamWaitEvent(sd->s, sd->fork, 0));
            side_guard.arm(sd->s, st, sd->join);
        }
        if ((rc = weight_prep(w, d, ws, sd ? sd->s : st))) return rc;
        // (the pair offsets / node -> graph table of the grouped attention kernels: the same side stream, needed by the first attention)
        if (sd && (d.dense || d.hybrid) && (rc = dense_train_prepare(g, d.H, ws.poff, ws.node_graph, sd->s))) return rc;
        if (sd) DA_CHECK_HIP(hipEventRecord(sd->done[0], sd->s));       // (done[] belongs to the backward; idle during a forward)
        return 0;
    }
    // the weight images are there (nothing else runs on the side stream in a forward)
    int join_weight_images() {
        if (sd) { DA_CHECK_HIP(hipStreamWaitEvent(st, sd->done[0], 0)); side_guard.armed = false; }
        return 0;
    }

    // [feats | pos | time] -> mlp -> h0 (+ the exophormer's virtual rows)
    int embed_mlp(const TrainCall &a) {
        const int nr = d.nr, D = d.D;
        int rc;
        if ((rc = launch_set_feats(P, nr, d.F, D, a.feats, ws.comb_in, st))) return rc;
        if (d.disc) {          // the embed is a gather: pos_mlp.weight[idx] | time_emb[t] (efficient_gat_discrete.py:81-86)
            if ((rc = launch_embed_idx_time(P, nr, d.c_out, d.F, D, a.idx, a.t, 0, w->steps, w->time_emb, w->pos_w1, ws.comb_in, st))) return rc;
        } else if ((rc = launch_embed_pos_time(P, nr, d.c_in, d.F, D, a.x, a.t, 0, w->steps, w->time_emb, w->pos_w0, w->pos_b0, w->pos_w1,
                                               w->pos_b1, ws.comb_in, st))) return rc;
        // mlp: Linear GELU Linear (efficient_gat.py:135); 3D: Linear LeakyReLU(0.2) Linear LeakyReLU(0.2) (efficient_gat_3d.py:136-141)
        if ((rc = linear_fw({.M = nr, .K = D, .Nout = d.hid, .A = ws.comb_in, .lda = D, .W = w->mlp_w0, .bias = w->mlp_b0, .out = ws.m1pre,
                             .ldo = d.hid, .act_out = ws.m1, .act = d.v3d ? DA_ACT_LEAKY02 : DA_ACT_GELU}))) return rc;
        if ((rc = linear(PL, nr, d.hid, D, ws.m1, d.hid, w->mlp_w1, w->mlp_b1, d.v3d ? DA_ACT_LEAKY02 : DA_ACT_NONE, nullptr, ws.h0, D, st))) return rc;
        if (d.V > 0) {
            DA_REQUIRE(w->virt_emb, "exophormer: virt_emb missing");
            if ((rc = launch_set_virtual_rows(P, d.n - nr, d.V, D, w->virt_emb, ws.h0 + (size_t)nr * D, st))) return rc;
        }
        return 0;
    }

    // gcn.py:16-22 with the inference path's reassociation: P0 = h0 W0^T, pre0 = A_hat P0 + b0, a0 = gelu(pre0),
    // Y = A_hat a0, pre1 = Y W1^T + b1, z = gelu(pre1) + h0.  Saved for the backward: qkvs[0] = P0 (unused), o[0] = pre0,
    // hact[0] = a0, qkvs[1] = Y, o[1] = pre1, hact[1] = z, Dd = dinv (CSR plans)
    int gcn_layers_fw(const float *&z) {
        const int n = d.n, D = d.D, hid = d.hc[0];
        float *dinv = ws.Dd;
        int rc;
        if ((rc = launch_gcn_dinv(g, dinv, st))) return rc;
        if ((rc = linear(PL, n, D, hid, ws.h0, D, w->conv_wq[0], nullptr, DA_ACT_NONE, nullptr, ws.qkvs[0], hid, st))) return rc;
        if ((rc = launch_gcn_aggregate(P, g, hid, dinv, ws.qkvs[0], w->conv_bq[0], DA_ACT_NONE, ws.o[0], st))) return rc;
        if ((rc = gelu_fwd((size_t)n * hid, ws.o[0], ws.hact[0], st))) return rc;
        if ((rc = launch_gcn_aggregate(P, g, hid, dinv, ws.hact[0], nullptr, DA_ACT_NONE, ws.qkvs[1], st))) return rc;
        if ((rc = linear(PL, n, hid, D, ws.qkvs[1], hid, w->conv_wq[1], w->conv_bq[1], DA_ACT_NONE, nullptr, ws.o[1], D, st))) return rc;
        if ((rc = launch_gcn_gelu_res((size_t)n * D, ws.o[1], ws.h0, ws.hact[1], st))) return rc;
        z = ws.hact[1];
        return 0;
    }

    // layer l's Q | K | V | skip projection into qkvs[l]
    int project_layer(int l, LayerIn &in) {
        const int n = d.n, din = d.din[l], nout = 4 * d.hc[l];
        if (!d.q16) return linear(PL, n, din, nout, in.x, in.ld, w->conv_wq[l], w->conv_bq[l], DA_ACT_NONE, nullptr, ws.qkvs[l], nout, st);
        // q16: a bf16 projection buffer (same allocation, half used).  Input and weight are rounded to bf16 ONCE, by a pass of their own
        // (into x16[l] and wh_conv[l]), and the projection runs on the bf16 kernels of the inference path (W in registers / a 64-deep LDS
        // ring instead of 128 x 128 fp32 tiles re-streamed through the L2 by every column group); the products are the same
        // bf16 x bf16 -> fp32 ones.  DA_TRAIN_Q16_CAST=0: fp32 operands rounded inside the kernel (launch_gemm_mfma_mixed)
        int rc = -1;
        if (q16_cast_on() && in.ld == din && ((size_t)n * din) % 8 == 0) {
            // (the weight's bf16 image comes from k_weight_prep; the input's from the GELU launch that produced it -- x16_ready --
            //  or, for layer 0 and the architectures without a GELU between the layers, from a cast of its own)
            if (!in.x16_ready && (rc = cast_h((size_t)n * din, in.x, ws.x16[l], st))) return rc;
            in.x16_ready = true;
            rc = launch_gemm_mfma(DA_PREC_BF16, n, din, nout, ws.x16[l], din, ws.wh_conv[l], w->conv_bq[l], DA_ACT_NONE, nullptr, ws.qkvs[l], nout,
                                  nullptr, st);
        }
        if (rc < 0) rc = launch_gemm_mfma_mixed(false, true, n, din, nout, in.x, in.ld, w->conv_wq[l], w->conv_bq[l], nullptr, ws.qkvs[l], nout, st);
        if (rc < 0) { set_error("training (q16): projection %d x %d x %d not covered", n, din, nout); return 1; }
        return rc;
    }

    // layer l's attention into o[l] (the last layer adds the residual h0): complete graphs, hybrid graphs, else the edge list
    int attend_layer(int l) {
        const float *res = l == d.L - 1 ? ws.h0 : nullptr;
        int rc;
        if (d.dense || d.hybrid) {
            if (l == 0 && !sd && (rc = dense_train_prepare(g, d.H, ws.poff, ws.node_graph, st))) return rc;      // (else: fork_weight_images)
            return d.dense ? dense_train_attn_fwd(g, d.H, d.C[l], ws.qkvs[l], res, ws.o[l], ws.P[l], ws.poff, ws.node_graph, st, d.bfc, d.q16)
                           : hybrid_train_attn_fwd(g, d.H, d.C[l], ws.qkvs[l], res, ws.o[l], ws.P[l], ws.stats[l], ws.poff, ws.node_graph, st, d.bfc);
        }
        return launch_attn_csr(P, d.n, g->row_ptr, g->col_src, nullptr, d.H, d.C[l], ws.qkvs[l], res, DA_ACT_NONE, ws.o[l], nullptr, ws.stats[l], st);
    }

    // the graph transformer layers; z = conv output + combined (efficient_gat.py:144)
    int conv_layers_fw(const float *&z) {
        LayerIn in{ws.h0, d.D, false};
        int rc;
        for (int l = 0; l < d.L; ++l) {
            if ((rc = project_layer(l, in))) return rc;
            if ((rc = attend_layer(l))) return rc;
            in = LayerIn{ws.o[l], d.hc[l], false};
            if (l < d.L - 1 && d.gelu_between) {
                // q16 mode: the same launch leaves the bf16 image of the next projection's input in x16[l + 1] (kept for the backward's dW product)
                const bool to16 = d.q16 && q16_cast_on() && ((size_t)d.n * d.hc[l]) % 8 == 0 && d.hc[l] == d.din[l + 1];
                if ((rc = gelu_fwd((size_t)d.n * d.hc[l], ws.o[l], ws.hact[l], st, to16 ? ws.x16[l + 1] : nullptr))) return rc;
                in = LayerIn{ws.hact[l], d.hc[l], to16};
            }
        }
        z = ws.o[d.L - 1];
        return 0;
    }

    // head: final_mlp (efficient_gat.py:145); 3D: mlp_t | mlp_r as one 512-wide hidden product, then the pose head, which leaves its
    // [r | t] pre-image in pre6 for the backward (efficient_gat_3d.py:207-219)
    int head_fw(const float *z, float *out, float *out_rot) {
        const int nr = d.nr;
        int rc;
        if ((rc = linear_fw({.M = nr, .K = d.D, .Nout = d.hh, .A = z, .lda = d.D, .W = w->head_w0, .bias = w->head_b0, .out = ws.f1pre, .ldo = d.hh,
                             .act_out = ws.f1}))) return rc;
        if (d.v3d) return launch_head3d(P, nr, d.tch, ws.f1, w->head_w1, w->head_b1, w->head_r_w1, w->head_r_b1, out, ws.pre6, st);
        if (d.rot)         // Linear(32, K) over columns 0..31 and Linear(32, 4) over columns 32..63: the logits half of the rot sampling step's tail kernel
            return launch_d3pm_rot_tail(P, nr, d.c_out, ws.f1, w->head_w1, w->head_b1, w->head_r_w1, w->head_r_b1, nullptr, nullptr, out, out_rot,
                                        nullptr, st);
        if (d.disc) {      // Linear(32, K): the logits half of the sampling step's tail kernel (fp32 in both modes, row k of final_mlp.2 in registers)
            D3pmRows rows;
            rows.hh = ws.f1;
            return launch_d3pm_tail(P, nr, d.c_out, d.H, &rows, nullptr, 0.f, w->head_w1, w->head_b1, nullptr, out, nullptr, st);
        }
        return launch_head2d(P, nr, d.c_out, ws.f1, w->head_w1, w->head_b1, out, st);
    }

    // ---- backward stages
    // 3D (efficient_gat_3d.py:207-219): d[q | t] -> d[r | t] through the pose head, then mlp_r.2 / mlp_t.2 (K = 256 each, the two
    // halves of the 512-wide hidden layer), one GELU backward over both halves
    int head3d_bwd(const float *d_out) {
        const int nr = d.nr;
        int rc;
        const int lp = 3 + d.tch;                         // [r | t] rows: 6, or 12 with use_6dof (mlp_t.2 is [9, 256] then)
        if ((rc = launch_head3d_bwd(nr, d.tch, ws.pre6, d_out, ws.dpre6, st))) return rc;
        if ((rc = linear_bwd({.M = nr, .N = 3, .K = 256, .dY = ws.dpre6, .ldy = lp, .X = ws.f1 + 256, .ldx = 512, .WT = ws.wt_head_r1,
                              .dW = G(grads->head_r_w1), .db = G(grads->head_r_b1), .dX = ws.df1 + 256, .lddx = 512}))) return rc;
        if ((rc = linear_bwd({.M = nr, .N = d.tch, .K = 256, .dY = ws.dpre6 + 3, .ldy = lp, .X = ws.f1, .ldx = 512, .WT = ws.wt_head1,
                              .dW = G(grads->head_w1), .db = G(grads->head_b1), .dX = ws.df1, .lddx = 512}))) return rc;
        return gelu_bwd((size_t)nr * 512, ws.f1pre, ws.df1, ws.df1, st);
    }
    // two heads (efficient_gat_discrete_rotation.py:111-114): final_mlp.2 over columns 0..31 and final_mlp_rot.2 over columns 32..63 of the
    // 64-wide hidden layer (leading dimension 64, the 3D heads' pattern), then one GELU backward over both halves.  d_out == NULL
    // (only_rotation): no position-head products; its half of the hidden gradient is zero
    int head_rot_bwd(const float *d_out, const float *d_out_rot) {
        const int nr = d.nr;
        int rc;
        if (d_out) {
            if ((rc = linear_bwd({.M = nr, .N = d.c_out, .K = 32, .dY = d_out, .ldy = d.c_out, .X = ws.f1, .ldx = 64, .WT = ws.wt_head1,
                                  .dW = G(grads->head_w1), .db = G(grads->head_b1), .dX = ws.df1, .lddx = 64}))) return rc;
        } else {
            DA_CHECK_HIP(hipMemset2DAsync(ws.df1, 64 * sizeof(float), 0, 32 * sizeof(float), (size_t)nr, st));
        }
        if ((rc = linear_bwd({.M = nr, .N = 4, .K = 32, .dY = d_out_rot, .ldy = 4, .X = ws.f1 + 32, .ldx = 64, .WT = ws.wt_head_r1,
                              .dW = G(grads->head_r_w1), .db = G(grads->head_r_b1), .dX = ws.df1 + 32, .lddx = 64}))) return rc;
        return gelu_bwd((size_t)nr * 64, ws.f1pre, ws.df1, ws.df1, st);
    }
    // head: final_mlp.2, GELU, final_mlp.0 (efficient_gat.py:145) -> dz
    int head_bwd(const float *d_out, const float *d_out_rot) {
        const int nr = d.nr, n = d.n, D = d.D;
        int rc;
        if (d.v3d) rc = head3d_bwd(d_out);
        else if (d.rot) rc = head_rot_bwd(d_out, d_out_rot);
        else rc = linear_bwd({.M = nr, .N = d.c_out, .K = 32, .dY = d_out, .ldy = d.c_out, .X = ws.f1, .ldx = 32, .WT = ws.wt_head1,
                              .dW = G(grads->head_w1), .db = G(grads->head_b1), .dX = ws.df1, .lddx = 32, .act_ref = ws.f1pre});
        if (rc) return rc;
        const float *z = d.gcn ? ws.hact[d.L - 1] : ws.o[d.L - 1];
        if (n > nr) DA_CHECK_HIP(hipMemsetAsync(ws.dz + (size_t)nr * D, 0, (size_t)(n - nr) * D * 4, st));
        if ((rc = linear_bwd({.M = nr, .N = d.hh, .K = D, .dY = ws.df1, .ldy = d.hh, .X = z, .ldx = D, .WT = ws.wt_head0, .dW = G(grads->head_w0),
                              .db = G(grads->head_b0), .dX = ws.dz, .lddx = D}))) return rc;
        // residual: z = conv_out + h0  ->  both get dz.  Without virtual rows dh0 = dz is not materialised: layer 0's dX product
        // takes dz as its residual operand and writes dh0 (dz is read-only from here on)
        if (dh0_copy()) DA_CHECK_HIP(hipMemcpyAsync(ws.dh0, ws.dz, (size_t)n * D * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }

    // GCN (gcn.py:16-22), EARLY: conv 1 -- z = gelu(pre1) + h0, pre1 = Y W1^T + b1
    int gcn_conv1_bwd() {
        const int n = d.n, D = d.D, hid = d.hc[0];
        int rc;
        if ((rc = gelu_bwd((size_t)n * D, ws.o[1], ws.dz, ws.dxa, st))) return rc;                          // d pre1
        return linear_bwd({.M = n, .N = D, .K = hid, .dY = ws.dxa, .ldy = D, .X = ws.qkvs[1], .ldx = hid, .WT = ws.wt_conv[1],
                           .dW = G(grads->conv_wq[1]), .db = G(grads->conv_bq[1]), .dX = ws.dxb, .lddx = hid});          // dW1, db1, dY
    }
    // GCN, LATE: conv 0 -- Y = A_hat a0, a0 = gelu(pre0), pre0 = A_hat P0 + b0, P0 = h0 W0^T; dh0 = dz (residual) + dP0 W0
    int gcn_conv0_bwd() {
        const int n = d.n, D = d.D, hid = d.hc[0];
        int rc;
        if ((rc = launch_gcn_aggregate_t(P, g, hid, ws.Dd, ws.dxb, ws.dY4, st))) return rc;                   // d a0 = A_hat^T dY
        if ((rc = gelu_bwd((size_t)n * hid, ws.o[0], ws.dY4, ws.dY4, st))) return rc;                         // d pre0
        if ((rc = colsum_add(n, hid, ws.dY4, hid, G(grads->conv_bq[0]), ws.partial, st))) return rc;         // db0 (bias after the aggregation)
        if ((rc = launch_gcn_aggregate_t(P, g, hid, ws.Dd, ws.dY4, ws.dY4b, st))) return rc;                  // d P0 = A_hat^T d pre0
        return linear_bwd({.M = n, .N = hid, .K = D, .dY = ws.dY4b, .ldy = hid, .X = ws.h0, .ldx = D, .WT = ws.wt_conv[0],
                           .dW = G(grads->conv_wq[0]), .db = nullptr /* db0: above */, .dX = ws.dh0, .lddx = D, .res = ws.dz});       // dW0, dh0
    }

    // graph transformer layer l of a call whose first layer is l_first; d_o: the gradient of its output, replaced by that of its input
    int conv_layer_bwd(int l, int l_first, const float *&d_o) {
        const int n = d.n, L = d.L, hc = d.hc[l], din = d.din[l];
        int rc;
        // this layer's projection gradient: the two buffers alternate, and the one about to be overwritten was last read by layer
        // l + 2's dW product on the side stream
        float *dY4 = (sd && ((L - 1 - l) & 1)) ? ws.dY4b : ws.dY4;
        if (sd && l + 2 <= l_first) DA_CHECK_HIP(hipStreamWaitEvent(st, sd->done[l + 2], 0));
        if (d.dense) {
            if ((rc = dense_train_attn_bwd(g, d.H, d.C[l], ws.qkvs[l], d_o, ws.P[l], ws.dP, dY4, ws.poff, ws.node_graph, st, d.bfc, d.q16))) return rc;
        } else if (d.hybrid) {
            if ((rc = hybrid_train_attn_bwd(g, d.H, d.C[l], ws.qkvs[l], d_o, ws.P[l], ws.dP, ws.stats[l], ws.Dd, dY4, ws.poff,
                                            ws.node_graph, st, d.bfc, ws.o[l], l == L - 1 ? ws.h0 : nullptr))) return rc;
        } else if ((rc = launch_attn_bwd(g, d.H, d.C[l], ws.qkvs[l], d_o, ws.stats[l], ws.Dd, dY4, st))) return rc;
        const float *xin = l == 0 ? ws.h0 : (d.gelu_between ? ws.hact[l - 1] : ws.o[l - 1]);
        float *dx = (l & 1) ? ws.dxa : ws.dxb;
        // DA_TRAIN_DW_X16=1: the convs' dW products read the bf16 image of X (measured slower: 69 vs 63 us at conv 3); the rest of the
        // condition is the forward's for writing it
        const bool dw_x16 = DA_XENV("DA_TRAIN_DW_X16", 0) != 0 && d.q16 && q16_cast_on() && ((size_t)n * din) % 8 == 0;
        // l == 0: the input is h0, whose gradient also carries the residual branch
        if ((rc = linear_bwd({.M = n, .N = 4 * hc, .K = din, .dY = dY4, .ldy = 4 * hc, .X = xin, .ldx = din, .WT = ws.wt_conv[l],
                              .dW = G(grads->conv_wq[l]), .db = G(grads->conv_bq[l]), .dX = l == 0 ? ws.dh0 : dx, .lddx = din,
                              .res = l == 0 ? (dh0_copy() ? ws.dh0 : ws.dz) : nullptr, .dy16 = d.q16, .X16 = dw_x16 ? ws.x16[l] : nullptr,
                              .act_ref = (l > 0 && d.gelu_between) ? ws.o[l - 1] : nullptr, .done = sd ? sd->done[l] : nullptr}))) return rc;
        if (l > 0) d_o = dx;
        return 0;
    }
    // the layers of this call, last to first (EARLY: L-1 .. 1; LATE: 0, whose incoming gradient is layer 1's dX buffer)
    int conv_layers_bwd() {
        const float *d_o = do_early ? ws.dz : (d.L > 1 ? ws.dxa : ws.dz);
        const int l_first = do_early ? d.L - 1 : 0;
        for (int l = l_first; l >= (do_late ? 0 : 1); --l)
            if (int rc = conv_layer_bwd(l, l_first, d_o)) return rc;
        return 0;
    }

    // virtual-node embedding (exophormer_gnn.py:169-178)
    int virt_bwd() {
        if (d.V == 0) return 0;
        DA_REQUIRE(grads->virt_emb, "exophormer: virt_emb gradient pointer missing");
        k_virt_grad<<<(d.V * d.D + 255) / 256, 256, 0, st>>>(d.n - d.nr, d.V, d.D, ws.dh0 + (size_t)d.nr * d.D, G(grads->virt_emb));
        DA_LAUNCH_CHECK();
        return 0;
    }
    // mlp.2, GELU, mlp.0 (efficient_gat.py:135); 3D: a LeakyReLU behind mlp.2 as well (efficient_gat_3d.py:136-141) -> dcomb
    int mlp_bwd() {
        const int nr = d.nr, D = d.D;
        int rc;
        if (d.v3d && (rc = leaky_bwd((size_t)nr * D, ws.h0, ws.dh0, ws.dh0, st))) return rc;
        if ((rc = linear_bwd({.M = nr, .N = D, .K = d.hid, .dY = ws.dh0, .ldy = D, .X = ws.m1, .ldx = d.hid, .WT = ws.wt_mlp1, .dW = G(grads->mlp_w1),
                              .db = G(grads->mlp_b1), .dX = ws.dm1, .lddx = d.hid, .act_ref = d.v3d ? ws.m1 : ws.m1pre,
                              .act = d.v3d ? DA_ACT_LEAKY02 : DA_ACT_GELU}))) return rc;
        return linear_bwd({.M = nr, .N = d.hid, .K = D, .dY = ws.dm1, .ldy = d.hid, .X = ws.comb_in, .ldx = D, .WT = ws.wt_mlp0,
                           .dW = G(grads->mlp_w0), .db = G(grads->mlp_b0), .dX = ws.dcomb, .lddx = D});
    }
    // concat pieces: [feats | pos | time]
    int concat_bwd(const TrainCall &a) {
        const int nr = d.nr, D = d.D;
        if (a.d_feats) {
            k_copy_cols<<<grid_for((size_t)nr * d.F), 256, 0, st>>>(nr, d.F, ws.dcomb, D, a.d_feats);
            DA_LAUNCH_CHECK();
        }
        k_time_scatter<<<(((nr + 15) / 16) * 32 + 255) / 256, 256, 0, st>>>(nr, D, d.F, w->steps, a.t, ws.dcomb, G(grads->time_emb));
        DA_LAUNCH_CHECK();
        if (d.disc)            // the lookup's gradient: one owner per table row, fixed order (da_d3pm_train.hip); no pos_mlp products
            return launch_embed_idx_grad(nr, d.c_out, D, d.F, a.idx, ws.dcomb, G(grads->pos_w1), st);
        return pos_mlp_bwd(a.x);
    }
    // pos_mlp (efficient_gat.py:133): Linear(c,16) GELU Linear(16,32); the hidden layer is recomputed
    int pos_mlp_bwd(const float *x) {
        const int nr = d.nr;
        int rc;
        k_pos_hidden<<<(nr * 16 + 255) / 256, 256, 0, st>>>(nr, d.c_in, x, w->pos_w0, w->pos_b0, ws.pa, ws.p1);
        DA_LAUNCH_CHECK();
        if ((rc = linear_bwd({.M = nr, .N = 32, .K = 16, .dY = ws.dcomb + d.F, .ldy = d.D, .X = ws.p1, .ldx = 16, .WT = ws.wt_pos1,
                              .dW = G(grads->pos_w1), .db = G(grads->pos_b1), .dX = ws.dp1, .lddx = 16, .act_ref = ws.pa}))) return rc;
        return linear_bwd({.M = nr, .N = 16, .K = d.c_in, .dY = ws.dp1, .ldy = 16, .X = x, .ldx = d.c_in, .WT = nullptr /* the poses are inputs: no dX */,
                           .dW = G(grads->pos_w0), .db = G(grads->pos_b0)});
    }
    // the caller's stream continues behind every dW / db launch of this call
    int join_side() {
        DA_CHECK_HIP(side_guard.join());
        return 0;
    }
};

// One implementation behind the float-pose, the index and the two-head entries
static int train_forward_impl(const TrainCall &a) {
    TrainCtx c;
    const float *z = nullptr;
    int rc;
    if ((rc = c.open(a, false))) return rc;
    if ((rc = c.fork_weight_images())) return rc;
    if ((rc = c.embed_mlp(a))) return rc;
    if ((rc = c.join_weight_images())) return rc;
    if ((rc = c.d.gcn ? c.gcn_layers_fw(z) : c.conv_layers_fw(z))) return rc;
    return c.head_fw(z, a.out, a.out_rot);
}

// The backward in two halves, cut where the gradients of final_mlp and of every conv but the first are complete (the data-parallel
// exchange of that bucket -- 1.7 M of the 3.2 M parameters -- can then run on a side stream under the largest dW / dX products
// of the step, conv 0's, and the mlp / embedding tail): DA_TRAIN_BWD_EARLY = head, convs L-1 .. 1; DA_TRAIN_BWD_LATE = conv 0,
// virtual-node embedding, mlp, concat pieces.  EARLY then LATE on one stream == DA_TRAIN_BWD_ALL, launch for launch.
static int train_backward_impl(const TrainCall &a) {
    TrainCtx c;
    int rc;
    DA_REQUIRE(a.stage == DA_TRAIN_BWD_ALL || a.stage == DA_TRAIN_BWD_EARLY || a.stage == DA_TRAIN_BWD_LATE, "da_train_backward_stage: unknown stage %d",
               a.stage);
    c.do_early = a.stage != DA_TRAIN_BWD_LATE;
    c.do_late = a.stage != DA_TRAIN_BWD_EARLY;
    if ((rc = c.open(a, true))) return rc;
    if (c.sd) c.side_guard.arm(c.sd->s, c.st, c.sd->join);      // every exit joins the dW / db launches of the side stream
    if (c.do_early && (rc = c.head_bwd(a.d_out, a.d_out_rot))) return rc;
    if (c.d.gcn) {
        if (c.do_early && (rc = c.gcn_conv1_bwd())) return rc;
        if (c.do_late && (rc = c.gcn_conv0_bwd())) return rc;
    } else if ((rc = c.conv_layers_bwd())) return rc;
    if (!c.do_late) return c.join_side();
    if ((rc = c.virt_bwd())) return rc;
    if ((rc = c.mlp_bwd())) return rc;
    if ((rc = c.concat_bwd(a))) return rc;
    return c.join_side();
}

}  // namespace da

using namespace da;

extern "C" {

size_t da_train_workspace_bytes(const da_weights *w, const da_graph *g) {
    return da_train_workspace_bytes_ex(w, g, DA_TRAIN_MMA_FP32);
}

size_t da_train_workspace_bytes_ex(const da_weights *w, const da_graph *g, int mma_precision) {
    Dims d;
    if (dims_of(w, g, d, mma_precision)) return 0;
    return carve_train(d, nullptr).total;
}

int da_train_forward(const da_weights *w, const da_graph *g, const float *x, const int64_t *t, const float *feats,
                     float *out, void *workspace, size_t workspace_bytes, void *stream) {
    return da_train_forward_ex(w, g, x, t, feats, out, workspace, workspace_bytes, DA_TRAIN_MMA_FP32, stream);
}

int da_train_forward_ex(const da_weights *w, const da_graph *g, const float *x, const int64_t *t, const float *feats,
                        float *out, void *workspace, size_t workspace_bytes, int mma_precision, void *stream) {
    DA_REQUIRE(x, "da_train_forward: null argument");
    return train_forward_impl({.w = w, .g = g, .x = x, .t = t, .feats = feats, .out = out, .workspace = workspace,
                               .workspace_bytes = workspace_bytes, .mma_precision = mma_precision, .stream = stream});
}

int da_train_forward_idx(const da_weights *w, const da_graph *g, const int32_t *idx, const int64_t *t, const float *feats,
                         float *logits, void *workspace, size_t workspace_bytes, int mma_precision, void *stream) {
    DA_REQUIRE(idx, "da_train_forward_idx: null argument");
    return train_forward_impl({.w = w, .g = g, .idx = idx, .t = t, .feats = feats, .out = logits, .workspace = workspace,
                               .workspace_bytes = workspace_bytes, .mma_precision = mma_precision, .stream = stream});
}

int da_train_forward_rot(const da_weights *w, const da_graph *g, const int32_t *idx, const int64_t *t, const float *feats,
                         float *logits, float *rot_logits, void *workspace, size_t workspace_bytes, int mma_precision, void *stream) {
    DA_REQUIRE(idx && rot_logits, "da_train_forward_rot: null argument");
    return train_forward_impl({.w = w, .g = g, .idx = idx, .t = t, .feats = feats, .out = logits, .out_rot = rot_logits, .workspace = workspace,
                               .workspace_bytes = workspace_bytes, .mma_precision = mma_precision, .stream = stream, .rot_entry = true});
}

int da_train_backward(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                      const int64_t *t, const float *d_out, float *d_feats, void *workspace, size_t workspace_bytes,
                      void *stream) {
    return da_train_backward_ex(w, grads, g, x, t, d_out, d_feats, workspace, workspace_bytes, DA_TRAIN_MMA_FP32, stream);
}

int da_train_backward_ex(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                         const int64_t *t, const float *d_out, float *d_feats, void *workspace, size_t workspace_bytes,
                         int mma_precision, void *stream) {
    return da_train_backward_stage(w, grads, g, x, t, d_out, d_feats, workspace, workspace_bytes, mma_precision, DA_TRAIN_BWD_ALL, stream);
}

int da_train_backward_stage(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                            const int64_t *t, const float *d_out, float *d_feats, void *workspace, size_t workspace_bytes,
                            int mma_precision, int stage, void *stream) {
    DA_REQUIRE(x, "da_train_backward: null argument");
    return train_backward_impl({.w = w, .grads = grads, .g = g, .x = x, .t = t, .d_out = d_out, .d_feats = d_feats, .workspace = workspace,
                                .workspace_bytes = workspace_bytes, .mma_precision = mma_precision, .stage = stage, .stream = stream});
}

int da_train_backward_idx(const da_weights *w, const da_weights *grads, const da_graph *g, const int32_t *idx,
                          const int64_t *t, const float *d_logits, float *d_feats, void *workspace, size_t workspace_bytes,
                          int mma_precision, int stage, void *stream) {
    DA_REQUIRE(idx, "da_train_backward_idx: null argument");
    return train_backward_impl({.w = w, .grads = grads, .g = g, .idx = idx, .t = t, .d_out = d_logits, .d_feats = d_feats, .workspace = workspace,
                                .workspace_bytes = workspace_bytes, .mma_precision = mma_precision, .stage = stage, .stream = stream});
}

int da_train_backward_rot(const da_weights *w, const da_weights *grads, const da_graph *g, const int32_t *idx, const int64_t *t,
                          const float *d_logits, const float *d_rot_logits, float *d_feats, void *workspace, size_t workspace_bytes,
                          int mma_precision, int stage, void *stream) {
    DA_REQUIRE(idx && d_rot_logits, "da_train_backward_rot: null argument");
    return train_backward_impl({.w = w, .grads = grads, .g = g, .idx = idx, .t = t, .d_out = d_logits, .d_out_rot = d_rot_logits,
                                .d_feats = d_feats, .workspace = workspace, .workspace_bytes = workspace_bytes, .mma_precision = mma_precision,
                                .stage = stage, .stream = stream, .rot_entry = true});
}

}  // extern "C"
