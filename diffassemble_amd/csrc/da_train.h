// The denoiser's training path: the record its files share.  da_train.hip (entry points, the forward and the backward as stages),
// da_train_gemm.hip (weight-gradient products, column sums, element-wise pieces), da_train_attn.hip (attention backward over the
// edge list) and da_train_dense.hip (attention on the matrix cores: complete and hybrid graphs) include it; the launchers other
// subsystems call as well (launch_gemm_tn*, colsum_add, launch_transpose_f32) are declared in da_internal.h.
#pragma once
#include "da_gemm_common.h"

namespace da {

constexpr size_t PART_CAP = (size_t)16 << 20;        // floats of split-reduction scratch (64 MB)

inline unsigned grid_for(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

struct TrainWs {
    float *comb_in, *m1pre, *m1, *h0;
    float *qkvs[DA_MAX_LAYERS], *o[DA_MAX_LAYERS], *hact[DA_MAX_LAYERS], *stats[DA_MAX_LAYERS];
    float *f1pre, *f1;
    float *dz, *dh0, *dY4, *dxa, *dxb, *Dd, *dm1, *df1, *dcomb, *partial, *csum, *pa, *p1, *dp1;
    float *wt;                         // UNUSED since k_weight_prep writes the per-matrix images below; still carved (see carve_train)
    float *P[DA_MAX_LAYERS], *dP;      // dense path: attention matrices kept per layer, one gradient scratch
    long long *poff;
    int32_t *node_graph;
    // weight images written by the forward's k_weight_prep launch, read by the backward of the same step: W^T of every Linear with
    // a dX product (fp32; bf16 for the convs in the q16 mode) and, q16 mode, the convs' bf16 forward operands
    void *wt_conv[DA_MAX_LAYERS];
    bf16_t *wh_conv[DA_MAX_LAYERS];
    float *partial2, *dY4b;            // side-stream dW products: their own split scratch, and the second projection-gradient buffer (see SideDw)
    bf16_t *x16[DA_MAX_LAYERS];        // q16 mode: bf16 image of every conv's input (the projection's operand in the forward, X of its dW product in the backward)
    float *wt_head1, *wt_head0, *wt_mlp1, *wt_mlp0, *wt_pos1;
    float *wt_head_r1, *pre6, *dpre6;  // 3D: mlp_r.2's W^T; the heads' [r | t] output and its gradient ([nr, 6]; use_6dof: [nr, 12])
    size_t total;
};

struct Dims {
    int nr, n, F, D, hid, H, L, V, c_in, c_out, G;
    int din[DA_MAX_LAYERS], C[DA_MAX_LAYERS], hc[DA_MAX_LAYERS];
    bool gelu_between;
    bool v3d;                  // DA_VARIANT_3D (efficient_gat_3d.py): LeakyReLU mlp, two pose heads behind one 512-wide hidden product
    int tch;                   // 3D: width of mlp_t.2 = c_in - 4: 3, or 9 with use_6dof (c_in = 13: translation | a1 | a2); 0 otherwise
    int hh;                    // width of the head's hidden layer: 32 (final_mlp.0), 3D: 512 (mlp_t.0 | mlp_r.0), discrete rot: 64 (final_mlp.0 | final_mlp_rot.0)
    bool disc;                 // DA_VARIANT_DISCRETE (efficient_gat_discrete.py): embedding lookup where the pose MLP was, K-wide logits head (c_out = K)
    bool rot;                  // DA_VARIANT_DISCRETE_ROT (efficient_gat_discrete_rotation.py): disc plus a 4-wide rotation head; final_mlp.0 | final_mlp_rot.0 one 64-wide product
    bool gcn;                  // DA_ARCH_GCN (backbones/gcn.py): two GCNConv, aggregation by da_gcn.hip, no attention
    bool dense;                // complete graphs: grouped-GEMM attention (da_train_dense.hip)
    bool hybrid;               // hybrid graphs: masked grouped GEMMs + CSR remainder (da_train_dense.hip)
    bool bfc;                  // DA_TRAIN_MMA_BF16: GEMM operands rounded to bf16 inside the matrix-core kernels (storage stays fp32)
    bool q16;                  // bf16-operand mode on small complete graphs: the projection buffers Q | K | V | skip and their gradient dY4 are
                               // STORED as bf16 (what autocast(bfloat16) makes of the reference's lin_query / key / value / skip outputs): they
                               // are only ever read as bf16 operands (k_attn_small_*, the dX and dW products), and at BASELINE configuration 5
                               // the last layer's two [n, 4608] buffers alone are 340 MB of fp32 per step
    size_t pair_floats;
};

// The library's side stream of one (device, caller stream) and its events (da_train.hip: the rationale stands above side_dw)
struct SideDw {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, done[DA_MAX_LAYERS] = {};
};
SideDw *side_dw(hipStream_t caller);      // null: da_config.train_side_streams bit 0 clear (everything on the caller's stream)

// da_train_gemm.hip: element-wise pieces (the dW / db products and the transposes are declared in da_internal.h)
int gelu_fwd(size_t n, const float *src, float *dst, hipStream_t st, bf16_t *dst16 = nullptr);    // dst16 (optional): the same values rounded to bf16
int gelu_bwd(size_t n, const float *pre, const float *dy, float *dx, hipStream_t st);             // dx = dy * gelu'(pre), dx may alias dy
int leaky_bwd(size_t n, const float *out, const float *dy, float *dx, hipStream_t st);            // LeakyReLU(0.2), from the layer's OUTPUT
int cast_h(size_t n, const float *src, bf16_t *dst, hipStream_t st);                              // dst = bf16(src); n a multiple of 8, both 16-byte aligned

// da_train_attn.hip: attention backward over the edge list, both CSR orientations; writes dQ | dK | dV | dskip into dY4 [n, 4 H C]
int launch_attn_bwd(const da_graph *g, int H, int C, const float *qkvs, const float *d_o, const float *stats, float *Dd, float *dY4,
                    hipStream_t st);

// da_train_dense.hip: complete graphs on the matrix cores (grouped GEMMs, attention matrix kept)
size_t dense_pair_floats(const da_graph *g, int H);
int dense_train_prepare(const da_graph *g, int H, long long *poff, int32_t *node_graph, hipStream_t st);
int dense_train_attn_fwd(const da_graph *g, int H, int C, const float *qkvs, const float *res, float *o, float *P,
                         const long long *poff, const int32_t *node_graph, hipStream_t st, bool bfc, bool q16);
int dense_train_attn_bwd(const da_graph *g, int H, int C, const float *qkvs, const float *d_o, const float *P, float *dP,
                         float *dY4, const long long *poff, const int32_t *node_graph, hipStream_t st, bool bfc, bool q16);
bool attn_small_ok(const da_graph *g, int C, bool bfc);      // the one-workgroup-per-group attention kernels take this layer
// hybrid graphs (adjacency-masked grouped GEMMs over the regular edges + CSR remainder, one softmax over both)
int hybrid_train_attn_fwd(const da_graph *g, int H, int C, const float *qkvs, const float *res, float *o, float *P, float *stats,
                          const long long *poff, const int32_t *node_graph, hipStream_t st, bool bfc);
int hybrid_train_attn_bwd(const da_graph *g, int H, int C, const float *qkvs, const float *d_o, const float *P, float *dP,
                          const float *stats, float *Dd, float *dY4, const long long *poff, const int32_t *node_graph, hipStream_t st, bool bfc,
                          const float *o, const float *res);
bool hybrid_flash_ok(const da_graph *g, int C, bool bfc);     // the flash-style kernels (no pair matrix) take this hybrid layer

}  // namespace da
