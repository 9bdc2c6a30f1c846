// Internal launcher declarations shared by the translation units of libdiffassemble_hip.so.
#pragma once
#include "da_common.h"
#include "da_config.h"

namespace da {

struct DeviceSchedule {
    int steps;
    const float *betas, *alphas_cumprod, *sqrt_recip_alphas, *sqrt_recip_alphas_cumprod,
        *sqrt_recipm1_alphas_cumprod, *sqrt_one_minus_alphas_cumprod, *posterior_variance;
};
inline DeviceSchedule to_dev(const da_schedule *s) {
    return {s->steps, s->betas, s->alphas_cumprod, s->sqrt_recip_alphas, s->sqrt_recip_alphas_cumprod, s->sqrt_recipm1_alphas_cumprod,
            s->sqrt_one_minus_alphas_cumprod, s->posterior_variance};
}

// DDIM update of one element, p_sample_ddim spatial_diffusion.py:555-566,603-627 (fp32, op order kept); shared by
// k_ddim2d and the fused tail of the folded head (k_head_fold), so both produce the same bits.
__device__ __forceinline__ float ddim2d_value(const DeviceSchedule &s, int mean_type, long long ti, int ratio,
                                              int prev_all_nonneg, float eta, float xv, float m, float noise) {
    ti = ti < 0 ? 0 : (ti >= s.steps ? s.steps - 1 : ti);
    const long long tp = ti - ratio;
    const float ap = s.alphas_cumprod[ti];
    const float ap_prev = (prev_all_nonneg && tp >= 0) ? s.alphas_cumprod[tp] : 1.0f;
    const float beta = 1.0f - ap;
    const float x0 = mean_type == DA_MEAN_START_X ? m : (xv - sqrtf(beta) * m) / sqrtf(ap);
    const float eps = (s.sqrt_recip_alphas_cumprod[ti] * xv - x0) / s.sqrt_recipm1_alphas_cumprod[ti];
    const float var = ((1.0f - ap_prev) / (1.0f - ap)) * (1.0f - ap / ap_prev);
    const float std_eta = eta * sqrtf(var);
    float prev = sqrtf(ap_prev) * x0 + sqrtf(1.0f - ap_prev - std_eta * std_eta) * eps;
    if (eta > 0.f) prev += std_eta * noise;
    return prev;
}

// Sampling loop: the deterministic DDIM update (eta = 0, scalar timestep) applied by the head kernel itself --
// one launch less per step.  `done` is set by forward_impl (da_forward.hip) when the folded head took it.
struct DdimFuse {
    DeviceSchedule s;
    int mean_type, ratio, prev_all_nonneg;
    long long t;
    const float *x;            // [n, c] current sample (c == c_out)
    float *x_prev;             // [n, c]
    int done;
    // the NEXT step's embedding + mlp.0 computed by the tail kernel itself (k_tail_fused, plain DDIM loops): the rows of x_prev never leave the
    // registers before they become the next step's h = GELU(mlp.0([features | pos_mlp(x_prev) | time_emb[t - ratio]])) -- per-row work that
    // used to be two more launches per step (k_embed_pos_time + the K = 64 GEMM over the hoisted feature part).  nx_on: requested by the
    // loop; nx_done: the kernel that ran did it (the next forward skips its embedding and mlp.0).
    int nx_on, nx_done, nx_steps, nx_cin, nx_ldw;
    long long nx_t;
    const float *nx_time_emb, *nx_w0, *nx_b0, *nx_w1, *nx_b1;
    const void *nx_wp;         // bf16 mlp.0 weight, columns F .. F + 63 (row stride nx_ldw elements)
    const void *nx_feat_proj;  // bf16 [n, 128]: mlp.0 over the feature columns + bias (hoisted)
    void *nx_h;                // bf16 [n, 128]: written in place (the rows this wave has already consumed)
};

// da_basic.hip
int launch_set_feats(int prec, int n, int F, int D, const float *feats, void *comb_in, hipStream_t st);
int launch_set_virtual_rows(int prec, int rows, int V, int D, const void *emb, void *dst, hipStream_t st);
// the constant conv-0 projections of the exophormer's virtual rows (launch_scatter_virtual's arguments): given to launch_embed_pos_time they are
// placed by extra workgroups of the embedding's launch -- the first kernel of a step -- instead of a launch of their own behind the projection
struct VirtScatter {
    int rows = 0, V = 0, H = 0, C = 0, n_real = 0, n_pad = 0;
    const void *src = nullptr;
    const int32_t *row_map = nullptr;
    void *Q = nullptr, *K = nullptr, *Vt = nullptr, *S = nullptr;
};
int launch_embed_pos_time(int prec, int n, int c_in, int F, int D, const float *x, const int64_t *t, int64_t t_scalar,
                          int steps, const float *time_emb, const float *w0, const float *b0, const float *w1,
                          const float *b1, void *comb_in, hipStream_t st, const VirtScatter *vs = nullptr);
int launch_gemm_simple(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias,
                       int act, const void *res, void *out, int ldo, hipStream_t st);
int launch_head2d(int prec, int n, int c_out, const void *hh, const float *w2, const float *b2, float *out, hipStream_t st);
int launch_ddim2d(const DeviceSchedule &s, int mean_type, int n, int c, const float *x, const float *mo,
                  const int64_t *t, int64_t t_scalar, int ratio, int prev_all_nonneg, float eta, const float *noise,
                  float *x_prev, hipStream_t st);
int launch_ddpm2d(const DeviceSchedule &s, int n, int c, const float *x, const float *mo, const int64_t *t,
                  int64_t t_scalar, const float *noise, float *x_prev, hipStream_t st);
int launch_convert(int prec, size_t n, const float *src, void *dst, hipStream_t st);
// da_train_gemm.hip: the products and sums of the training paths that more than one subsystem calls (the denoiser's own record: da_train.h)
int launch_transpose_f32(int rows, int cols, const float *src, float *dst, hipStream_t st);      // dst[c][r] = src[r][c]
// C (+)= A^T B over rows (A [M, N], B [M, K] row-major; split-row partials through `partial`, >= 16 M floats)
int launch_gemm_tn(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, float *partial,
                   hipStream_t st, bool bfc = false);      // bfc: operands rounded to bf16 inside the kernel (DA_TRAIN_MMA_BF16)
int launch_gemm_tn_bf16(int M, int N, int K, const bf16_t *A, int lda, const bf16_t *B, int ldb, float *C, int ldc, float *partial,
                        hipStream_t st);
int launch_gemm_mfma_splitk(int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias, const void *res,
                            void *out, int ldo, float *partial, size_t partial_floats, hipStream_t st, bool in16 = false,
                            const float *gelu_pre = nullptr, float *act_out = nullptr);   // da_gemm_mfma.hip; -1: shape not taken.  gelu_pre: out *= gelu'(pre); act_out = gelu(out)
int launch_gemm_mfma_mixed(bool in16, bool out16, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias,
                           const void *res, void *out, int ldo, hipStream_t st);                              // fp32 x fp32 -> bf16 / bf16 x bf16 -> fp32
int launch_gemm_tn_db(int M, int N, int K, const void *A, int lda, const void *B, int ldb, float *C, int ldc, float *partial,
                      float *db, float *bscratch, hipStream_t st, bool a16 = false, bool b16 = false);                                            // dW + db, bf16-operand mode
int colsum_add(int M, int N, const float *A, int lda, float *out, float *scratch, hipStream_t st);   // out[c] += sum_m A[m][c]
// da_encoder.hip: implicit-GEMM convolution over zero-haloed NHWC maps; the fp32 stem
int launch_conv(int prec, int B, const void *X, int Cin, int Hi, const void *W, const float *bias, const void *res, void *Y,
                int Cout, int ksize, int stride, int relu, hipStream_t st);
int launch_enc_stem(int prec, int B, const float *patches, const float *w, const float *bias, void *Y, int relu, hipStream_t st);
int launch_mm_nn_f32(int M, int N, int K, const float *A, int lda, const float *B, int ldb, const float *bias, float *C,
                     int ldc, hipStream_t st);
int launch_scatter_virtual(int prec, int rows, int V, int H, int C, const void *src, int n_real, const int32_t *row_map,
                           int n_pad, void *Q, void *K, void *Vt, void *S, void *qkvs, hipStream_t st);
int launch_tail_fused(int prec, int n, int H, int c_out, int hidden, int din, const void *h, const void *xin, int ldx, const void *wh,
                      const float *bh, const void *wsk, const float *bsk, const void *pz, const float *w2, const float *b2, float *out,
                      hipStream_t st, DdimFuse *dfp);
int launch_head_fold(int prec, int n, int H, int c_out, const void *pz, const void *pre, const float *w2, const float *b2,
                     float *out, hipStream_t st, const DdimFuse *df = nullptr);

// da_attn_csr.hip
// tiny complete graphs (<= 32 pieces) at C = 104: K | V of a graph staged in LDS (da_attn_csr.hip); 0 = launched, -1 = shape not covered
int launch_attn_tiny(int prec, int n_graphs, int max_graph_nodes, const int32_t *graph_ptr, int nodiag, int heads, int C, const void *qkvs,
                     const void *residual, int act, void *out, hipStream_t st);
int launch_attn_csr(int prec, int n_nodes, const int32_t *row_ptr, const int32_t *col_src, const int32_t *edge_id,
                    int heads, int C, const void *qkvs, const void *residual, int act, void *out, float *alpha,
                    float *stats /* [n, H, 2] running max and 1/(sum + 1e-16), or NULL */, hipStream_t st);

// da_so3.hip (3D head + SO(3) DDIM)
// t_ch = the translation head's width: 3, or 9 with use_6dof (translation | a1 | a2); pose rows are 4 + t_ch wide, [r | t] rows 3 + t_ch
int launch_head3d(int prec, int n, int t_ch, const void *hh, const float *wt, const float *bt, const float *wr, const float *br,
                  float *out7, float *pre_head, hipStream_t st);
int launch_head3d_bwd(int n, int t_ch, const float *pre, const float *d_out, float *d_pre, hipStream_t st);     // [r | t], d[q | t] -> d[r | t]
int launch_ddim3d(const DeviceSchedule &s, int mean_type, int n, int t_ch, const float *x, const float *mo, const int64_t *t,
                  int64_t t_scalar, int ratio, int prev_all_nonneg, float *x_prev, hipStream_t st);

// da_gemm_mfma.hip / da_attn_dense.hip (dense block-diagonal path)
// Joins a library-owned side stream back into the caller's stream on EVERY exit of the scope that forked it (an early
// `return rc` between fork and join left side-stream work un-joined while the caller freed or rewrote the workspace).  The success
// path calls join() itself (and sees its errors); the destructor covers the error exits, best effort.
struct StreamJoin {
    hipStream_t side = nullptr, caller = nullptr;
    hipEvent_t ev = nullptr;
    bool armed = false;
    void arm(hipStream_t side_, hipStream_t caller_, hipEvent_t ev_) { side = side_; caller = caller_; ev = ev_; armed = true; }
    hipError_t join() {
        if (!armed) return hipSuccess;
        armed = false;
        hipError_t e = hipEventRecord(ev, side);
        return e == hipSuccess ? hipStreamWaitEvent(caller, ev, 0) : e;
    }
    ~StreamJoin() { (void)join(); }
};
struct QkvScatter {            // where the fused projection scatters its four column blocks
    int HC, C, n_pad;
    int Cv = 0;                // > 0: three blocks only (Q | K | V'), V' heads Cv wide (folded value heads), no skip
    int blocks = 0;            // > 0: only the first `blocks` column blocks exist (2: a K | V-only projection hands its blocks in through the Q and K slots)
    int col0 = 0;              // > 0 (a multiple of 128): the launch starts at this column of the Q | K | V | skip row -- Nout is that much shorter, W and bias are
                               // handed in offset by col0 rows, every column lands where the full launch puts it (HC: the K | V' projection of a folded last
                               // layer whose attention kernel projects Q itself).  Every kernel launch_gemm_mfma can pick takes it.
    const int32_t *row_map;    // node -> padded row
    void *Q, *K, *Vt, *S;      // [H][n_pad][C] x 3 (Vt keeps its name; V is row-major since the tr_b16 rewrite), [M][H*C]
};
struct DenseLayout {
    const void *Q, *K, *Vt, *S;
    int n_pad;
    int q_prescaled = 0;       // Q rows already carry log2(e) / sqrt(C) (projection weights scaled at pack time, da_denoiser.h ConvW::wd)
    // the layer's projection inside the resident attention kernel (attn_qsf_applicable; no projection kernel runs: the attention kernel writes Q / S
    // itself and keeps K | V in LDS):
    const void *x = nullptr;   // the layer's input rows [N][ldx], bf16
    int ldx = 0, kin = 0;
    const void *wqs = nullptr; // pack_w_qs image of the layer's projection weights
    const float *bias = nullptr;   // [4 * H * 32]: Q | K | V | skip
    // fragment-major rows over the padded slots (AttnDenseParams::x_fm / out_fm; only with x set): x is stored so / out is written so
    bool x_fm = false, out_fm = false;
};
// da_attn_dense.hip / da_attn_opt.hip: whether launch_attn_dense will take the resident kernel's projection-in-the-prologue form for this layer
bool attn_qsf_applicable(int prec, int heads, int C, int kin, int n_graphs, int max_graph_nodes, int n_pad, int q_prescaled);
// the switch: da_config.disable_folds bit 64 (DA_FOLD_ATTN_PROJ) clear, the default (experiments build: DA_ATTN_RES_QSF=0 / 1 overrides).  A denoiser
// asks ONCE, when it is created, like for every other fold (da_denoiser::attn_qsf: it packs the weight image then or never); da_conv_dense_ex, which
// keeps nothing between calls, asks per call
bool attn_qsf_enabled();
// da_attn_dense.hip / da_attn_opt.hip: the un-masked folded last layer with Q projected in the attention kernel's prologue (k_attn_optt<144, true, false, ..,
// 8192>; DenseLayout::x / wqs = pack_w_qlast image / bias = the Q bias): whether launch_attn_dense takes the form for this layer, and the switch
// (da_config.disable_folds bit 256, DA_FOLD_LAST_QPROJ, clear; asked once per denoiser at creation, per call by da_conv_dense_ex)
bool attn_last_qproj_applicable(int prec, int heads, int C, int kin, int n_pad, int q_prescaled);
bool attn_last_qproj_enabled();
size_t w_qlast_bytes(int heads, int C, int kin);
int pack_w_qlast(int heads, int C, int kin, const void *wq, void *packed, hipStream_t st);
long long attn_last_qproj_launches(int reset);   // da_attn_opt.hip: launches of the folded last layer that projected Q themselves
size_t w_qs_bytes(int heads, int kin);
int pack_w_qs(int heads, int kin, int hc, const void *wd, void *packed, hipStream_t st);
// wpacked: optional fragment-major copy of W (pack_w_xpanel) for the row-panel kernel (da_gemm_xpanel.hip)
int launch_gemm_mfma(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias,
                     int act, const void *res, void *out, int ldo, const QkvScatter *qs, hipStream_t st, int ldw = 0,
                     const void *pre = nullptr, const void *wpacked = nullptr);
size_t xpanel_packed_bytes(int K, int Nout);
bool xpanel_in_model();          // DA_ENABLE_XPANEL=1 (off by default, see da_gemm_xpanel.hip)
void gemm_thin_set(int v);      // run-time form of DA_GEMM_THIN (da_gemm_mfma.hip): 1 = projections take the co-resident kernel of da_gemm_thin.hip
int xpanel_mode();               // 0 never, 1 always, 2 = Batches whose largest graph has >= 512 pieces (the default, DA_STEP_AUTO)
int pack_w_xpanel(int K, int Nout, const void *W, int ldw, void *packed, hipStream_t st);
struct DenseMask {             // hybrid mode: adjacency bits of the regular edges + the remainder CSR (da_attn_dense.hip)
    const uint8_t *mask;
    const int64_t *mask_ptr;
    const int32_t *irr_row_ptr, *irr_col_src, *row_map;
    const int32_t *slot_node = nullptr;            // banded layout: slot -> node (da_graph.slot_node)
    const uint8_t *blk_class = nullptr;            // block classes (da_graph.blk_class*)
    const int64_t *blk_class_ptr = nullptr;
    int blk_class_stride = 0;
    const int32_t *rm_meta = nullptr;              // per-slot remainder metadata (da_graph.rm_meta)
    // the virtual rows of the exophormer arch inside the masked attention's launch (AttnDenseParams::v_*): set v_rows > 0 to ask for it;
    // *v_taken is set to 1 by the launcher whose kernel took them (else the caller launches launch_attn_csr_cont itself)
    int v_rows = 0, v_n_real = 0;
    const int32_t *v_row_ptr = nullptr, *v_col_src = nullptr;
    const float *v_mult = nullptr;
    float *v_part = nullptr;
    unsigned *v_cnt = nullptr;
    int *v_taken = nullptr;
};
constexpr int DA_VIRT_SPLIT_MAX = 8;               // workgroups per virtual row at most (sizes the scratch)
inline DenseMask dense_mask_of(const da_graph *g) {
    DenseMask mk;
    mk.mask = g->mask; mk.mask_ptr = g->mask_ptr; mk.irr_row_ptr = g->irr_row_ptr; mk.irr_col_src = g->irr_col_src; mk.row_map = g->row_map;
    mk.slot_node = g->slot_node;
    mk.rm_meta = g->rm_meta;
    const bool cls = g->blk_class && g->blk_class_ptr && g->blk_class_stride > 0;
    mk.blk_class = cls ? g->blk_class : nullptr; mk.blk_class_ptr = cls ? g->blk_class_ptr : nullptr; mk.blk_class_stride = cls ? g->blk_class_stride : 0;
    return mk;
}
struct DenseFold {             // value heads folded with the next linear layer: V is [H][n_pad][cv], output per head
    int cv;
    void *out;                 // [H][n_rows][cv] in the activation dtype, normalised
    int n_rows;
};
int launch_attn_dense(int prec, const DenseLayout &L, int heads, int C, int n_graphs, int max_graph_nodes,
                      const int32_t *graph_ptr, const int32_t *pad_ptr, int nodiag, const void *res, int act,
                      void *out, hipStream_t st, const DenseMask *mk = nullptr, const DenseFold *fold = nullptr);
// da_attn_dual.hip: bf16, complete graphs, two query slabs per wave; Q must arrive pre-scaled by log2(e) / sqrt(C)
int launch_attn_dual(const DenseLayout &L, int heads, int C, int n_graphs, int max_graph_nodes, const int32_t *graph_ptr,
                     const int32_t *pad_ptr, int nodiag, int act, void *out, const DenseFold *fold, hipStream_t st);
// fallback counters of the shift-free softmax kernels (da_debug_counters)
int attn_dense_counters(unsigned long long *out4, int reset);
long long attn_virt_launches(int reset);     // da_attn_opt.hip: masked hidden-layer launches that carried the virtual rows
long long attn_res_launches(int reset);      // da_attn_opt.hip: launches of the K / V-resident kernel since the last reset
long long attn_res_qsf_launches(int reset);  // ... those of them that projected their layer themselves
long long attn_res_fm_launches(int reset);   // ... and of those, the ones that read their input rows fragment-major
int attn_dual_counters(unsigned long long *out2, int reset);
// hybrid mode: the rows the masked kernel does not own (virtual nodes) over their remainder edges
int launch_attn_csr_cont(int prec, int n_nodes, int n_real, const int32_t *irr_row_ptr, const int32_t *irr_col_src,
                         const int32_t *row_map, int heads, int C, int n_pad, const DenseLayout &L,
                         const void *residual, int act, void *out, hipStream_t st,
                         const float *mult = nullptr /* multiplicity per (aggregated) remainder edge, or NULL = 1 */);

// da_conv_fused.hip: one hidden conv (projection + attention of a (graph, head)) as ONE kernel, K / V resident in LDS
bool conv_fused_applicable(int prec, int heads, int C, int kin, int max_graph_nodes, int ldo);
int launch_conv_fused(int prec, int heads, int C, int kin, int n_graphs, int max_graph_nodes, const int32_t *graph_ptr,
                      int nodiag, const void *x, int ldx, const void *W, const float *bias, int act, void *out, int ldo,
                      hipStream_t st);

// da_pcd_encoder.hip: the eval passes of the point-cloud encoder, reused by its training path (da_pcd_train.hip)
int pcd_knn_launch(int clouds, int N, int dim, const float *x, int ldx, int32_t *idx, const float *xn, hipStream_t st);
int pcd_premap_launch(int C, const float *X, int ldx, const float *Wm, long long total, float *T, hipStream_t st);
int pcd_edge_launch(const float *T, const int32_t *idx, const float *bn_a, const float *wb, int N, int clouds, float *Xout,
                    float *xn, hipStream_t st);
// conv6 + its activation + mean over points (partial: clouds * ceil(N / 256) * feat * 3 floats), then k_pcd_final into out
int pcd_conv6_final_launch(const float *X1, const float *X2, const float *X3, const float *w6, int feat, int N, int clouds,
                           float *partial, const float *lin0, int inv, float *out, int ldo, hipStream_t st);

// da_gcn.hip: the GCN backbone's aggregation (0 = dense, 1 = band, 2 = csr, -1 = no path for this plan)
int gcn_plan_kind(const da_graph *g);
int launch_gcn_dinv(const da_graph *g, float *dinv, hipStream_t st);
int launch_gcn_aggregate(int prec, const da_graph *g, int W, const float *dinv, const void *X, const float *bias, int act, void *out,
                         hipStream_t st);
int launch_gcn_aggregate_t(int prec, const da_graph *g, int W, const float *dinv, const void *X, void *out, hipStream_t st);   // A_hat^T X
int launch_gcn_gelu_res(size_t n, const float *pre, const float *res, float *out, hipStream_t st);                           // gelu(pre) + res

// da_d3pm.hip: the discrete (D3PM) variant's embedding lookup and its tail (logits head + guidance + categorical reverse step)
struct D3pmStep {
    DeviceSchedule s = {};
    const int32_t *x_t = nullptr;
    const int64_t *t = nullptr;
    int64_t t_scalar = 0;
    int ratio = 1;
    const float *noise = nullptr;        // [n, K] uniforms of this iteration, or NULL: drawn from `seed`
    const uint64_t *seed = nullptr;      // device {seed, offset}
    int iteration = 0;
    int32_t *x_prev = nullptr;
    float *post = nullptr;               // nullable [n, K]: the posterior logits before the Gumbel term
};
// launch_embed_idx_time_rot (below) without the addend rows
int launch_embed_idx_time(int prec, int n, int K, int F, int D, const int32_t *idx, const int64_t *t, int64_t t_scalar, int steps,
                          const float *time_emb, const float *pos_emb, void *comb_in, hipStream_t st);
// where a pass left its final_mlp.0 rows: post-GELU `hh` [n, 32], or (last-layer fold) the per-head outputs `pz` [H, n, 32] of the folded
// attention with the pre-activation addend `pre` [n, 32] -- hh = GELU(pre + sum_h pz_h), summed in k_head_fold's order; act dtype
struct D3pmRows {
    const void *hh = nullptr, *pz = nullptr, *pre = nullptr;
};
// Philox4x32-10 (Salmon et al., SC'11).  One uniform per flat element e = r K + k: key = the two halves of seed[0], counter =
// (e + seed[1] as 64 bits, iteration, a constant); the first output word gives u = ((bits >> 8) + 1) 2^-24 in (0, 1].  The constant
// names the draw's DOMAIN: the reverse step's Gumbel uniforms (the default) and the training-side noising of q_sample
// (da_d3pm_train.hip) use different words, so one seed never gives the two the same stream.
constexpr uint32_t D3PM_WORD_SAMPLING = 0xD3B07384u, D3PM_WORD_TRAINING = 0x51ED270Bu;
constexpr uint32_t D3PM_WORD_SAMPLING_ROT = 0x2A65C0F1u;      // the rotation half of the position + rotation model (da_d3pm_rot.hip)
constexpr uint32_t D3PM_WORD_TRAINING_ROT = 0x7C3A91E5u;      // the rotation half of the training-side noising (da_d3pm_rot_train.hip)
inline uint32_t d3pm_domain_word(int domain) {
    return domain == DA_D3PM_DRAW_TRAINING ? D3PM_WORD_TRAINING : domain == DA_D3PM_DRAW_SAMPLING_ROT ? D3PM_WORD_SAMPLING_ROT :
           domain == DA_D3PM_DRAW_TRAINING_ROT ? D3PM_WORD_TRAINING_ROT : D3PM_WORD_SAMPLING;
}
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t ctr, uint32_t iteration, uint32_t word = D3PM_WORD_SAMPLING) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = iteration, c3 = word;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (float)((c0 >> 8) + 1u) * 5.9604644775390625e-8f;
}
// da_d3pm_train.hip: pos_mlp.weight.grad[idx[r]] += dcomb[r, F : F + 32], one owner per table row, fixed order
int launch_embed_idx_grad(int n, int K, int D, int F, const int32_t *idx, const float *dcomb, float *grad, hipStream_t st);
// the training-side noising of both discrete models, either half optional: x_noisy NULL skips the K-wide position draw, rot_noisy NULL
// the four-wide rotation draw
int launch_d3pm_q_sample(int n, int K, const da_schedule *s, const int32_t *x_start, const int32_t *rot_start, const int64_t *t,
                         const float *noise_x, const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_noisy,
                         int32_t *rot_noisy, hipStream_t st);
// logits from the conditional rows (and the unconditional ones under guidance) through w2 / b2, or given (logits_in: rows_c may be
// NULL); logits_out nullable; step == NULL: logits only
int launch_d3pm_tail(int prec, int n, int K, int H, const D3pmRows *rows_c, const D3pmRows *rows_u, float cfg_w, const float *w2,
                     const float *b2, const float *logits_in, float *logits_out, const D3pmStep *step, hipStream_t st);

// da_d3pm_rot.hip: the position + rotation variant (DA_VARIANT_DISCRETE_ROT).  The embedding lookup (pos_emb[idx] | time_emb[t] into
// comb_in) that, given proj4, also copies row rot_acc[r] of the four hoisted feature projections proj4 [4][img_stride] (rows of `hidden`
// elements, act dtype) into `sel` [n, hidden], the addend of the K = 64 mlp.0 product; rot_acc NULL = image 0
int launch_embed_idx_time_rot(int prec, int n, int K, int F, int D, int hidden, const int32_t *idx, const int32_t *rot_acc, const int64_t *t,
                              int64_t t_scalar, int steps, const float *time_emb, const float *pos_emb, void *comb_in, const void *proj4,
                              size_t img_stride, void *sel, hipStream_t st);
struct D3pmRotStep {
    DeviceSchedule s = {};
    const int32_t *x_t = nullptr, *rot_t = nullptr;
    const int64_t *t = nullptr;
    int64_t t_scalar = 0;
    int ratio = 1;
    const float *noise_x = nullptr, *noise_rot = nullptr;      // [n, K] / [n, 4] uniforms of this iteration, or NULL: drawn from `seed`
    const uint64_t *seed = nullptr;
    int iteration = 0;
    int32_t *x_prev = nullptr, *rot_0 = nullptr, *rot_prev = nullptr;       // rot_0 / rot_prev nullable
    float *post_x = nullptr, *post_rot = nullptr;                           // nullable
    // the loop's state update: rot_next = cold ? rot_prev : rot_0, rot_acc_out = (rot_acc_in + rot_next) % 4 (rot_acc_in NULL = 0)
    int cold = 0, need_prev = 1;                                            // need_prev 0: the rotation posterior and its draws are skipped
    const int32_t *rot_acc_in = nullptr;
    int32_t *rot_next = nullptr, *rot_acc_out = nullptr;
};
// hh [n, 64] post-GELU rows (final_mlp.0 | final_mlp_rot.0) through w2 [K, 32] / wr [4, 32], or given logits (logits_in + rot_logits_in);
// logits_out / rot_logits_out nullable; step NULL: logits only
int launch_d3pm_rot_tail(int prec, int n, int K, const void *hh, const float *w2, const float *b2, const float *wr, const float *br,
                         const float *logits_in, const float *rot_logits_in, float *logits_out, float *rot_logits_out,
                         const D3pmRotStep *step, hipStream_t st);

// generic linear dispatch (MFMA when the shape allows, else simple)
int linear(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias, int act,
           const void *res, void *out, int ldo, hipStream_t st);

}  // namespace da
