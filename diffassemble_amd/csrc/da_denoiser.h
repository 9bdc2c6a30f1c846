// The denoiser's host record and its workspace layout.  Private to three translation units: da_api.hip (entry points, loop graphs),
// da_denoiser_create.hip (the record's weights, built once per checkpoint) and da_forward.hip (one forward over it).
#pragma once
#include <vector>

#include "da_common.h"
#include "da_internal.h"
#include "da_config.h"

namespace da {

struct ConvW {
    void *w = nullptr;     // [4*HC, Din] act dtype, rows = Q | K | V | skip
    float *b = nullptr;    // [4*HC] fp32
    // the same projection for the matrix-core attention kernels (da_attn_dense.hip / da_attn_dual.hip): the Q rows and
    // biases are PRE-SCALED by log2(e) / sqrt(C), so that the kernels' scores arrive in log2 units and exp2 applies to them
    // directly -- the softmax scale costs no instruction per score (scaled in fp32, before the rounding to the act dtype)
    void *wd = nullptr;
    float *bd = nullptr;
    void *wdp = nullptr;   // wd in the fragment order of the row-panel projection kernel (da_gemm_xpanel.hip), bf16 only
    void *wqs = nullptr;   // wd as per-head MFMA fragments (pack_w_qs): hidden layers whose attention kernel does the projection itself
    int din = 0, hc = 0, C = 0;
};

struct LoopKey {
    da_graph g;
    da_schedule s;
    int mean_type, ratio, max_iters;
    const float *x_init;
    float *traj, *x_final;
    void *ws;
    size_t ws_bytes;
    da_loop_opts opts;        // zero for the plain DDIM loop
    size_t traj_stride;       // elements between consecutive iterations of `traj` (0 = n_real * c)
    size_t noise_stride;      // the same for opts.noise (two-branch loops read row ranges of one [n_iters, N, c] buffer)
    da_config cfg;            // the switches the graph was recorded under (da_config_set between two calls records a new graph)
    const void *seed;         // da_sample_loop_idx: the device {seed, offset} pair the recorded kernels read (NULL otherwise)
    // da_sample_loop_rot (mean_type -2): the rotation side's pointers and the cold switch (zero otherwise)
    const void *rot_init, *rot_traj, *rot_final, *x_fixed, *noise_rot;
    int cold;
};

}  // namespace da

struct da_denoiser {
    int prec = 0, variant = 0, arch = 0, steps = 0, c_in = 0, c_out = 0, F = 0, D = 0, hidden = 0, heads = 0,
        n_layers = 0, V = 0, head_hidden = 0;
    float *time_emb = nullptr, *pos_w0 = nullptr, *pos_b0 = nullptr, *pos_w1 = nullptr, *pos_b1 = nullptr;
    void *mlp_w0 = nullptr, *mlp_w1 = nullptr;
    float *mlp_b0 = nullptr, *mlp_b1 = nullptr;
    da::ConvW conv[DA_MAX_LAYERS];
    void *virt_emb = nullptr;
    void *head_w0 = nullptr;
    float *head_b0 = nullptr;
    float *head_w1 = nullptr, *head_b1 = nullptr, *head_r_w1 = nullptr, *head_r_b1 = nullptr;
    // 2D transformer arch: mlp.2 has no activation, so it is composed into its two consumers once per
    // checkpoint (da_denoiser_create.hip: fold_mlp2): conv-0 projection over the 128-wide hidden layer, and the residual's
    // share of final_mlp.0 as a pre-activation addend -- `combined` [N, 1152] is never materialised
    bool fused_mlp2 = false;
    da::ConvW conv0c;                 // layer 0 under fused_mlp2 (layer_w): w = Wcat0 . W2 [4*HC0, hidden], b = Wcat0 . b2 + bcat0, din = hidden
    void *headc_w = nullptr;          // [32, hidden] act dtype = Wf0 . W2
    float *headc_b = nullptr;         // [32] = Wf0 . b2
    void *virt_qkvs = nullptr;        // exophormer: [V, 4*HC0] act dtype = virt_emb . Wcat0^T + bcat0 (constant per checkpoint)
    void *virt_qkvs_d = nullptr;      // its dense-path variant (Q pre-scaled, see ConvW)
    void *convLf_wp = nullptr;        // convLf_w packed for the row-panel kernel (see ConvW::wdp)
    // disable_folds bit 256 (DA_FOLD_LAST_QPROJ) was clear when this denoiser was created: the folded last layer of complete graphs projects Q in the prologue
    // of its attention kernel (k_attn_optt<144, true, false, .., 8192>), the projection kernel in front of it writes the K | V' columns only
    bool last_qproj = false;
    long owner_pid = 0;               // the process that created this denoiser: a forked child holds a copy of the handle but no HIP context (da_denoiser_destroy)
    void *convLf_wp_kv = nullptr;     // rows HC .. of convLf_w (K | V') packed for the row-panel kernel
    void *convLf_wq = nullptr;        // pack_w_qlast image of rows 0 .. HC - 1 (Q)
    bool attn_qsf = false;            // disable_folds bit 64 was clear when this denoiser was created: the wqs images exist, hidden layers of large complete
                                      // graphs are projected by their attention kernel (a later da_config_set changes neither)
    bool attn_x_fm = false;           // ... and disable_folds bit 128 (DA_FOLD_X_FM) was clear too: two such layers in a row hand their rows over fragment-major
    bool q_prescaled = false;
    // ... and the LAST conv's value / skip projections are folded with final_mlp.0 (its consumer, linear up to
    // the GELU): softmax(QK^T)(V Wf_h^T) == (softmax(QK^T) V) Wf_h^T per head, so the last attention runs with
    // 32-wide value heads and the [N, 1152] tensor z is never formed either (dense path only)
    bool lastfold = false;
    bool dense_only = false;     // every layer can take the block-diagonal MFMA attention: complete graphs never touch the CSR arrays
    void *convLf_w = nullptr;         // [2*HC + H*32, 256] act dtype: Wq | Wk | (Wf_h Wv_h)_h
    float *convLf_b = nullptr;        // [2*HC + H*32]
    void *skipc_w = nullptr;          // [32, 256] act dtype = Wf0 . Ws_last
    float *skipc_b = nullptr;         // [32] = Wf0 . bs_last + bf0
    std::vector<void *> owned;
    // optional per-kernel-class timing with HIP events (da_profile_*)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;      // pairs (start, stop)
    std::vector<int> prof_cls;
    size_t prof_used = 0;
    // cached sampling-loop graphs (a few distinct loops, e.g. a full loop and a remainder), oldest first.  One entry type for both caches:
    // a one-branch loop leaves `b` zero and `exec_b` null; a pair loop in split mode keeps its second branch as a graph of its own in `exec_b`
    struct LoopEntry { da::LoopKey a, b; hipGraphExec_t exec, exec_b; };
    std::vector<LoopEntry> loops;
    hipStream_t cap_stream = nullptr;     // private stream used only to RECORD graphs (the caller's
                                          // stream may be the legacy null stream, which cannot capture)
    // hybrid graphs: the virtual rows of a hidden layer (one 16-wave workgroup per row, latency-bound, 256 rows
    // for 32 puzzles) run on this side stream UNDER the masked MFMA attention of the real rows -- the two
    // kernels read the same Q / K / V and write disjoint rows.  Fork / join with events, so the pattern is
    // captured into the sampling-loop hipGraph as two parallel branches.
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // (round 6, measured: a SECOND side stream for the second branch of two Batches in flight makes configuration 3 slower -- x0.98 against
    //  x1.14 - 1.25 with this one shared; small Batches do not fork at all, see da_forward.hip: hybrid_layer)
    // da_sample_loop_pair: the second branch of the two-branch loop graph
    hipStream_t pair_stream = nullptr;
    hipEvent_t ev_pair_fork = nullptr, ev_pair_join = nullptr;
    std::vector<LoopEntry> pair_loops;
};

namespace da {

// The projection weights layer l runs with: the mlp.2-composed ones for layer 0 of a denoiser that took that fold.
inline const ConvW &layer_w(const da_denoiser *d, int l) { return (d->fused_mlp2 && l == 0) ? d->conv0c : d->conv[l]; }

struct Workspace {
    char *comb_in, *h, *combined, *qkvs, *xa, *xb, *z, *hh;
    char *hh_unc, *pz_unc, *head_pre_unc;   // discrete variant: the unconditional pass's head rows (guidance: both passes' rows feed ONE tail kernel)
    void *pz;                         // [H, n_real, 32] act dtype: per-head outputs of the folded last attention
    char *head_pre;                   // [n_real, 32] act dtype: residual share of final_mlp.0 (fused_mlp2)
    char *feat_proj;                  // [n_real, hidden] act dtype: mlp.0 over the piece-feature columns (+ bias), once per Batch
    char *feat_proj_unc;              // the same for ZERO features (= the bias, broadcast): the unconditional pass of classifier-free guidance
    char *feat_proj4;                 // DA_VARIANT_DISCRETE_ROT: the four rotated crops' feat_proj images [4][proj4_stride elements]; a step copies
    size_t proj4_stride;              // row rot_acc[piece] of them into feat_proj (k_embed_idx_time_rot)
    float *model_out_unc;
    char *dq, *dk, *dvt, *dskip;      // dense path: head-major Q, K, V ([H][n_pad][C] each), row-major skip
    size_t dense_off, dense_bytes;    // [dq, dq + dense_bytes) is zero-filled once per Batch
    unsigned *virt_cnt;               // hybrid graphs with virtual rows: arrival counters of the rows' workgroups (inside the zero-filled region) ...
    float *virt_part;                 // ... and their partial softmax states (AttnDenseParams::v_cnt / v_part)
    float *model_out, *xbuf0, *xbuf1;
    float *gcn_dinv;                  // GCN arch, CSR plans: deg^-1/2 per node (da_gcn.hip), once per Batch
    size_t total;
};

// Width of a pose row as the model returns it.  3D: quaternion wxyz | the translation head's outputs = c_in, 7 or (use_6dof: translation | a1 | a2)
// 13; the translation head is t_channels = c_in - 4 wide
inline int pose_width(const da_denoiser *d) { return d->variant == DA_VARIANT_3D ? d->c_in : d->c_out; }
inline int t_channels(const da_denoiser *d) { return d->c_in - 4; }

inline Workspace carve(const da_denoiser *d, const da_graph *g, void *base) {
    const size_t s = esize(d->prec);
    const size_t n = (size_t)g->n_nodes, nr = (size_t)g->n_real;
    const size_t nrp = nr + 64, np = n + 64;          // slack rows so tile kernels may over-read
    char *p = (char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + off : nullptr;
        off += align_up(bytes, 256);
        return q;
    };
    Workspace w;
    int hcmax = 0;
    for (int l = 0; l < d->n_layers; ++l) hcmax = d->conv[l].hc > hcmax ? d->conv[l].hc : hcmax;
    w.comb_in = take(nrp * d->D * s);
    w.h = take(nrp * d->hidden * s);
    w.feat_proj = take(nrp * d->hidden * s);
    w.feat_proj_unc = take(nrp * d->hidden * s);
    const bool rotv = d->variant == DA_VARIANT_DISCRETE_ROT;
    w.head_pre = take(nrp * (rotv ? 64 : 32) * s);
    w.pz = take(nrp * 32 * (size_t)d->heads * sizeof(float));
    w.combined = take(np * d->D * s);
    const bool gcn = d->arch == DA_ARCH_GCN;           // (the GCN reads none of the attention buffers: xa / xb / z / combined only)
    w.qkvs = take(gcn ? 0 : np * 4 * (size_t)hcmax * s);
    // (hidden layers' rows; fragment-major between two layers projected by their attention kernel, da_forward.hip: dense_layer: n_pad rows of padded slots then)
    const size_t nx = (g->dense || g->hybrid) && (size_t)g->n_pad > np ? (size_t)g->n_pad : np;
    w.xa = take(nx * 256 * s);
    w.xb = take(nx * 256 * s);
    w.z = take(np * d->D * s);
    w.hh = take(nrp * d->head_hidden * s);
    const bool disc = d->variant == DA_VARIANT_DISCRETE;
    w.hh_unc = take(disc ? nrp * d->head_hidden * s : 0);
    w.pz_unc = take(disc ? nrp * 32 * (size_t)d->heads * sizeof(float) : 0);
    w.head_pre_unc = take(disc ? nrp * 32 * s : 0);
    w.dq = w.dk = w.dvt = w.dskip = nullptr;
    w.virt_cnt = nullptr; w.virt_part = nullptr;
    w.dense_off = off;
    w.dense_bytes = 0;
    if ((g->dense || g->hybrid) && g->n_pad > 0 && !gcn) {
        const size_t hb = ((size_t)g->n_pad + 64) * hcmax * s;
        w.dq = take(hb);
        w.dk = take(hb);
        w.dvt = take(hb);
        if (g->hybrid && n > nr) w.virt_cnt = (unsigned *)take((n - nr) * sizeof(unsigned));
        w.dense_bytes = off - w.dense_off;
        if (g->hybrid && n > nr) w.virt_part = (float *)take((n - nr) * (size_t)DA_VIRT_SPLIT_MAX * 64 * 6 * sizeof(float));
        w.dskip = take(np * (size_t)hcmax * s);
    }
    const int cpose = pose_width(d);
    const size_t cbuf = cpose > 8 ? cpose : 8;
    w.model_out = (float *)take(nr * cpose * sizeof(float));
    w.model_out_unc = (float *)take(nr * cpose * sizeof(float));
    w.xbuf0 = (float *)take(nr * cbuf * sizeof(float));
    w.xbuf1 = (float *)take(nr * cbuf * sizeof(float));
    w.gcn_dinv = d->arch == DA_ARCH_GCN ? (float *)take(n * sizeof(float)) : nullptr;
    w.proj4_stride = align_up(nrp * d->hidden * s, 256) / s;
    w.feat_proj4 = take(rotv ? 4 * w.proj4_stride * s : 0);
    w.total = off;
    return w;
}

inline bool mfma_disabled() { return cfg().disable_mfma != 0; }
inline bool dense_disabled() { return cfg().disable_dense != 0; }

// The large-Batch step rule (da_config.xpanel = tail_next = -1): row-panel projections + the next step's embedding inside the tail kernel for
// Batches whose largest graph has >= 512 pieces (round 5) OR that hold >= 16 384 pieces in all (round 6: tools/ab_config.py on configuration 2,
// 512 puzzles of 144 pieces -- -6.9 % at 20-step loops, -4.0 % at 100, twelve of twelve interleaved pairs each; round 5's process-level A/B had
// read that Batch as a loss).  Small Batches (the scripted 8-puzzle ones) keep the old path: nothing to gain from a panel of nine row tiles.
inline bool step_rule_batch(const da_graph *g) { return g->max_graph_nodes >= 512 || g->n_real >= 16384; }

// Whether a graph and a head shape can take the block-diagonal matrix-core attention, under the two kill switches as given
inline bool dense_ok(const da_graph *g, int heads, int C, bool dense_off = dense_disabled(), bool mfma_off = mfma_disabled()) {
    const bool hyb = g->hybrid && g->mask && g->mask_ptr && g->irr_row_ptr;
    return !dense_off && (g->dense || hyb) && g->n_pad > 0 && g->graph_ptr && g->pad_ptr && g->row_map && heads == 8 &&
           (C == 32 || C == 144) && !mfma_off;
}

// Bracket one launch with a (start, stop) event pair on the launch stream when profiling.
template <typename F>
static int timed(da_denoiser *d, int cls, hipStream_t st, F &&launch) {
    if (!d->prof_on) return launch();
    if (d->prof_used + 2 > d->prof_ev.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t e;
            DA_CHECK_HIP(hipEventCreate(&e));
            d->prof_ev.push_back(e);
        }
    }
    hipEvent_t a = d->prof_ev[d->prof_used], b = d->prof_ev[d->prof_used + 1];
    DA_CHECK_HIP(hipEventRecord(a, st));
    int rc = launch();
    DA_CHECK_HIP(hipEventRecord(b, st));
    d->prof_used += 2;
    d->prof_cls.push_back(cls);
    return rc;
}

// The discrete variant's inputs (da_d3pm.hip): position indices where the poses were; forward_impl then stops behind final_mlp.0 and
// leaves its post-GELU rows in `hh` -- the K-wide head belongs to the tail kernel, which the caller launches.
// With the last-layer fold the rows stay one step earlier: per-head outputs `pz` of the folded attention and the pre-activation addend
// `pre` (hh = GELU(pre + sum_h pz_h), formed by the tail kernel as k_head_fold forms it); `folded` says which form this pass left.
struct DiscreteIn {
    const int32_t *idx;     // [n_real]
    char *hh;               // [n_real, 32] act dtype
    char *pz, *pre;         // [H, n_real, 32], [n_real, 32] act dtype
    int folded;             // out
    int rot = 0;            // DA_VARIANT_DISCRETE_ROT: hh is [n_real, 64], and the embedding selects the piece's feat_proj row by rot_acc
    const int32_t *rot_acc = nullptr;       // [n_real] or NULL = image 0
    D3pmRows rows() const { D3pmRows r; if (folded) { r.pz = pz; r.pre = pre; } else r.hh = hh; return r; }
};

// da_forward.hip: one forward of the denoiser over a carved workspace, enqueued on `st`
int forward_impl(da_denoiser *d, const da_graph *g, const float *x, const int64_t *t, int64_t t_scalar, float *out, float *alpha,
                 int alpha_all, float *pre_head, const Workspace &w, hipStream_t st, DdimFuse *ddim = nullptr, bool uncond = false,
                 bool h_ready = false, DiscreteIn *disc = nullptr);
// da_denoiser_create.hip: the device-side weights of a record whose scalar fields are set; on failure the caller destroys the record
int denoiser_build(da_denoiser *d, const da_weights *w, hipStream_t st);

}  // namespace da
