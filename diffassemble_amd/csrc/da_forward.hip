// One forward of the denoiser (da_denoiser_forward*, every step of the sampling loops): stages over one context.
//
// Every stage returns ONE tri-state:  0  taken -- its kernels are enqueued (a layer stage has advanced the LayerIO),
//                                    -1  not applicable, or no kernel of the route covers the shape: try the next route,
//                                   > 0  error, the message is set.
// forward_impl reads as "try this route, else the next"; its own result is 0 or an error.
#include "da_denoiser.h"

namespace da {
namespace {

// inside a route that has launched and cannot be abandoned any more, "no kernel" is an error
int must(int rc) { return rc < 0 ? 1 : rc; }

// what one layer hands to the next: its rows, their pitch, and whether they are fragment-major over the padded slots (written so by an attention
// kernel that projects its layer itself, for a reader of the same kind)
struct LayerIO {
    const void *xin;
    int ldx;
    bool x_fm;
};

// one layer's constants (FwdCtx::layer)
struct Layer {
    int l;
    const ConvW &c;             // layer_w: the mlp.2-composed weights for layer 0 of a fused denoiser
    bool last, virt0;           // virt0: fused conv 0 of the exophormer arch -- only the real rows go through the GEMM, the virtual rows' projections are
    int nproj;                  //        constants that launch_scatter_virtual places behind them (nproj: the rows that are projected)
    int act, cls;               // cls: the profile class of the layer's attention
    void *dst;
    float *al;                  // this layer's attention weights, or NULL
    const void *resid;          // last layer: the residual `feats + combined_feats` (efficient_gat.py:144) is fused in the epilogue
};

// the virtual rows' edges: aggregated (one entry per distinct source, with its multiplicity) where the plan has them, else the remainder CSR
struct VirtCsr { const int32_t *row_ptr, *col_src; const float *mult; };
VirtCsr virt_csr(const da_graph *g) {
    return g->agg_row_ptr ? VirtCsr{g->agg_row_ptr, g->agg_col_src, g->agg_mult} : VirtCsr{g->irr_row_ptr, g->irr_col_src, nullptr};
}

struct FwdCtx {
    da_denoiser *d;
    const da_graph *g;
    const Workspace &w;
    hipStream_t st;
    int prec, n, nr;
    const float *x;
    const int64_t *t;
    int64_t t_scalar;
    float *out, *alpha;         // alpha: the attention weights' request (alpha_all: of every layer, else of the last)
    int alpha_all;
    float *pre_head;
    DdimFuse *ddim;
    bool uncond, h_ready;
    DiscreteIn *disc;
    // the run-time switches, read ONCE per forward (the launchers and linear() below the stages still ask da::cfg() themselves)
    bool mfma_off, dense_off, overlap_off;
    int xpm;                    // xpanel_mode()
    bool fused;                 // d->fused_mlp2
    bool virt_scattered = false;        // the embedding's launch has placed the virtual rows' conv-0 projections (embed_mlp -> dense_layer)

    bool dense(int C) const { return dense_ok(g, d->heads, C, dense_off, mfma_off); }
    template <typename F> int timed(int cls, F &&launch) const { return da::timed(d, cls, st, launch); }
    // a QkvScatter / DenseLayout over the workspace's head-major buffers (S: the row-major skip block, or none)
    template <typename T> T head_major(void *S) const {
        T o{};
        o.Q = w.dq; o.K = w.dk; o.Vt = w.dvt; o.S = S; o.n_pad = g->n_pad;
        return o;
    }
    QkvScatter scatter(const ConvW &c, void *S) const {
        QkvScatter qs = head_major<QkvScatter>(S);
        qs.HC = c.hc; qs.C = c.C; qs.row_map = g->row_map;
        return qs;
    }
    DenseLayout layout(void *S) const {
        DenseLayout L = head_major<DenseLayout>(S);
        L.q_prescaled = d->q_prescaled;
        return L;
    }
    Layer layer(int l) const {
        const bool first = fused && l == 0, last = l == d->n_layers - 1;
        float *al = !alpha ? nullptr : (alpha_all ? alpha + (size_t)l * g->n_edges * d->heads : (last ? alpha : nullptr));
        return {l, layer_w(d, l), last, first && n > nr, first ? nr : n, (!last && d->arch == DA_ARCH_TRANSFORMER) ? DA_ACT_GELU : DA_ACT_NONE,
                last ? DA_PROF_ATTN_LAST : DA_PROF_ATTN_HIDDEN, last ? (void *)w.z : (void *)((l & 1) ? w.xb : w.xa), al,
                (last && !fused) ? w.combined : nullptr};
    }

    int embed_mlp(LayerIO &io);
    int gcn_body();
    bool layer_qsf(int l, int ldx_in) const;
    int folded_tail(const Layer &ly, const LayerIO &io);
    int folded_last_layer(const Layer &ly, const LayerIO &io);
    int conv_fused_layer(const Layer &ly, LayerIO &io);
    int hybrid_layer(const Layer &ly, LayerIO &io, const DenseLayout &L);
    int dense_layer(const Layer &ly, LayerIO &io);
    int edge_list_layer(const Layer &ly, LayerIO &io);
    int pose_head();
};

// (a-3) embedding: pose MLP + learned timestep lookup into the concat buffer, then mlp.0 and (unless folded away) mlp.2; `io` = the first layer's rows
// (h_ready: the previous step's tail kernel already wrote this step's w.h -- DdimFuse::nx_*, sampling loops only)
int FwdCtx::embed_mlp(LayerIO &io) {
    const int D = d->D;
    int rc;
    // exophormer, dense / hybrid path: the virtual rows' constant conv-0 projections are placed by extra workgroups of the embedding's launch (they
    // depend on nothing of this step; dense_layer skips its launch_scatter_virtual then)
    VirtScatter vsc;
    if (!h_ready && fused && n > nr && !alpha && w.dq && d->virt_qkvs_d && dense(d->conv[0].C) && DA_XENV("DA_VIRT_SCATTER_IN_EMBED", 1)) {
        vsc.rows = n - nr; vsc.V = d->V; vsc.H = d->heads; vsc.C = d->conv[0].C; vsc.n_real = nr; vsc.n_pad = g->n_pad;
        vsc.src = d->virt_qkvs_d; vsc.row_map = g->row_map; vsc.Q = w.dq; vsc.K = w.dk; vsc.Vt = w.dvt; vsc.S = w.dskip;
        virt_scattered = true;
    }
    if (disc) {
        disc->folded = 0;
        if ((rc = timed(DA_PROF_EMBED, [&] {
                 if (disc->rot)
                     return launch_embed_idx_time_rot(prec, nr, d->c_out, d->F, D, d->hidden, disc->idx, disc->rot_acc, t, t_scalar, d->steps, d->time_emb,
                                                      d->pos_w1, w.comb_in, w.feat_proj4, w.proj4_stride, w.feat_proj, st);
                 return launch_embed_idx_time(prec, nr, d->c_out, d->F, D, disc->idx, t, t_scalar, d->steps, d->time_emb, d->pos_w1, w.comb_in, st); }))) return rc;
    } else if (!h_ready && (rc = timed(DA_PROF_EMBED, [&] {
                   return launch_embed_pos_time(prec, nr, d->c_in, d->F, D, x, t, t_scalar, d->steps, d->time_emb,
                                                d->pos_w0, d->pos_b0, d->pos_w1, d->pos_b1, w.comb_in, st, virt_scattered ? &vsc : nullptr); }))) return rc;
    const int act1 = d->variant == DA_VARIANT_3D ? DA_ACT_LEAKY02 : DA_ACT_GELU;
    const int act2 = d->variant == DA_VARIANT_3D ? DA_ACT_LEAKY02 : DA_ACT_NONE;
    // mlp.0 over [features | pose | time]: the feature columns (F of the D inputs) do not change inside a
    // sampling loop, so their part of the product (+ bias) was computed once in da_denoiser_set_features;
    // per step only the 64 pose / timestep columns are multiplied and the cached part is added before the
    // activation (the reference recomputes the whole Linear(1152 -> 128) every step)
    if (!h_ready && (rc = timed(DA_PROF_LINEAR_MLP, [&] {
             const size_t es_ = esize(prec);
             int r2 = mfma_off ? -1
                               : launch_gemm_mfma(prec, nr, D - d->F, d->hidden, w.comb_in + (size_t)d->F * es_, D,
                                                  (const char *)d->mlp_w0 + (size_t)d->F * es_, nullptr, act1, nullptr,
                                                  w.h, d->hidden, nullptr, st, D, uncond ? w.feat_proj_unc : w.feat_proj);
             if (r2 >= 0) return r2;
             if (uncond) { set_error("unconditional pass: the hoisted mlp.0 path is not available for this shape"); return 1; }
             if (disc && disc->rot) { set_error("discrete rot: the hoisted mlp.0 path is not available for this shape"); return 1; }
             return linear(prec, nr, D, d->hidden, w.comb_in, D, d->mlp_w0, d->mlp_b0, act1, nullptr, w.h, d->hidden, st); }))) return rc;
    // mlp.2 (Linear(128 -> 1152), no activation in 2D) only feeds two linear consumers -- the conv-0 projection
    // and, through the residual, final_mlp.0 -- so for the transformer arch it is folded into their weights at
    // create time: the [N, 1152] `combined` tensor is never written, conv 0 reduces over 128 instead of 1152
    if (!fused && (rc = timed(DA_PROF_LINEAR_MLP, [&] {
             return linear(prec, nr, d->hidden, D, w.h, d->hidden, d->mlp_w1, d->mlp_b1, act2, nullptr, w.combined, D, st); }))) return rc;
    io = fused ? LayerIO{w.h, d->hidden, false} : LayerIO{w.combined, D, false};
    return 0;
}

// backbones/gcn.py:16-22, gelu(conv1(gelu(conv0(x)))), reassociated so that both aggregations run 256 wide:
// conv 0 projects first (A_hat (X W0^T)), conv 1 aggregates first ((A_hat H) W1^T); the residual `feats + combined_feats`
// (efficient_gat.py:144 / efficient_gat_3d.py:199) is added in the epilogue of conv 1's GEMM, after its GELU
int FwdCtx::gcn_body() {
    const ConvW &c0 = d->conv[0], &c1 = d->conv[1];
    const int D = d->D, hid = c0.hc;
    int rc;
    if ((rc = timed(DA_PROF_LINEAR_QKVS, [&] { return linear(prec, nr, D, hid, w.combined, D, c0.w, nullptr, DA_ACT_NONE, nullptr, w.xa, hid, st); }))) return rc;
    if ((rc = timed(DA_PROF_ATTN_HIDDEN, [&] { return launch_gcn_aggregate(prec, g, hid, w.gcn_dinv, w.xa, c0.b, DA_ACT_GELU, w.xb, st); }))) return rc;
    if ((rc = timed(DA_PROF_ATTN_LAST, [&] { return launch_gcn_aggregate(prec, g, hid, w.gcn_dinv, w.xb, nullptr, DA_ACT_NONE, w.xa, st); }))) return rc;
    return timed(DA_PROF_LINEAR_QKVS, [&] { return linear(prec, nr, hid, D, w.xa, hid, c1.w, c1.b, DA_ACT_GELU, w.combined, w.z, D, st); });
}

// Whether layer l, fed rows of length ldx_in, is projected by its own attention kernel (k_attn_res<.., 64>: no projection kernel, K | V never
// leave the CU).  ONE predicate, asked twice by dense_layer: for the layer at hand, and one layer ahead -- two such layers in a row hand their rows
// over fragment-major (LayerIO::x_fm), and the layer that writes them has to know what its reader will be.
bool FwdCtx::layer_qsf(int l, int ldx_in) const {
    if (l < 0 || l >= d->n_layers - 1 || d->arch == DA_ARCH_GCN) return false;          // (the last layer has its own kernels)
    const ConvW &c = layer_w(d, l);
    const bool virt0 = fused && l == 0 && n > nr, al = alpha && alpha_all;
    if (al || !w.dq || !dense(c.C)) return false;
#ifdef DA_EXPERIMENTS
    if (g->dense && !g->hybrid && n == nr && conv_fused_applicable(prec, d->heads, c.C, c.din, g->max_graph_nodes, c.hc)) return false;
#endif
    return !g->hybrid && !virt0 && n == nr && c.wqs && ldx_in == c.din &&
           attn_qsf_applicable(prec, d->heads, c.C, c.din, g->n_graphs, g->max_graph_nodes, g->n_pad, d->q_prescaled);
}

// behind the folded last attention: final_mlp.0's GELU, the pose head and (sampling loops) the DDIM update -- the whole tail in one kernel where it
// is covered (bf16, hidden 128, conv input 256), else in three
int FwdCtx::folded_tail(const Layer &ly, const LayerIO &io) {
    const int din = ly.c.din;
    DdimFuse *df = (ddim && d->c_out == d->c_in) ? ddim : nullptr;
    int rc, rt = -1;
    if ((rc = timed(DA_PROF_HEAD, [&] {
             rt = launch_tail_fused(prec, nr, d->heads, d->c_out, d->hidden, din, w.h, io.xin, io.ldx, d->headc_w, d->headc_b,
                                    d->skipc_w, d->skipc_b, w.pz, d->head_w1, d->head_b1, out, st, df);
             return rt > 0 ? rt : 0; }))) return rc;
    if (rt == 0) { if (df) df->done = 1; return 0; }
    // ... else: pre-activation of final_mlp.0 from the hidden layer (mlp.2 share) and from this conv's input (skip share)
    if ((rc = timed(DA_PROF_HEAD, [&] {
             return linear(prec, nr, d->hidden, 32, w.h, d->hidden, d->headc_w, d->headc_b, DA_ACT_NONE, nullptr, w.head_pre, 32, st); }))) return must(rc);
    if ((rc = timed(DA_PROF_HEAD, [&] {
             return linear(prec, nr, din, 32, io.xin, io.ldx, d->skipc_w, d->skipc_b, DA_ACT_NONE, w.head_pre, w.head_pre, 32, st); }))) return must(rc);
    if (df) df->done = 1;        // the head kernel applies the DDIM update itself
    return must(timed(DA_PROF_HEAD, [&] { return launch_head_fold(prec, nr, d->heads, d->c_out, w.pz, w.head_pre, d->head_w1, d->head_b1, out, st, df); }));
}

// The last layer with its value / skip projections folded into final_mlp.0 (da_denoiser::lastfold): Q | K | (V Wf_h^T) projection, 32-wide value heads,
// per-head outputs to pz, then the tail.  Taken, it ends the forward.
int FwdCtx::folded_last_layer(const Layer &ly, const LayerIO &io) {
    const ConvW &c = ly.c;
    if (!fused || !d->lastfold || ly.al || !w.dq || !(g->hybrid || d->V == 0) || !dense(c.C)) return -1;
    QkvScatter qs = scatter(c, nullptr);
    qs.Cv = 32;
    // complete graphs (disable_folds bit 256 clear at creation): the K | V' columns only -- Q is projected by the attention kernel, per 32-query slab,
    // in its prologue, and never exists in memory (45 % of this launch's stores, and the attention kernel's reads of them).  Hybrid graphs keep the
    // three-block launch and the masked kernel.
    const bool lq = d->last_qproj && !g->hybrid && n == nr && !io.x_fm && attn_last_qproj_applicable(prec, d->heads, c.C, c.din, g->n_pad, d->q_prescaled);
    if (lq) qs.col0 = c.hc;
    int rc = timed(DA_PROF_LINEAR_QKVS, [&] {
        if (lq)
            return launch_gemm_mfma(prec, n, c.din, c.hc + d->heads * 32, io.xin, io.ldx, (const char *)d->convLf_w + (size_t)c.hc * c.din * esize(prec),
                                    d->convLf_b + c.hc, DA_ACT_NONE, nullptr, nullptr, 0, &qs, st, 0, nullptr, d->convLf_wp_kv);
        return launch_gemm_mfma(prec, n, c.din, 2 * c.hc + d->heads * 32, io.xin, io.ldx, d->convLf_w, d->convLf_b, DA_ACT_NONE,
                                nullptr, nullptr, 0, &qs, st, 0, nullptr, d->convLf_wp); });
    DA_REQUIRE(rc >= 0 || !lq, "da_denoiser_forward: no projection kernel took the last layer's K | V' columns");
    if (rc) return rc;
    DenseLayout L = layout(nullptr);
    if (lq) { L.Q = nullptr; L.x = io.xin; L.ldx = io.ldx; L.kin = c.din; L.wqs = d->convLf_wq; L.bias = d->convLf_b; }
    DenseFold fo;
    fo.cv = 32; fo.out = disc ? (void *)disc->pz : w.pz; fo.n_rows = nr;
    // hybrid graphs: adjacency-masked, remainder edges of the real rows folded in the epilogue; the
    // virtual rows' outputs of the LAST layer are dropped by the model (exophormer_gnn.py:209), so the
    // CSR-side kernels are not needed here
    const DenseMask mk = dense_mask_of(g);
    rc = timed(DA_PROF_ATTN_LAST, [&] {
        return launch_attn_dense(prec, L, d->heads, c.C, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->pad_ptr, g->dense == 2, nullptr, DA_ACT_NONE,
                                 nullptr, st, g->hybrid ? &mk : nullptr, &fo); });
    if (rc) return rc;
    if (!disc) return folded_tail(ly, io);
    // discrete variant: the addend of final_mlp.0 (mlp.2 share + skip share); the K-wide head is the tail kernel's
    if ((rc = timed(DA_PROF_HEAD, [&] {
             return linear(prec, nr, d->hidden, 32, w.h, d->hidden, d->headc_w, d->headc_b, DA_ACT_NONE, nullptr, disc->pre, 32, st); }))) return must(rc);
    if ((rc = timed(DA_PROF_HEAD, [&] {
             return linear(prec, nr, c.din, 32, io.xin, io.ldx, d->skipc_w, d->skipc_b, DA_ACT_NONE, disc->pre, disc->pre, 32, st); }))) return must(rc);
    disc->folded = 1;
    return 0;
}

// (DA_CONV_FUSED=1: the one-kernel hidden conv, da_conv_fused.hip -- a measured tie / loss, experiments build only)
// hidden conv on complete graphs: projection + attention of a (graph, head) in ONE kernel, K / V in LDS
int FwdCtx::conv_fused_layer([[maybe_unused]] const Layer &ly, [[maybe_unused]] LayerIO &io) {
#ifdef DA_EXPERIMENTS
    const ConvW &c = ly.c;
    if (ly.al || ly.last || !g->dense || g->hybrid || n != nr || ly.resid || !dense(c.C) ||
        !conv_fused_applicable(prec, d->heads, c.C, c.din, g->max_graph_nodes, c.hc)) return -1;
    const int rc = must(timed(DA_PROF_CONV_FUSED, [&] {
        return launch_conv_fused(prec, d->heads, c.C, c.din, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->dense == 2, io.xin, io.ldx, c.w, c.b,
                                 ly.act, ly.dst, c.hc, st); }));
    if (rc == 0) io = {ly.dst, c.hc, false};
    return rc;
#else
    return -1;
#endif
}

// Hybrid graphs (sparse but heavy): masked MFMA attention over the regular edges of the real rows (partial softmax state, the remaining edges +
// normalisation + skip / activation in its epilogue), and the virtual rows over their CSR -- in one of three forms.  Q / K / V are in place: never -1.
int FwdCtx::hybrid_layer(const Layer &ly, LayerIO &io, const DenseLayout &L) {
    const ConvW &c = ly.c;
    DenseMask mk = dense_mask_of(g);
    const VirtCsr vr = virt_csr(g);
    auto real_rows = [&] {
        return launch_attn_dense(prec, L, d->heads, c.C, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->pad_ptr, 0, ly.resid, ly.act, ly.dst, st, &mk); };
    auto virt_rows = [&](hipStream_t on) {
        return launch_attn_csr_cont(prec, n, nr, vr.row_ptr, vr.col_src, g->row_map, d->heads, c.C, g->n_pad, L, ly.resid, ly.act, ly.dst, on, vr.mult); };
    int rc;
    [[maybe_unused]] const int vil = DA_XENV("DA_VIRT_IN_LAUNCH", 1);
    if (n > nr && !ly.resid && w.virt_cnt && w.virt_part && !overlap_off && vil && (g->n_real < 8192 || vil == 2)) {
        // SMALL Batches (below 8 192 pieces: the ones that do not fork a side stream below): the virtual rows inside the masked
        // attention's own launch (bf16 hidden layers: k_attn_optt<32, false, true>; da_config disable_folds bit 5 keeps the two-kernel
        // form) -- the scripted 8-puzzle Batch 0.152 -> 0.114 ms per step, 0.085 -> 0.066 / 0.052 -> 0.043 per Batch-step with two /
        // four Batches in flight.  Large Batches keep the side stream: configuration 3 measured -2 % ... +4 % with the rows in the
        // launch, depending on where in the grid they sit (profiles/r06/r06_virtual_rows_in_launch_ab*.log).
        // (experiments build: DA_VIRT_IN_LAUNCH=0 two kernels everywhere, =2 in the launch for every Batch)
        int virt_taken = 0;
        mk.v_rows = n - nr; mk.v_n_real = nr;
        mk.v_row_ptr = vr.row_ptr; mk.v_col_src = vr.col_src; mk.v_mult = vr.mult;
        mk.v_part = w.virt_part; mk.v_cnt = w.virt_cnt; mk.v_taken = &virt_taken;
        if ((rc = must(timed(ly.cls, real_rows)))) return rc;
        // (a kernel without the extra workgroups took the layer: the rows' own kernel behind it)
        if (!virt_taken && (rc = must(timed(ly.cls, [&] { return virt_rows(st); })))) return rc;
    } else if (d->side_stream && !d->prof_on && n > nr && g->n_real >= 8192) {
        // fork: virtual rows on the side stream, real rows here, join before the next projection
        // (small Batches keep the virtual rows on the caller's stream: below ~8 k pieces the fork / join costs more than the overlap
        //  buys -- the scripted 8-puzzle Batch: 0.165 -> 0.152 ms per step, profiles/r06/r06_scripted_side_stream_variants.log)
        StreamJoin side_guard;      // the error exits below still join the side stream (a capture of `st` must not be left forked)
        DA_CHECK_HIP(hipEventRecord(d->ev_fork, st));
        DA_CHECK_HIP(hipStreamWaitEvent(d->side_stream, d->ev_fork, 0));
        side_guard.arm(d->side_stream, st, d->ev_join);
        if ((rc = must(virt_rows(d->side_stream)))) return rc;
        DA_CHECK_HIP(hipEventRecord(d->ev_join, d->side_stream));
        if ((rc = must(real_rows()))) return rc;
        DA_CHECK_HIP(hipStreamWaitEvent(st, d->ev_join, 0));
        side_guard.armed = false;   // joined above: ev_join was recorded behind the rows' kernel, before the real rows' launch
    } else if ((rc = must(timed(ly.cls, [&] { const int r2 = real_rows(); return r2 ? r2 : virt_rows(st); })))) return rc;
    io = {ly.dst, c.hc, false};
    return 0;
}

// Complete and hybrid graphs at a head width with a matrix-core kernel: projection scattered into head-major Q / K / V, block-diagonal MFMA attention
int FwdCtx::dense_layer(const Layer &ly, LayerIO &io) {
    const ConvW &c = ly.c;
    if (ly.al || !w.dq || !dense(c.C)) return -1;
    const QkvScatter qs = scatter(c, w.dskip);
    const void *wpanel = (xpm == 1 || (xpm == 2 && step_rule_batch(g))) ? c.wdp : nullptr;
    // Hidden layers of large complete graphs: the resident attention kernel (k_attn_res<.., 64>) does the layer's projection in its own
    // prologue -- no projection kernel, K | V never leave the CU
    const bool qsf = !ly.resid && layer_qsf(ly.l, io.ldx);
    // ... and hands its rows to the next layer in MFMA operand order where that one is projected the same way (disable_folds bit 128 clear
    // at creation): its prologue then reads 1 KB-contiguous fragments instead of 32-byte pieces of 64 rows.  Private between the two launches;
    // the last hidden layer's rows stay row-major (the last layer's projection and the tail kernel read them)
    const bool out_fm = qsf && d->attn_x_fm && layer_qsf(ly.l + 1, c.hc);
    DA_REQUIRE(!io.x_fm || qsf, "da_denoiser_forward: layer %d was handed fragment-major rows it does not take", ly.l);
    int rc = qsf ? 0 : timed(DA_PROF_LINEAR_QKVS, [&] {
        return launch_gemm_mfma(prec, ly.nproj, c.din, 4 * c.hc, io.xin, io.ldx, c.wd, c.bd, DA_ACT_NONE, nullptr, nullptr, 0, &qs, st, 0, nullptr, wpanel); });
    if (rc) return rc;
    if (ly.virt0 && !virt_scattered &&
        (rc = launch_scatter_virtual(prec, n - nr, d->V, d->heads, c.C, d->virt_qkvs_d, nr, g->row_map, g->n_pad, w.dq, w.dk, w.dvt, w.dskip, nullptr, st))) return must(rc);
    DenseLayout L = layout(w.dskip);
    if (qsf) { L.x = io.xin; L.ldx = io.ldx; L.kin = c.din; L.wqs = c.wqs; L.bias = c.bd; L.x_fm = io.x_fm; L.out_fm = out_fm; }
    if (g->hybrid) return hybrid_layer(ly, io, L);
    // (a layer projected by its attention kernel is ONE kernel: priced as such, projection + attention FLOP, Q | K | V | skip never in HBM)
    rc = timed(qsf ? DA_PROF_CONV_FUSED : ly.cls, [&] {
        return launch_attn_dense(prec, L, d->heads, c.C, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->pad_ptr, g->dense == 2, ly.resid, ly.act, ly.dst, st); });
    if (rc == 0) io = {ly.dst, c.hc, out_fm};
    return rc;
}

// Every other layer: row-major Q | K | V | skip, one walk of the edge list per destination (the only route that yields attention weights).  The last
// route: never -1.
int FwdCtx::edge_list_layer(const Layer &ly, LayerIO &io) {
    const ConvW &c = ly.c;
    int rc;
    DA_REQUIRE(!io.x_fm, "da_denoiser_forward: layer %d was handed fragment-major rows it does not take", ly.l);
    if ((rc = timed(DA_PROF_LINEAR_QKVS, [&] {
             return linear(prec, ly.nproj, c.din, 4 * c.hc, io.xin, io.ldx, c.w, c.b, DA_ACT_NONE, nullptr, w.qkvs, 4 * c.hc, st); }))) return must(rc);
    if (ly.virt0 && (rc = launch_scatter_virtual(prec, n - nr, d->V, d->heads, c.C, d->virt_qkvs, nr, nullptr, 0, nullptr, nullptr,
                                                 nullptr, nullptr, w.qkvs, st))) return must(rc);
    DA_REQUIRE(g->row_ptr && (g->col_src || g->n_edges == 0), "da_graph: this call walks the edge list (alpha requested or no "
               "MFMA attention for this layer) but the CSR arrays are missing");
    // tiny complete graphs at a head width without a matrix-core kernel (the 3D variant: 20-fragment objects, C = 104): one workgroup per graph
    // with the graph's K | V rows in LDS instead of one walk of the edge list per destination
    int tiny = -1;
    if (!ly.al && g->dense && n == nr && g->graph_ptr && !dense_off) {
        if ((rc = timed(ly.cls, [&] {
                 tiny = launch_attn_tiny(prec, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->dense == 2, d->heads, c.C, w.qkvs, ly.resid, ly.act, ly.dst, st);
                 return tiny > 0 ? tiny : 0; }))) return rc;
    }
    if (tiny != 0 && (rc = timed(ly.cls, [&] {
             return launch_attn_csr(prec, n, g->row_ptr, g->col_src, g->edge_id, d->heads, c.C, w.qkvs, ly.resid, ly.act, ly.dst, ly.al, nullptr, st); }))) return must(rc);
    io = {ly.dst, c.hc, false};
    return 0;
}

// (a-7 / a-13) pose head over the last layer's rows in w.z
int FwdCtx::pose_head() {
    const int D = d->D;
    char *const hh = disc ? disc->hh : w.hh;
    int rc;
    if (fused) {
        // final_mlp.0(conv_out + combined) = Wf . conv_out + (Wf W2) . h + (Wf b2 + bf): the second term first
        // (hw: 32 rows of final_mlp.0; the discrete rot variant runs final_mlp.0 | final_mlp_rot.0 as one 64-wide product, as the 3D heads do)
        const int hw = d->variant == DA_VARIANT_DISCRETE_ROT ? 64 : 32;
        if ((rc = timed(DA_PROF_HEAD, [&] {
                 return linear(prec, nr, d->hidden, hw, w.h, d->hidden, d->headc_w, d->headc_b, DA_ACT_NONE, nullptr, w.head_pre, hw, st); }))) return rc;
        rc = timed(DA_PROF_HEAD, [&] {
            return launch_gemm_mfma(prec, nr, D, d->head_hidden, w.z, D, d->head_w0, d->head_b0, DA_ACT_GELU, nullptr, hh, d->head_hidden, nullptr, st, D, w.head_pre); });
        if (rc > 0) return rc;
        DA_REQUIRE(rc == 0, "fused head GEMM: shape not supported");
    } else if ((rc = timed(DA_PROF_HEAD, [&] {
                    return linear(prec, nr, D, d->head_hidden, w.z, D, d->head_w0, d->head_b0, DA_ACT_GELU, nullptr, hh, d->head_hidden, st); }))) return rc;
    if (disc) return 0;
    return timed(DA_PROF_HEAD, [&] {
        if (d->variant == DA_VARIANT_3D)
            return launch_head3d(prec, nr, t_channels(d), hh, d->head_w1, d->head_b1, d->head_r_w1, d->head_r_b1, out, pre_head, st);
        return launch_head2d(prec, nr, d->c_out, hh, d->head_w1, d->head_b1, out, st);
    });
}

}  // namespace

int forward_impl(da_denoiser *d, const da_graph *g, const float *x, const int64_t *t, int64_t t_scalar, float *out, float *alpha, int alpha_all,
                 float *pre_head, const Workspace &w, hipStream_t st, DdimFuse *ddim, bool uncond, bool h_ready, DiscreteIn *disc) {
    FwdCtx f{d, g, w, st, d->prec, g->n_nodes, g->n_real, x, t, t_scalar, out, alpha, alpha_all, pre_head, ddim, uncond, h_ready, disc,
             mfma_disabled(), dense_disabled(), (cfg().disable_folds & DA_FOLD_HYBRID_OVERLAP) != 0, xpanel_mode(), d->fused_mlp2};
    LayerIO io;
    int rc = f.embed_mlp(io);
    if (rc) return rc;
    if (d->arch == DA_ARCH_GCN) return (rc = f.gcn_body()) ? rc : f.pose_head();
    // (a-4..a-6) graph transformer: fused Q|K|V|skip projection + attention per layer
    // use_6dof (3D, c_in = 13): what the forward returns does not depend on whether attention weights are asked for, so the per-step
    // sampling route (return_attentions) and the captured loop give the same bits.  Only the edge-list kernels produce the weights: a layer
    // whose weights are wanted walks the edge list for them first -- its rows land in the layer's own destination and are overwritten --
    // and then runs exactly as it does without the request.  (The other models keep their one pass: their outputs stay what they were.)
    const bool alpha_apart = d->variant == DA_VARIANT_3D && d->c_in == 13;
    for (int l = 0; l < d->n_layers; ++l) {
        Layer ly = f.layer(l);
        if (alpha_apart && ly.al) {
            LayerIO unused = io;
            if ((rc = f.edge_list_layer(ly, unused))) return rc;
            ly.al = nullptr;
        }
        if (ly.last && (rc = f.folded_last_layer(ly, io)) >= 0) return rc;         // taken: it ran the head behind the layer too
        if ((rc = f.conv_fused_layer(ly, io)) < 0 && (rc = f.dense_layer(ly, io)) < 0) rc = f.edge_list_layer(ly, io);
        if (rc) return rc;
    }
    return f.pose_head();
}

}  // namespace da
