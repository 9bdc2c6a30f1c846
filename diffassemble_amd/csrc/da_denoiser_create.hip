// The device-side weights of a denoiser (da_denoiser_create): the caller's fp32 tensors packed in the activation dtype, the projections'
// dense-path images, and the weights composed once per checkpoint (mlp.2 fold, last-layer fold).  Everything is enqueued on one stream, in
// one fixed order: the composed weights are fp32 products, and their bits depend on nothing else.
#include "da_denoiser.h"

namespace da {

// p[r][c] *= s for r < rows, c < cols (row pitch ld): scales the Q block of a packed projection in fp32
__global__ void k_scale_block(float *p, int rows, int cols, int ld, float s) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * cols) p[(i / cols) * ld + (i % cols)] *= s;
}
static int scale_block(float *p, int rows, int cols, int ld, float s, hipStream_t st) {
    const size_t n = (size_t)rows * cols;
    if (!n) return 0;
    k_scale_block<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p, rows, cols, ld, s);
    DA_LAUNCH_CHECK();
    return 0;
}
static bool q_prescale_on() { return !(cfg().disable_folds & DA_FOLD_QSCALE); }
static float q_scale_log2(int C) { return 1.4426950408889634f / sqrtf((float)C); }

namespace {

// One device step of the builder: skipped once a step has failed, a failure is code 2.
#define DA_STEP(expr) do { if (!rc && (expr)) rc = 2; } while (0)

struct Builder {
    da_denoiser *const d;
    const da_weights *const w;
    const hipStream_t st;
    const int prec, D, H;
    const size_t s;
    const bool rotv, discrete;
    float *hw0 = nullptr;       // discrete rot: the two first head layers stacked, fp32 (heads -> fold_mlp2)
    int rc = 0;                 // sticky: the first failure (1 = a missing tensor, 2 = the device); every later step is skipped

    Builder(da_denoiser *d_, const da_weights *w_, hipStream_t st_)
        : d(d_), w(w_), st(st_), prec(d_->prec), D(d_->D), H(d_->heads), s(esize(d_->prec)), rotv(d_->variant == DA_VARIANT_DISCRETE_ROT),
          discrete(d_->variant == DA_VARIANT_DISCRETE || d_->variant == DA_VARIANT_DISCRETE_ROT) {}

    void *alloc(size_t bytes) {
        void *p = nullptr;
        if (rc) return nullptr;
        if (hipMalloc(&p, bytes < 256 ? 256 : bytes) != hipSuccess) { set_error("hipMalloc(%zu) failed", bytes); rc = 2; return nullptr; }
        d->owned.push_back(p);
        return p;
    }
    float *alloc_f32(size_t n) { return (float *)alloc(n * 4); }
    void missing(bool absent, const char *fmt, int l = 0) { if (!rc && absent) { set_error(fmt, l); rc = 1; } }
    void copy_into(void *dst, const void *src, size_t bytes) { DA_STEP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess); }
    float *copy_f32(const float *src, size_t n) {
        float *p = alloc_f32(n);
        copy_into(p, src, n * 4);
        return rc ? nullptr : p;
    }
    void *pack(const float *src, size_t n) {
        void *p = alloc(n * s + 4096);       // slack: tile kernels may over-read a partial tile
        DA_STEP(launch_convert(prec, n, src, p, st));
        return rc ? nullptr : p;
    }
    // per-head Q / skip fragments of a hidden layer's dense-path projection (bf16, 32-wide heads, K = 128 / 256); nullptr otherwise
    void *pack_qs(const void *wsrc, int K, int hc, int C) {
        if (!d->attn_qsf || prec != DA_PREC_BF16 || C != 32 || H != 8 || (K != 128 && K != 256) || !wsrc || mfma_disabled()) return nullptr;
        void *p = alloc(w_qs_bytes(H, K));
        DA_STEP(pack_w_qs(H, K, hc, wsrc, p, st));
        return rc ? nullptr : p;
    }
    // fragment-major copy of a projection weight for the row-panel kernel; nullptr when the shape has no packed form
    void *pack_panel(const void *wsrc, int K, int Nout) {
        const size_t nb = xpanel_in_model() ? da_linear_packed_bytes(prec, K, Nout) : 0;
        if (!nb || !wsrc) return nullptr;
        void *p = alloc(nb);
        DA_STEP(pack_w_xpanel(K, Nout, wsrc, K, p, st));
        return rc ? nullptr : p;
    }
    // The dense-path image of a projection (ConvW::wd): the Q block of the fp32 matrix `wf` (q_rows x q_cols, row pitch ld) and, where given, the
    // Q entries of its bias are scaled by log2(e) / sqrt(C) IN PLACE, in fp32; then all n elements are packed -- into `dst`, or a new allocation.
    void *pack_q_scaled(float *wf, int q_rows, int q_cols, int ld, size_t n, int C, float *q_bias = nullptr, void *dst = nullptr) {
        DA_STEP(scale_block(wf, q_rows, q_cols, ld, q_scale_log2(C), st));
        if (q_bias) scale_q_bias(q_bias, q_rows, C);
        if (!dst) return pack(wf, n);
        DA_STEP(launch_convert(prec, n, wf, dst, st));
        return rc ? nullptr : dst;
    }
    void scale_q_bias(float *b, int hc, int C) { DA_STEP(scale_block(b, 1, hc, hc, q_scale_log2(C), st)); }

    void embed_mlp() {
        d->time_emb = copy_f32(w->time_emb, (size_t)w->steps * 32);
        if (discrete) {
            d->pos_w1 = copy_f32(w->pos_w1, (size_t)w->c_out * 32);        // pos_mlp.weight [K, 32]; pos_w0 / pos_b0 / pos_b1 are not read
        } else {
            d->pos_w0 = copy_f32(w->pos_w0, 16 * (size_t)w->c_in); d->pos_b0 = copy_f32(w->pos_b0, 16);
            d->pos_w1 = copy_f32(w->pos_w1, 32 * 16); d->pos_b1 = copy_f32(w->pos_b1, 32);
        }
        d->mlp_w0 = pack(w->mlp_w0, (size_t)d->hidden * D); d->mlp_b0 = copy_f32(w->mlp_b0, d->hidden);
        d->mlp_w1 = pack(w->mlp_w1, (size_t)D * d->hidden); d->mlp_b1 = copy_f32(w->mlp_b1, D);
    }

    // GCNConv(D, 256), GCNConv(256, D) (gcn.py:9-14): lin.weight [out, in] packed in the act dtype (no bias in lin), bias fp32
    void gcn_convs() {
        for (int l = 0; l < 2; ++l) {
            ConvW &c = d->conv[l];
            c.din = l == 0 ? D : 256;
            c.hc = l == 0 ? 256 : D;
            missing(!w->conv_wq[l] || !w->conv_bq[l], "gcn conv %d: missing weight pointer", l);
            c.w = pack(w->conv_wq[l], (size_t)c.hc * c.din);
            c.b = copy_f32(w->conv_bq[l], c.hc);
            c.wd = c.w; c.bd = c.b;
        }
    }

    // TransformerConv layers: Q | K | V | skip as one [4*HC, Din] projection, its dense-path image and that image's two packed forms
    void attn_convs() {
        for (int l = 0; l < d->n_layers; ++l) {
            ConvW &c = d->conv[l];
            c.din = l == 0 ? D : 32 * H;
            c.C = l == d->n_layers - 1 ? D / H : 32;
            c.hc = c.C * H;
            const size_t blk = (size_t)c.hc * c.din;
            char *wp = (char *)alloc(4 * blk * s + 4096);
            c.b = alloc_f32(4 * (size_t)c.hc);
            c.w = wp;
            const float *ws[4] = {w->conv_wq[l], w->conv_wk[l], w->conv_wv[l], w->conv_ws[l]};
            const float *bs[4] = {w->conv_bq[l], w->conv_bk[l], w->conv_bv[l], w->conv_bs[l]};
            for (int k = 0; k < 4; ++k) missing(!ws[k] || !bs[k], "conv %d: missing weight pointer", l);
            if (rc) return;
            for (int k = 0; k < 4; ++k) {
                DA_STEP(launch_convert(prec, blk, ws[k], wp + k * blk * s, st));
                copy_into(c.b + (size_t)k * c.hc, bs[k], (size_t)c.hc * 4);
            }
            c.wd = c.w; c.bd = c.b;
            if (q_prescale_on()) {
                char *wd = (char *)alloc(4 * blk * s + 4096);
                float *tq = copy_f32(ws[0], blk);
                if (rc) return;
                c.wd = pack_q_scaled(tq, c.hc, c.din, c.din, blk, c.C, nullptr, wd);
                copy_into(wd + blk * s, wp + blk * s, 3 * blk * s);
                c.bd = copy_f32(c.b, 4 * (size_t)c.hc);
                scale_q_bias(c.bd, c.hc, c.C);
            }
            c.wdp = pack_panel(c.wd, c.din, 4 * c.hc);
            if (l < d->n_layers - 1) c.wqs = pack_qs(c.wd, c.din, c.hc, c.C);
        }
    }

    // two fp32 matrices of `rows` rows each stacked into one packed [2 * rows, D] weight, their biases into one fp32 vector (3D: mlp_t.0 | mlp_r.0;
    // discrete rot: final_mlp.0 | final_mlp_rot.0 -- that one keeps the fp32 stack too, it feeds the mlp.2 fold)
    void stacked_head0(int rows) {
        d->head_b0 = alloc_f32(2 * (size_t)rows);
        if (rotv) {
            hw0 = alloc_f32(2 * (size_t)rows * D);
            if (rc) return;
            copy_into(hw0, w->head_w0, (size_t)rows * D * 4);
            copy_into(hw0 + (size_t)rows * D, w->head_r_w0, (size_t)rows * D * 4);
        } else {
            char *hp = (char *)alloc(2 * (size_t)rows * D * s + 4096);
            if (rc) return;
            d->head_w0 = hp;
            DA_STEP(launch_convert(prec, (size_t)rows * D, w->head_w0, hp, st));
            DA_STEP(launch_convert(prec, (size_t)rows * D, w->head_r_w0, hp + (size_t)rows * D * s, st));
        }
        copy_into(d->head_b0, w->head_b0, (size_t)rows * 4);
        copy_into(d->head_b0 + rows, w->head_r_b0, (size_t)rows * 4);
        if (rotv) d->head_w0 = pack(hw0, 2 * (size_t)rows * D);
    }
    void heads() {
        if (d->variant == DA_VARIANT_3D) {
            stacked_head0(256);
            const size_t tch = (size_t)t_channels(d);          // mlp_t.2: 3 rows, or 9 with use_6dof
            d->head_w1 = copy_f32(w->head_w1, tch * 256); d->head_b1 = copy_f32(w->head_b1, tch);
            d->head_r_w1 = copy_f32(w->head_r_w1, 3 * 256); d->head_r_b1 = copy_f32(w->head_r_b1, 3);
        } else if (rotv) {
            stacked_head0(32);
            d->head_w1 = copy_f32(w->head_w1, (size_t)w->c_out * 32); d->head_b1 = copy_f32(w->head_b1, w->c_out);
            d->head_r_w1 = copy_f32(w->head_r_w1, 4 * 32); d->head_r_b1 = copy_f32(w->head_r_b1, 4);
        } else {
            d->head_w0 = pack(w->head_w0, 32 * (size_t)D); d->head_b0 = copy_f32(w->head_b0, 32);
            d->head_w1 = copy_f32(w->head_w1, (size_t)w->c_out * 32); d->head_b1 = copy_f32(w->head_b1, w->c_out);
        }
    }

    // mlp.2 composed into its two consumers, in fp32 from the caller's fp32 weights, then packed (da_denoiser::conv0c / headc_*); behind it the last-layer fold
    // (the discrete variant shares the body between the embedding and final_mlp.0, so it takes both folds; its K-wide head is the tail
    //  kernel of da_d3pm.hip, which forms GELU(pre + sum_h pz_h) itself -- k_head_fold / k_tail_fused write at most 8 pose channels)
    void fold_mlp2() {
        if ((cfg().disable_folds & DA_FOLD_MLP2) || mfma_disabled() || !(d->variant == DA_VARIANT_2D || discrete) || d->hidden % 32 != 0 ||
            d->arch == DA_ARCH_GCN) return;
        const int hid = d->hidden, hc0 = d->conv[0].hc, C0 = d->conv[0].C;
        ConvW &c = d->conv0c;
        c.din = hid; c.hc = hc0; c.C = C0;
        float *w2t = alloc_f32((size_t)hid * D);                   // W2^T [hidden, D]
        float *cw = alloc_f32((size_t)4 * hc0 * hid);              // Wcat0 . W2
        const int hwn = rotv ? 64 : 32;                            // rows of the (stacked) first head layer
        const float *hsrc = rotv ? hw0 : w->head_w0;
        float *hw = alloc_f32((size_t)hwn * hid);                  // Wf0 . W2
        c.b = alloc_f32((size_t)4 * hc0);
        d->headc_b = alloc_f32(hwn);
        DA_STEP(launch_transpose_f32(D, hid, w->mlp_w1, w2t, st));
        const float *ws[4] = {w->conv_wq[0], w->conv_wk[0], w->conv_wv[0], w->conv_ws[0]};
        const float *bs[4] = {w->conv_bq[0], w->conv_bk[0], w->conv_bv[0], w->conv_bs[0]};
        for (int k = 0; k < 4; ++k) {
            // rows of block k: [hc0, D] . W2 [D, hid]  ==  A [hc0, D] @ (W2^T [hid, D])^T
            DA_STEP(launch_gemm_simple(DA_PREC_F32, hc0, D, hid, ws[k], D, w2t, nullptr, DA_ACT_NONE, nullptr, cw + (size_t)k * hc0 * hid, hid, st));
            // bias: b2 [1, D] @ (W_k [hc0, D])^T + b_k
            DA_STEP(launch_gemm_simple(DA_PREC_F32, 1, D, hc0, w->mlp_b1, D, ws[k], bs[k], DA_ACT_NONE, nullptr, c.b + (size_t)k * hc0, hc0, st));
        }
        DA_STEP(launch_gemm_simple(DA_PREC_F32, hwn, D, hid, hsrc, D, w2t, nullptr, DA_ACT_NONE, nullptr, hw, hid, st));
        DA_STEP(launch_gemm_simple(DA_PREC_F32, 1, D, hwn, w->mlp_b1, D, hsrc, nullptr, DA_ACT_NONE, nullptr, d->headc_b, hwn, st));
        c.w = pack(cw, (size_t)4 * hc0 * hid);
        d->headc_w = pack(hw, (size_t)hwn * hid);
        c.wd = c.w; c.bd = c.b;
        if (d->q_prescaled) {          // (cw is not used afterwards)
            c.bd = copy_f32(c.b, (size_t)4 * hc0);
            scale_q_bias(c.bd, hc0, C0);
            c.wd = pack_q_scaled(cw, hc0, hid, hid, (size_t)4 * hc0 * hid, C0);
        }
        c.wdp = pack_panel(c.wd, hid, 4 * hc0);
        if (d->n_layers > 1) c.wqs = pack_qs(c.wd, hid, hc0, C0);
        if (d->V > 0) {            // exophormer: conv-0 projections of the virtual rows (they bypass mlp)
            float *vq = alloc_f32((size_t)d->V * 4 * hc0);
            for (int k = 0; k < 4; ++k)
                DA_STEP(launch_gemm_simple(DA_PREC_F32, d->V, D, hc0, w->virt_emb, D, ws[k], bs[k], DA_ACT_NONE, nullptr, vq + (size_t)k * hc0, 4 * hc0, st));
            d->virt_qkvs = pack(vq, (size_t)d->V * 4 * hc0);
            d->virt_qkvs_d = d->q_prescaled ? pack_q_scaled(vq, d->V, hc0, 4 * hc0, (size_t)d->V * 4 * hc0, C0) : d->virt_qkvs;
        }
        if (rc) return;
        d->fused_mlp2 = true;
        fold_last();
    }

    // last conv: value heads and skip folded with final_mlp.0 (da_denoiser::convLf_* / skipc_*)
    // (the discrete rot variant does not take this fold: both folded attention kernels exist for 32 value channels only, and its
    //  stacked head has 64 -- it runs the last layer that disable_folds = 2 selects for the position model)
    void fold_last() {
        const int L = d->n_layers - 1, hcL = d->conv[L].hc, CL = d->conv[L].C, dinL = d->conv[L].din;
        if ((cfg().disable_folds & DA_FOLD_LAST) || rotv || CL != 144 || hcL != D || dinL % 32 != 0 || !(d->c_out <= 8 || discrete)) return;   // (k_head_fold: 8 outputs per row at most)
        const int nf = 2 * hcL + H * 32;
        float *lw = alloc_f32((size_t)nf * dinL);
        float *sw = alloc_f32((size_t)32 * dinL);
        d->convLf_b = alloc_f32(nf);
        d->skipc_b = alloc_f32(32);
        if (rc) return;
        const size_t blk = (size_t)hcL * dinL;
        copy_into(lw, w->conv_wq[L], blk * 4);
        copy_into(lw + blk, w->conv_wk[L], blk * 4);
        copy_into(d->convLf_b, w->conv_bq[L], (size_t)hcL * 4);
        copy_into(d->convLf_b + hcL, w->conv_bk[L], (size_t)hcL * 4);
        for (int h = 0; h < H; ++h) {
            // (Wf[:, hC:(h+1)C] [32, C]) . (Wv[hC:(h+1)C, :] [C, din]) and the same block of the bias
            DA_STEP(launch_mm_nn_f32(32, dinL, CL, w->head_w0 + (size_t)h * CL, D, w->conv_wv[L] + (size_t)h * CL * dinL, dinL, nullptr,
                                     lw + 2 * blk + (size_t)h * 32 * dinL, dinL, st));
            DA_STEP(launch_mm_nn_f32(32, 1, CL, w->head_w0 + (size_t)h * CL, D, w->conv_bv[L] + (size_t)h * CL, 1, nullptr,
                                     d->convLf_b + 2 * hcL + h * 32, 1, st));
        }
        // skip: Wf [32, D] . Ws [D, din];  bias: Wf . bs + bf0
        DA_STEP(launch_mm_nn_f32(32, dinL, D, w->head_w0, D, w->conv_ws[L], dinL, nullptr, sw, dinL, st));
        DA_STEP(launch_mm_nn_f32(32, 1, D, w->head_w0, D, w->conv_bs[L], 1, w->head_b0, d->skipc_b, 1, st));
        // (this projection only ever feeds the matrix-core attention)
        d->convLf_w = d->q_prescaled ? pack_q_scaled(lw, hcL, dinL, dinL, (size_t)nf * dinL, CL, d->convLf_b) : pack(lw, (size_t)nf * dinL);
        d->convLf_wp = pack_panel(d->convLf_w, dinL, nf);
        d->last_qproj = attn_last_qproj_enabled() && prec == DA_PREC_BF16 && H == 8 && dinL == 256 && d->q_prescaled && d->convLf_w && !mfma_disabled();
        if (d->last_qproj) {
            d->convLf_wp_kv = pack_panel((const char *)d->convLf_w + blk * s, dinL, nf - hcL);
            d->convLf_wq = alloc(w_qlast_bytes(H, CL, dinL));
            DA_STEP(pack_w_qlast(H, CL, dinL, d->convLf_w, d->convLf_wq, st));
        }
        d->skipc_w = pack(sw, (size_t)32 * dinL);
        d->lastfold = rc == 0;
    }

    // side stream of the hybrid path (see the struct); da_config.disable_folds bit 32 keeps everything on one stream
    void side_stream() {
        if (rc || d->V <= 0 || (cfg().disable_folds & DA_FOLD_HYBRID_OVERLAP)) return;
        if (hipStreamCreateWithFlags(&d->side_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming) != hipSuccess) {
            set_error("da_denoiser_create: side stream / events");
            rc = 2;
        }
    }
};
#undef DA_STEP

}  // namespace

int denoiser_build(da_denoiser *d, const da_weights *w, hipStream_t st) {
    Builder b(d, w, st);
    d->attn_qsf = attn_qsf_enabled();
    d->attn_x_fm = d->attn_qsf && !(cfg().disable_folds & DA_FOLD_X_FM);
    b.embed_mlp();
    if (d->arch == DA_ARCH_GCN) b.gcn_convs(); else b.attn_convs();
    d->q_prescaled = q_prescale_on();
    if (d->V > 0) {
        b.missing(!w->virt_emb, "exophormer: virt_emb missing");
        d->virt_emb = b.pack(w->virt_emb, (size_t)d->V * d->D);
    }
    b.heads();
    b.fold_mlp2();
    if (!b.rc && hipStreamSynchronize(st) != hipSuccess) { set_error("da_denoiser_create: sync failed"); b.rc = 2; }
    b.side_stream();
    d->dense_only = d->heads == 8 && !dense_disabled() && !mfma_disabled();
    for (int l = 0; l < d->n_layers; ++l) d->dense_only = d->dense_only && (d->conv[l].C == 32 || d->conv[l].C == 144);
    if (d->arch == DA_ARCH_GCN) d->dense_only = true;     // complete / banded plans aggregate in closed form (da_gcn.hip): no CSR
    return b.rc;
}

}  // namespace da
