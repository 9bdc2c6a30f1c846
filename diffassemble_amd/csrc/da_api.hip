// C-ABI entry points of libdiffassemble_hip.so (include/diffassemble_hip.h), and the recording and caching of the loops' graphs.
// The denoiser's record is da_denoiser.h; its weights are built in da_denoiser_create.hip, one forward is da_forward.hip.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <utility>

#include "da_denoiser.h"

namespace da {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// dst[r][c] = bias[c] in the activation dtype (the feature share of mlp.0 for zero features)
__global__ void k_fill_bias_rows(int prec, int rows, int cols, const float *bias, void *dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * cols) return;
    const float v = bias[i % cols];
    if (prec == DA_PREC_BF16) ((bf16_t *)dst)[i] = f2bf(v); else ((float *)dst)[i] = v;
}
// classifier-free guidance, spatial_diffusion.py:585-589: out = (1 + w) cond - w unc, in place on `cond`
__global__ void k_cfg_combine(size_t n, float wgt, float *cond, const float *unc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cond[i] = (1.0f + wgt) * cond[i] - wgt * unc[i];
}

int linear(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias, int act,
           const void *res, void *out, int ldo, hipStream_t st) {
    if (!mfma_disabled()) {
        const int rc = launch_gemm_mfma(prec, M, K, Nout, A, lda, W, bias, act, res, out, ldo, nullptr, st);
        if (rc >= 0) return rc;
    }
    return launch_gemm_simple(prec == DA_PREC_F32_BF16MMA ? DA_PREC_F32 : prec, M, K, Nout, A, lda, W, bias, act, res, out, ldo, st);
}

static bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

static int check_graph(const da_denoiser *d, const da_graph *g) {
    DA_REQUIRE(g && g->n_real > 0 && g->n_nodes >= g->n_real, "da_graph: bad node counts");
    // complete graphs (dense != 0) on a denoiser whose every layer has an MFMA attention kernel never walk the
    // edge list; the host may then leave the CSR arrays out (da_denoiser_flags bit 2) unless alpha is wanted
    const bool hyb = g->hybrid && g->mask && g->mask_ptr && g->irr_row_ptr;
    if (!((g->dense || hyb) && d->dense_only)) DA_REQUIRE(g->row_ptr && (g->col_src || g->n_edges == 0), "da_graph: CSR arrays missing");
    DA_REQUIRE(d->V == 0 || g->n_nodes == g->n_real + d->V * g->n_graphs,
               "da_graph: exophormer expects n_nodes = n_real + V*G (%d vs %d + %d*%d)", g->n_nodes, g->n_real,
               d->V, g->n_graphs);
    return 0;
}

}  // namespace da

using namespace da;

// one wave that waits `ticks` of the 100 MHz real-time counter (phase-offset experiment of the two-branch loop)
__global__ void k_pair_delay(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ---------------------------------------------------------------------------------------- recording and caching the loops' graphs
//  Every loop entry point validates its arguments, builds a LoopKey, and either replays the cached graph of that key or
// records one: record_graph is the only place that captures, loop_key the only place that builds a key, cache_find / cache_insert the
// only cache policy, and every fork of a library-owned stream sits under a StreamJoin.

static int loop_iters(const da_schedule *s, int ratio, int max_iters) {
    const int total = (s->steps + ratio - 1) / ratio;
    return (max_iters > 0 && max_iters < total) ? max_iters : total;
}

// the caller's da_loop_opts (NULL = the plain DDIM loop) copied field by field into a zeroed struct -- it becomes part of a LoopKey -- and checked
static int loop_opts(const char *who, const da_denoiser *d, const da_loop_opts *opts, da_loop_opts *o) {
    memset(o, 0, sizeof(*o));
    if (opts) { o->sampler = opts->sampler; o->eta = opts->eta; o->cfg = opts->cfg; o->cfg_w = opts->cfg_w; o->noise = opts->noise; }
    DA_REQUIRE(o->sampler == 0 || o->sampler == 1, "%s: sampler must be 0 (DDIM) or 1 (DDPM)", who);
    DA_REQUIRE(!(o->sampler == 1 || o->eta > 0.f) || o->noise, "%s: eta > 0 / DDPM need the noise buffer", who);
    DA_REQUIRE(d->variant == DA_VARIANT_2D || (!o->cfg && o->sampler == 0 && o->eta == 0.f), "%s: the 3D loop has no guidance / stochastic variant", who);
    return 0;
}

// Everything a recorded graph has baked in.  memset, then assign: keys are compared with memcmp, padding included.
static LoopKey loop_key(const da_graph *g, const da_schedule *s, int mean_type, int ratio, int n_iters, const void *x_init, void *traj,
                        void *x_final, void *ws, size_t ws_bytes, const da_loop_opts &o, size_t traj_stride = 0, size_t noise_stride = 0,
                        const void *seed = nullptr) {
    LoopKey k;
    memset(&k, 0, sizeof(k));
    k.g = *g; k.s = *s; k.mean_type = mean_type; k.ratio = ratio; k.max_iters = n_iters;
    k.x_init = (const float *)x_init; k.traj = (float *)traj; k.x_final = (float *)x_final; k.ws = ws; k.ws_bytes = ws_bytes;
    k.opts = o; k.traj_stride = traj ? traj_stride : 0; k.noise_stride = o.noise ? noise_stride : 0;
    k.cfg = cfg(); k.seed = seed;
    return k;
}
static const LoopKey no_key = {};           // the `b` of a one-branch entry (static storage: zero, padding included)

// two_graphs: a pair entry matches only in the form (da_config.pair_split) it was recorded in
static const da_denoiser::LoopEntry *cache_find(const std::vector<da_denoiser::LoopEntry> &c, const LoopKey &a, const LoopKey &b, bool two_graphs) {
    const da_denoiser::LoopEntry *hit = nullptr;
    for (const auto &e : c)
        if (memcmp(&a, &e.a, sizeof(a)) == 0 && memcmp(&b, &e.b, sizeof(b)) == 0 && (e.exec_b != nullptr) == two_graphs) hit = &e;
    return hit;
}
// small LRU-less caches: a full one drops its oldest entry
static void cache_insert(std::vector<da_denoiser::LoopEntry> &c, size_t capacity, const da_denoiser::LoopEntry &e) {
    if (c.size() >= capacity) {
        (void)hipGraphExecDestroy(c.front().exec);
        if (c.front().exec_b) (void)hipGraphExecDestroy(c.front().exec_b);
        c.erase(c.begin());
    }
    c.push_back(e);
}

// enqueue(cs) -> 0 recorded on the library's capture stream into *out.  The capture is ended and the hipGraph_t destroyed on every path; a
// non-zero rc of the callback comes back unchanged (its message stands), a capture / instantiate failure is 2.
template <typename F>
static int record_graph(da_denoiser *d, const char *what, F &&enqueue, hipGraphExec_t *out) {
    *out = nullptr;
    if (!d->cap_stream) DA_CHECK_HIP(hipStreamCreateWithFlags(&d->cap_stream, hipStreamNonBlocking));
    hipStream_t cs = d->cap_stream;
    hipGraph_t graph = nullptr;
    DA_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed));
    const int rc = enqueue(cs);
    const hipError_t e_end = hipStreamEndCapture(cs, &graph);
    const bool captured = e_end == hipSuccess && graph;
    hipError_t e_inst = hipSuccess;
    if (!rc && captured) e_inst = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    if (!captured) { set_error("%s: hipStreamEndCapture failed: %s", what, hipGetErrorString(e_end)); return 2; }
    if (e_inst != hipSuccess || !*out) { *out = nullptr; set_error("%s: hipGraphInstantiate failed: %s", what, hipGetErrorString(e_inst)); return 2; }
    return 0;
}

// a one-branch loop: replay the graph cached under `key`, recording it first if there is none
template <typename F>
static int launch_loop_graph(da_denoiser *d, const char *what, const LoopKey &key, F &&enqueue, hipStream_t st) {
    const da_denoiser::LoopEntry *hit = cache_find(d->loops, key, no_key, false);
    hipGraphExec_t exec = hit ? hit->exec : nullptr;
    if (!exec) {
        const int rc = record_graph(d, what, enqueue, &exec);
        if (rc) return rc;
        cache_insert(d->loops, 8, {key, no_key, exec, nullptr});       // eight: four Batches in flight x two loop lengths
    }
    DA_CHECK_HIP(hipGraphLaunch(exec, st));
    return 0;
}

static int ensure_pair_stream(da_denoiser *d) {
    if (d->pair_stream) return 0;
    // DA_PAIR_PRIO (experiment, default 0): 1 = the pair stream at the device's highest priority, -1 = at its lowest -- a standing
    // asymmetry between the branches (one takes free slots first, the other fills its tails) instead of two equals in lockstep
    const int prio = DA_XENV("DA_PAIR_PRIO", 0);
    if (prio) {
        int lo = 0, hi = 0;                                                     // lo = numerically greatest = lowest priority
        DA_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        DA_CHECK_HIP(hipStreamCreateWithPriority(&d->pair_stream, hipStreamNonBlocking, prio > 0 ? hi : lo));
    } else
        DA_CHECK_HIP(hipStreamCreateWithFlags(&d->pair_stream, hipStreamNonBlocking));
    DA_CHECK_HIP(hipEventCreateWithFlags(&d->ev_pair_fork, hipEventDisableTiming));
    DA_CHECK_HIP(hipEventCreateWithFlags(&d->ev_pair_join, hipEventDisableTiming));
    return 0;
}
// the pair stream behind everything enqueued on `us` so far; `join` brings it back into `us` on every exit of the caller's scope
static int fork_pair_stream(da_denoiser *d, hipStream_t us, StreamJoin &join) {
    DA_CHECK_HIP(hipEventRecord(d->ev_pair_fork, us));
    DA_CHECK_HIP(hipStreamWaitEvent(d->pair_stream, d->ev_pair_fork, 0));     // (under a capture of `us`: the pair stream joins the capture)
    join.arm(d->pair_stream, us, d->ev_pair_join);
    return 0;
}

extern "C" {

int da_abi_version(void) { return DA_ABI_VERSION; }
const char *da_last_error(void) { return da::g_err; }

int da_denoiser_create(const da_weights *w, int precision, void *stream, da_denoiser **out) {
    DA_REQUIRE(w && out, "da_denoiser_create: null argument");
    DA_REQUIRE(precision == DA_PREC_F32 || precision == DA_PREC_BF16, "bad precision %d", precision);
    DA_REQUIRE(w->n_layers >= 2 && w->n_layers <= DA_MAX_LAYERS, "n_layers out of range");
    DA_REQUIRE(w->arch == DA_ARCH_TRANSFORMER || w->arch == DA_ARCH_EXOPHORMER || w->arch == DA_ARCH_GCN, "bad arch %d", w->arch);
    DA_REQUIRE(w->arch != DA_ARCH_GCN || w->n_layers == 2, "gcn arch: n_layers must be 2 (backbones/gcn.py:9-14)");
    DA_REQUIRE(w->heads == 8, "heads must be 8");
    // k_embed_pos_time keeps the pose-MLP weight rows in a fixed register array (da_basic.hip); fail here, not on the first
    // forward or inside a hipGraph capture (the reference uses c_in = 2 / 4 in 2D and 7 in 3D, 13 in 3D with use_6dof)
    DA_REQUIRE(w->variant == DA_VARIANT_2D || w->variant == DA_VARIANT_3D || w->variant == DA_VARIANT_DISCRETE || w->variant == DA_VARIANT_DISCRETE_ROT,
               "bad variant %d", w->variant);
    if (w->variant == DA_VARIANT_3D)       // 7: quaternion wxyz | translation; 13: quaternion | translation | a1 | a2 (use_6dof), mlp_t.2 then [9, 256]
        DA_REQUIRE(w->c_in == 7 || w->c_in == 13, "da_denoiser_create(3D): c_in = %d is neither 7 nor 13 (use_6dof)", w->c_in);
    else
        DA_REQUIRE(w->c_in >= 1 && w->c_in <= 8, "da_denoiser_create: c_in = %d outside [1, 8]", w->c_in);
    const bool rotv = w->variant == DA_VARIANT_DISCRETE_ROT;           // Eff_GAT_Discrete_ROT: Eff_GAT_Discrete plus final_mlp_rot
    const bool discrete = w->variant == DA_VARIANT_DISCRETE || rotv;
    if (discrete) {
        // Eff_GAT_Discrete (efficient_gat_discrete.py:19-51): an index in, K logits out, always the transformer
        DA_REQUIRE(w->c_in == 1, "da_denoiser_create(discrete): c_in must be 1 (one position index per piece), got %d", w->c_in);
        DA_REQUIRE(w->c_out >= 2 && w->c_out <= 1024, "da_denoiser_create(discrete): K = c_out = %d outside [2, 1024]", w->c_out);
        DA_REQUIRE(w->arch == DA_ARCH_TRANSFORMER, "da_denoiser_create(discrete): arch must be DA_ARCH_TRANSFORMER");
        DA_REQUIRE(w->pos_w1 && w->head_w1 && w->head_b1, "da_denoiser_create(discrete): pos_w1 (pos_mlp.weight [K, 32]) / head_w1 / head_b1 missing");
        DA_REQUIRE(!rotv || (w->head_w0 && w->head_b0 && w->head_r_w0 && w->head_r_b0 && w->head_r_w1 && w->head_r_b1),
                   "da_denoiser_create(discrete rot): head_w0 / head_b0 or head_r_w0 / head_r_b0 / head_r_w1 / head_r_b1 (final_mlp_rot) missing");
    }
    da_denoiser *d = new da_denoiser();
    d->owner_pid = (long)getpid();
    d->prec = precision; d->variant = w->variant; d->arch = w->arch; d->steps = w->steps; d->c_in = w->c_in;
    d->c_out = w->c_out; d->F = w->feat_dim; d->D = w->feat_dim + 64; d->hidden = w->hidden; d->heads = w->heads;
    d->n_layers = w->n_layers; d->V = w->arch == DA_ARCH_EXOPHORMER ? w->virt_nodes : 0;
    d->head_hidden = w->variant == DA_VARIANT_3D ? 512 : (rotv ? 64 : 32);
    const int rc = denoiser_build(d, w, (hipStream_t)stream);       // da_denoiser_create.hip
    if (rc) { da_denoiser_destroy(d); return rc; }
    *out = d;
    return 0;
}

// bit 3: the hoisted mlp.0 product (feature columns once per loop, pose / timestep columns per step through launch_gemm_mfma's `pre`
// operand) exists for THIS denoiser's shapes -- the conditions launch_gemm_mfma itself checks (reduction a multiple of its 128-byte
// K stage, 16-byte aligned column slice and rows), not merely "MFMA enabled": the captured classifier-free-guidance loop needs it
static bool hoisted_mlp0_ok(const da_denoiser *d) {
    if (da::mfma_disabled()) return false;
    const int es = (int)da::esize(d->prec), bk = 128 / es, kpose = d->D - d->F;
    return kpose > 0 && kpose % bk == 0 && ((size_t)d->F * es) % 16 == 0 && ((size_t)d->D * es) % 16 == 0 && d->hidden % (16 / es) == 0;
}
int da_denoiser_flags(const da_denoiser *d) {
    return d ? (d->fused_mlp2 ? 1 : 0) | (d->lastfold ? 2 : 0) | (d->dense_only ? 4 : 0) | (hoisted_mlp0_ok(d) ? 8 : 0) : 0;
}

void da_denoiser_destroy(da_denoiser *d) {
    if (!d) return;
    // A forked child (multiprocessing's default start method) inherits the handle, and its garbage collector may drop it: the graphs, streams and
    // allocations belong to the parent's HIP context, and destroying them from the child faults.  The child gives up its copy of the host record only.
    if (d->owner_pid != (long)getpid()) { delete d; return; }
    for (hipEvent_t e : d->prof_ev) (void)hipEventDestroy(e);
    for (auto &e : d->loops) (void)hipGraphExecDestroy(e.exec);
    if (d->cap_stream) (void)hipStreamDestroy(d->cap_stream);
    if (d->side_stream) (void)hipStreamDestroy(d->side_stream);
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    for (auto &e : d->pair_loops) { (void)hipGraphExecDestroy(e.exec); if (e.exec_b) (void)hipGraphExecDestroy(e.exec_b); }
    if (d->pair_stream) (void)hipStreamDestroy(d->pair_stream);
    if (d->ev_pair_fork) (void)hipEventDestroy(d->ev_pair_fork);
    if (d->ev_pair_join) (void)hipEventDestroy(d->ev_pair_join);
    for (void *p : d->owned) (void)hipFree(p);
    delete d;
}

size_t da_denoiser_workspace_bytes(const da_denoiser *d, const da_graph *g) {
    if (!d || !g) return 0;
    return da::carve(d, g, nullptr).total;
}

int da_denoiser_set_features(da_denoiser *d, const da_graph *g, const float *feats, void *workspace,
                             size_t workspace_bytes, void *stream) {
    DA_REQUIRE(d && g && feats && workspace, "da_denoiser_set_features: null argument");
    int rc = check_graph(d, g);
    if (rc) return rc;
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = launch_set_feats(d->prec, g->n_real, d->F, d->D, feats, w.comb_in, st))) return rc;
    if (!mfma_disabled()) {       // loop-invariant part of mlp.0 (see da_forward.hip: embed_mlp); unsupported shapes fall back there
        rc = launch_gemm_mfma(d->prec, g->n_real, d->F, d->hidden, w.comb_in, d->D, d->mlp_w0, d->mlp_b0, DA_ACT_NONE, nullptr,
                              w.feat_proj, d->hidden, nullptr, st, d->D, nullptr);
        if (rc > 0) return rc;
        DA_REQUIRE(rc == 0, "da_denoiser_set_features: feature projection shape not supported (F=%d)", d->F);
        const size_t nb = (size_t)g->n_real * d->hidden;
        k_fill_bias_rows<<<(unsigned)((nb + 255) / 256), 256, 0, st>>>(d->prec, g->n_real, d->hidden, d->mlp_b0, w.feat_proj_unc);
        DA_LAUNCH_CHECK();
    }
    if (w.dense_bytes)      // padded rows / columns of the head-major buffers must be finite
        DA_CHECK_HIP(hipMemsetAsync((char *)workspace + w.dense_off, 0, w.dense_bytes, st));
    if (d->arch == DA_ARCH_GCN && (rc = launch_gcn_dinv(g, w.gcn_dinv, st))) return rc;
    if (d->V > 0) {
        char *dst = w.combined + (size_t)g->n_real * d->D * esize(d->prec);
        if ((rc = launch_set_virtual_rows(d->prec, g->n_nodes - g->n_real, d->V, d->D, d->virt_emb, dst, st))) return rc;
    }
    return 0;
}

int da_denoiser_forward(da_denoiser *d, const da_graph *g, const float *x, const int64_t *t, int64_t t_scalar,
                        float *out, float *alpha, int alpha_all_layers, float *pre_head, void *workspace,
                        size_t workspace_bytes, void *stream) {
    DA_REQUIRE(d && g && x && out && workspace, "da_denoiser_forward: null argument");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE, "da_denoiser_forward: a discrete denoiser takes position indices (da_denoiser_forward_idx)");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE_ROT, "da_denoiser_forward: a discrete rot denoiser takes position indices (da_denoiser_forward_rot)");
    int rc = check_graph(d, g);
    if (rc) return rc;
    DA_REQUIRE(!alpha || d->arch != DA_ARCH_GCN, "alpha requested from a GCN denoiser: GCN.forward returns no attention weights (gcn.py:22)");
    DA_REQUIRE(!alpha || g->edge_id, "alpha requested but graph has no edge_id");
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    return forward_impl(d, g, x, t, t_scalar, out, alpha, alpha_all_layers, pre_head, w, (hipStream_t)stream);
}

int da_ddim_step(const da_schedule *s, int variant, int mean_type, int n, int c, const float *x,
                 const float *model_out, const int64_t *t, int64_t t_scalar, int inference_ratio,
                 int prev_all_nonneg, float eta, const float *noise, float *x_prev, void *stream) {
    DA_REQUIRE(s && x && model_out && x_prev, "da_ddim_step: null argument");
    DA_REQUIRE(variant != DA_VARIANT_DISCRETE, "da_ddim_step: the discrete variant has no pose update (da_d3pm_step)");
    DA_REQUIRE(variant != DA_VARIANT_DISCRETE_ROT, "da_ddim_step: the discrete rot variant has no pose update (da_d3pm_rot_step)");
    DA_REQUIRE(eta == 0.f || noise, "da_ddim_step: eta > 0 needs noise");
    if (variant == DA_VARIANT_3D) {
        DA_REQUIRE(c == 7 || c == 13, "da_ddim_step(3D): c must be 7, or 13 (use_6dof), not %d", c);
        DA_REQUIRE(eta == 0.f, "da_ddim_step(3D): eta must be 0 (the reference binds DDIM only)");
        return launch_ddim3d(to_dev(s), mean_type, n, c - 4, x, model_out, t, t_scalar, inference_ratio, prev_all_nonneg,
                             x_prev, (hipStream_t)stream);
    }
    return launch_ddim2d(to_dev(s), mean_type, n, c, x, model_out, t, t_scalar, inference_ratio, prev_all_nonneg, eta,
                         noise, x_prev, (hipStream_t)stream);
}

int da_ddpm_step(const da_schedule *s, int n, int c, const float *x, const float *model_out, const int64_t *t,
                 int64_t t_scalar, const float *noise, float *x_prev, void *stream) {
    DA_REQUIRE(s && x && model_out && x_prev, "da_ddpm_step: null argument");
    return launch_ddpm2d(to_dev(s), n, c, x, model_out, t, t_scalar, noise, x_prev, (hipStream_t)stream);
}

static int enqueue_loop(da_denoiser *d, const da_graph *g, const da_schedule *s, int mean_type, int ratio,
                        int n_iters, const float *x_init, float *traj, float *x_final, const Workspace &w,
                        hipStream_t st, const da_loop_opts *o = nullptr, size_t traj_stride = 0, size_t noise_stride = 0) {
    const int nr = g->n_real;
    const int c = d->c_in;          // (3D: 7, or 13 with use_6dof -- the pose row the model returns, da_denoiser.h: pose_width)
    const size_t bytes = (size_t)nr * c * sizeof(float);
    const DeviceSchedule ds = to_dev(s);
    const float *cur = x_init;
    int it = 0, rc;
    const int first = ((s->steps - 1) / ratio) * ratio;            // reversed(range(0, steps, ratio))[0]
    // the variants of the reference's samplers that need more than forward + deterministic update (all inside the same
    // enqueue, so all inside the captured graph): classifier-free guidance = a second forward over zero features and a
    // linear combination (spatial_diffusion.py:568-589); eta > 0 / DDPM = a noise term read from a caller-filled
    // [n_iters, n_real, c] buffer (:485-510, :620-627 draw torch.randn_like per step; the host draws them in one call)
    const bool cfg = o && o->cfg, ddpm = o && o->sampler == 1;
    const float eta = o ? o->eta : 0.f;
    const bool plain = !cfg && !ddpm && eta == 0.f;
    bool h_ready = false;           // w.h already holds this step's value (written by the previous step's tail kernel)
    for (int i = first; i >= 0 && it < n_iters; i -= ratio, ++it) {
        float *nxt = traj ? traj + (size_t)it * (traj_stride ? traj_stride : (size_t)nr * c) : ((it & 1) ? w.xbuf1 : w.xbuf0);
        const int nonneg = (i - ratio) >= 0;
        DdimFuse df;
        df.s = ds; df.mean_type = mean_type; df.ratio = ratio; df.prev_all_nonneg = nonneg; df.t = i; df.x = cur; df.x_prev = nxt;
        df.done = 0;
        df.nx_on = 0; df.nx_done = 0;
        const bool fuse_off = (da::cfg().disable_folds & DA_FOLD_DDIM) != 0;
        const bool try_fuse = plain && !fuse_off && d->variant == DA_VARIANT_2D && !d->prof_on;
        // the tail kernel of this step may also produce the NEXT step's h (embedding + mlp.0 over the hoisted feature part): bf16, the 2D
        // transformer widths, a next step that exists
        // DA_TAIL_NEXT: 1 = every Batch, 0 = never, unset = Batches whose largest graph has >= 512 pieces (DA_STEP_AUTO; 144-piece Batches lose)
        const int nx_mode = da::cfg().tail_next;          // -1 = the large-Batch step rule (step_rule_batch), 0 never, 1 always
        const bool nx_want = nx_mode == 1 || (nx_mode < 0 && step_rule_batch(g));
        if (try_fuse && nx_want && nonneg && it + 1 < n_iters && d->prec == DA_PREC_BF16 && d->hidden == 128 && d->D - d->F == 64 && w.feat_proj &&
            !mfma_disabled()) {
            df.nx_on = 1; df.nx_t = i - ratio; df.nx_steps = d->steps; df.nx_cin = d->c_in; df.nx_ldw = d->D;
            df.nx_time_emb = d->time_emb; df.nx_w0 = d->pos_w0; df.nx_b0 = d->pos_b0; df.nx_w1 = d->pos_w1; df.nx_b1 = d->pos_b1;
            df.nx_wp = (const char *)d->mlp_w0 + (size_t)d->F * esize(d->prec); df.nx_feat_proj = w.feat_proj; df.nx_h = w.h;
        }
        if ((rc = forward_impl(d, g, cur, nullptr, i, w.model_out, nullptr, 0, nullptr, w, st, try_fuse ? &df : nullptr, false, h_ready))) return rc;
        h_ready = df.done && df.nx_done;
        if (df.done) { cur = nxt; continue; }
        if (cfg) {
            if ((rc = forward_impl(d, g, cur, nullptr, i, w.model_out_unc, nullptr, 0, nullptr, w, st, nullptr, true))) return rc;
            const size_t ne = (size_t)nr * c;
            k_cfg_combine<<<(unsigned)((ne + 255) / 256), 256, 0, st>>>(ne, o->cfg_w, w.model_out, w.model_out_unc);
            DA_LAUNCH_CHECK();
        }
        const float *nz = (o && o->noise) ? o->noise + (size_t)it * (noise_stride ? noise_stride : (size_t)nr * c) : nullptr;
        rc = timed(d, DA_PROF_UPDATE, st, [&] {
            if (d->variant == DA_VARIANT_3D)
                return launch_ddim3d(ds, mean_type, nr, t_channels(d), cur, w.model_out, nullptr, i, ratio, nonneg, nxt, st);
            if (ddpm)       // t_index == 0 adds no noise (spatial_diffusion.py:504-506)
                return launch_ddpm2d(ds, nr, c, cur, w.model_out, nullptr, i, i == 0 ? nullptr : nz, nxt, st);
            return launch_ddim2d(ds, mean_type, nr, c, cur, w.model_out, nullptr, i, ratio, nonneg, eta, eta > 0.f ? nz : nullptr, nxt, st);
        });
        if (rc) return rc;
        cur = nxt;
    }
    if (x_final && cur != x_final) DA_CHECK_HIP(hipMemcpyAsync(x_final, cur, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
}

int da_sample_loop_ex(da_denoiser *d, const da_graph *g, const da_schedule *s, int mean_type, int inference_ratio,
                      int max_iters, const float *x_init, float *traj, float *x_final, void *workspace,
                      size_t workspace_bytes, int use_graph, const da_loop_opts *opts, void *stream) {
    DA_REQUIRE(d && g && s && x_init && workspace, "da_sample_loop: null argument");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE, "da_sample_loop: a discrete denoiser samples position indices (da_sample_loop_idx)");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE_ROT, "da_sample_loop: a discrete rot denoiser samples position indices (da_sample_loop_rot)");
    da_loop_opts o;
    int rc = loop_opts("da_sample_loop_ex", d, opts, &o);
    if (rc) return rc;
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1, "da_sample_loop: bad ratio/steps");
    DA_REQUIRE(d->variant == DA_VARIANT_3D || d->c_in == d->c_out, "da_sample_loop: c_in != c_out");
    if ((rc = check_graph(d, g))) return rc;
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const int n_iters = loop_iters(s, inference_ratio, max_iters);
    auto enqueue = [&](hipStream_t on) { return enqueue_loop(d, g, s, mean_type, inference_ratio, n_iters, x_init, traj, x_final, w, on, &o); };
    if (d->prof_on) use_graph = 0;       // event bracketing is not capturable
    // the CALLER is capturing `stream` (e.g. a predict_step wrapped in torch.cuda.graph): the loop's kernels are enqueued on it directly -- they
    // become nodes of the caller's graph -- instead of launching a graph of the library's own from inside a capture
    if (stream_is_capturing(st)) use_graph = 0;
    if (!use_graph) return enqueue(st);
    return launch_loop_graph(d, "da_sample_loop",
                             loop_key(g, s, mean_type, inference_ratio, n_iters, x_init, traj, x_final, workspace, workspace_bytes, o), enqueue, st);
}

int da_sample_loop(da_denoiser *d, const da_graph *g, const da_schedule *s, int mean_type, int inference_ratio,
                   int max_iters, const float *x_init, float *traj, float *x_final, void *workspace,
                   size_t workspace_bytes, int use_graph, void *stream) {
    return da_sample_loop_ex(d, g, s, mean_type, inference_ratio, max_iters, x_init, traj, x_final, workspace, workspace_bytes,
                             use_graph, nullptr, stream);
}

// Two independent halves of one Batch as two parallel branches of ONE hipGraph: each branch is the complete loop of
// da_sample_loop over its own graphs, poses and workspace; the branches share nothing but the weights, so the runtime
// overlaps one half's projections / tail kernels with the other half's attention.
int da_sample_loop_pair_ex(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio, int max_iters,
                           const da_graph *g_a, const float *x_init_a, float *x_final_a, void *workspace_a, size_t workspace_a_bytes,
                           const da_graph *g_b, const float *x_init_b, float *x_final_b, void *workspace_b, size_t workspace_b_bytes,
                           float *traj_a, float *traj_b, size_t traj_stride, const da_loop_opts *opts, const float *noise_b,
                           size_t noise_stride, void *stream) {
    DA_REQUIRE(d && s && g_a && g_b && x_init_a && x_init_b && x_final_a && x_final_b && workspace_a && workspace_b,
               "da_sample_loop_pair: null argument");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE, "da_sample_loop_pair: a discrete denoiser samples position indices (da_sample_loop_idx)");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE_ROT, "da_sample_loop_pair: a discrete rot denoiser samples position indices (da_sample_loop_rot)");
    // the samplers of da_sample_loop_ex on both branches: one option set, half a reads opts->noise, half b noise_b (row ranges
    // of one [n_iters, N, c] draw: the poses then equal the one-branch loop's bit for bit)
    da_loop_opts oa, ob;
    int rc = loop_opts("da_sample_loop_pair_ex", d, opts, &oa);
    if (rc) return rc;
    ob = oa;
    ob.noise = noise_b;
    DA_REQUIRE(!(oa.sampler == 1 || oa.eta > 0.f) || ob.noise, "da_sample_loop_pair_ex: eta > 0 / DDPM need both noise pointers");
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1, "da_sample_loop_pair: bad ratio/steps");
    DA_REQUIRE(d->variant == DA_VARIANT_3D || d->c_in == d->c_out, "da_sample_loop_pair: c_in != c_out");
    // hybrid graphs fork the denoiser's side stream (virtual rows) inside every layer: fine when each branch is recorded as a graph of its
    // own (pair_split, the default), a cross-branch dependency through that one stream when both are recorded in one capture
    DA_REQUIRE((!g_a->hybrid && !g_b->hybrid) || da::cfg().pair_split, "da_sample_loop_pair: hybrid graphs need the two-graph form (da_config.pair_split = 1)");
    DA_REQUIRE(!d->prof_on, "da_sample_loop_pair: not available while profiling (event bracketing is not capturable)");
    DA_REQUIRE((traj_a == nullptr) == (traj_b == nullptr), "da_sample_loop_pair_traj: both trajectory pointers or none");
    DA_REQUIRE(!traj_a || traj_stride >= (size_t)(g_a->n_real + g_b->n_real) * d->c_in,
               "da_sample_loop_pair_traj: traj_stride smaller than one iteration of both halves");
    if ((rc = check_graph(d, g_a)) || (rc = check_graph(d, g_b))) return rc;
    const Workspace wa = carve(d, g_a, workspace_a), wb = carve(d, g_b, workspace_b);
    DA_REQUIRE(workspace_a_bytes >= wa.total && workspace_b_bytes >= wb.total, "da_sample_loop_pair: workspace too small");
    {
        const char *a0 = (const char *)workspace_a, *b0 = (const char *)workspace_b;
        DA_REQUIRE(a0 + wa.total <= b0 || b0 + wb.total <= a0, "da_sample_loop_pair: the two workspaces overlap");
    }
    const int n_iters = loop_iters(s, inference_ratio, max_iters);
    const LoopKey ka = loop_key(g_a, s, mean_type, inference_ratio, n_iters, x_init_a, traj_a, x_final_a, workspace_a, workspace_a_bytes, oa, traj_stride, noise_stride);
    const LoopKey kb = loop_key(g_b, s, mean_type, inference_ratio, n_iters, x_init_b, traj_b, x_final_b, workspace_b, workspace_b_bytes, ob, traj_stride, noise_stride);
    if ((rc = ensure_pair_stream(d))) return rc;
    hipStream_t us = (hipStream_t)stream, ps = d->pair_stream;
    auto branch = [&](int br, hipStream_t on) {
        return br == 0 ? enqueue_loop(d, g_a, s, mean_type, inference_ratio, n_iters, x_init_a, traj_a, x_final_a, wa, on, &oa, traj_stride, noise_stride)
                       : enqueue_loop(d, g_b, s, mean_type, inference_ratio, n_iters, x_init_b, traj_b, x_final_b, wb, on, &ob, traj_stride, noise_stride);
    };
    // both branches under ONE capture of `on`: branch A on it, branch B on the pair stream between a fork and a join (two parallel branches of
    // that capture's graph); the join also runs when a branch fails, so the capture is never left forked
    auto both = [&](hipStream_t on, int delay_us) -> int {
        StreamJoin join;
        int r = fork_pair_stream(d, on, join);
        if (r) return r;
        if (delay_us > 0) k_pair_delay<<<1, 64, 0, ps>>>((unsigned long long)delay_us * 100ull);
        if ((r = branch(0, on)) || (r = branch(1, ps))) return r;
        DA_CHECK_HIP(join.join());
        return 0;
    };
    // the caller is capturing `stream`: both branches go straight into the caller's capture -- no graph of the library's own is launched
    if (stream_is_capturing(us)) return both(us, 0);
    // DA_PAIR_SPLIT (default 1): the two branches as TWO graphs, launched on the caller's stream and on the library's pair stream between a
    // fork and a join event, instead of two parallel branches of one graph.  Measured (tools/multi_branch_probe.py, round 5): two independently
    // launched one-branch graphs of 32 puzzles ran a 64-puzzle step in 0.6734 ms where the one-graph pair loop needed 0.7002 on the same box --
    // the runtime does not run the two branches of one graph as independently as it runs two graphs on two streams.
    const bool split = cfg().pair_split != 0;
    const da_denoiser::LoopEntry *hit = cache_find(d->pair_loops, ka, kb, split);
    hipGraphExec_t exec = hit ? hit->exec : nullptr, exec_b = hit ? hit->exec_b : nullptr;
    if (!hit) {
        if (split) {
            if ((rc = record_graph(d, "da_sample_loop_pair, branch a", [&](hipStream_t cs) { return branch(0, cs); }, &exec))) return rc;
            if ((rc = record_graph(d, "da_sample_loop_pair, branch b", [&](hipStream_t cs) { return branch(1, cs); }, &exec_b))) {
                (void)hipGraphExecDestroy(exec);
                return rc;
            }
        } else {
            // experiment switch (DA_PAIR_DELAY_US, default 0): branch B starts this many microseconds after branch A, so that the two
            // branches run out of phase for the whole loop (one branch's attention beside the other's projections)
            if ((rc = record_graph(d, "da_sample_loop_pair", [&](hipStream_t cs) { return both(cs, DA_XENV("DA_PAIR_DELAY_US", 0)); }, &exec))) return rc;
        }
        cache_insert(d->pair_loops, 4, {ka, kb, exec, exec_b});
    }
    if (!exec_b) {
        DA_CHECK_HIP(hipGraphLaunch(exec, us));
        return 0;
    }
    StreamJoin join;
    if ((rc = fork_pair_stream(d, us, join))) return rc;
    DA_CHECK_HIP(hipGraphLaunch(exec, us));
    DA_CHECK_HIP(hipGraphLaunch(exec_b, ps));
    DA_CHECK_HIP(join.join());
    return 0;
}

int da_sample_loop_pair_traj(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio, int max_iters,
                             const da_graph *g_a, const float *x_init_a, float *x_final_a, void *workspace_a, size_t workspace_a_bytes,
                             const da_graph *g_b, const float *x_init_b, float *x_final_b, void *workspace_b, size_t workspace_b_bytes,
                             float *traj_a, float *traj_b, size_t traj_stride, void *stream) {
    return da_sample_loop_pair_ex(d, s, mean_type, inference_ratio, max_iters, g_a, x_init_a, x_final_a, workspace_a, workspace_a_bytes,
                                  g_b, x_init_b, x_final_b, workspace_b, workspace_b_bytes, traj_a, traj_b, traj_stride, nullptr, nullptr, 0,
                                  stream);
}

int da_sample_loop_pair(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio, int max_iters,
                        const da_graph *g_a, const float *x_init_a, float *x_final_a, void *workspace_a, size_t workspace_a_bytes,
                        const da_graph *g_b, const float *x_init_b, float *x_final_b, void *workspace_b, size_t workspace_b_bytes,
                        void *stream) {
    return da_sample_loop_pair_traj(d, s, mean_type, inference_ratio, max_iters, g_a, x_init_a, x_final_a, workspace_a, workspace_a_bytes,
                                    g_b, x_init_b, x_final_b, workspace_b, workspace_b_bytes, nullptr, nullptr, 0, stream);
}

// ---------------------------------------------------------------------------------------- discrete (D3PM) variant
int da_denoiser_forward_idx(da_denoiser *d, const da_graph *g, const int32_t *idx, const int64_t *t, int64_t t_scalar, float *logits,
                            float *alpha, int alpha_all_layers, void *workspace, size_t workspace_bytes, void *stream) {
    DA_REQUIRE(d && g && idx && logits && workspace, "da_denoiser_forward_idx: null argument");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE_ROT, "da_denoiser_forward_idx: a discrete rot denoiser has two heads and four feature images "
               "(da_denoiser_set_features_rot / da_denoiser_forward_rot)");
    DA_REQUIRE(d->variant == DA_VARIANT_DISCRETE, "da_denoiser_forward_idx: not a discrete denoiser (da_denoiser_forward takes poses)");
    int rc = check_graph(d, g);
    if (rc) return rc;
    DA_REQUIRE(!alpha || g->edge_id, "alpha requested but graph has no edge_id");
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    DiscreteIn di{idx, w.hh, (char *)w.pz, w.head_pre, 0};
    if ((rc = forward_impl(d, g, nullptr, t, t_scalar, nullptr, alpha, alpha_all_layers, nullptr, w, st, nullptr, false, false, &di))) return rc;
    const D3pmRows rows = di.rows();
    return timed(d, DA_PROF_HEAD, st, [&] {
        return launch_d3pm_tail(d->prec, g->n_real, d->c_out, d->heads, &rows, nullptr, 0.f, d->head_w1, d->head_b1, nullptr, logits, nullptr, st); });
}

static int enqueue_loop_idx(da_denoiser *d, const da_graph *g, const da_schedule *s, int ratio, int n_iters, const int32_t *idx_init,
                            int32_t *traj, int32_t *idx_final, const Workspace &w, hipStream_t st, const da_d3pm_opts &o) {
    // p_sample_loop, spatial_diffusion_discrete.py:324-356: for i in reversed(range(0, steps, ratio)): forward (two under guidance),
    // categorical reverse step.  Per step: the embedding lookup, the shared denoiser body up to final_mlp.0, ONE tail kernel.
    const int nr = g->n_real, K = d->c_out;
    const int first = ((s->steps - 1) / ratio) * ratio;
    const int32_t *cur = idx_init;
    int it = 0, rc;
    for (int i = first; i >= 0 && it < n_iters; i -= ratio, ++it) {
        int32_t *nxt = traj ? traj + (size_t)it * nr : (int32_t *)((it & 1) ? w.xbuf1 : w.xbuf0);
        DiscreteIn dc{cur, w.hh, (char *)w.pz, w.head_pre, 0}, du{cur, w.hh_unc, w.pz_unc, w.head_pre_unc, 0};
        if ((rc = forward_impl(d, g, nullptr, nullptr, i, nullptr, nullptr, 0, nullptr, w, st, nullptr, false, false, &dc))) return rc;
        if (o.cfg && (rc = forward_impl(d, g, nullptr, nullptr, i, nullptr, nullptr, 0, nullptr, w, st, nullptr, true, false, &du))) return rc;
        D3pmStep sp;
        sp.s = to_dev(s); sp.x_t = cur; sp.t_scalar = i; sp.ratio = ratio; sp.iteration = it; sp.x_prev = nxt; sp.seed = o.seed;
        sp.noise = o.noise ? o.noise + (size_t)it * nr * K : nullptr;
        const D3pmRows rc_ = dc.rows(), ru_ = du.rows();
        if ((rc = timed(d, DA_PROF_UPDATE, st, [&] {
                 return launch_d3pm_tail(d->prec, nr, K, d->heads, &rc_, o.cfg ? &ru_ : nullptr, o.cfg_w, d->head_w1, d->head_b1, nullptr, nullptr, &sp, st); }))) return rc;
        cur = nxt;
    }
    if (idx_final && cur != idx_final) DA_CHECK_HIP(hipMemcpyAsync(idx_final, cur, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return 0;
}

int da_sample_loop_idx(da_denoiser *d, const da_graph *g, const da_schedule *s, int inference_ratio, int max_iters, const int32_t *idx_init,
                       int32_t *traj, int32_t *idx_final, void *workspace, size_t workspace_bytes, int use_graph, const da_d3pm_opts *opts,
                       void *stream) {
    DA_REQUIRE(d && g && s && idx_init && workspace && opts, "da_sample_loop_idx: null argument");
    DA_REQUIRE(d->variant != DA_VARIANT_DISCRETE_ROT, "da_sample_loop_idx: a discrete rot denoiser samples positions and rotations (da_sample_loop_rot)");
    DA_REQUIRE(d->variant == DA_VARIANT_DISCRETE, "da_sample_loop_idx: not a discrete denoiser (da_sample_loop takes poses)");
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1 && s->alphas_cumprod, "da_sample_loop_idx: bad ratio / schedule");
    DA_REQUIRE(opts->noise || opts->seed, "da_sample_loop_idx: needs the uniforms (opts->noise) or a seed (opts->seed)");
    da_d3pm_opts o;
    memset(&o, 0, sizeof(o));
    o.cfg = opts->cfg ? 1 : 0; o.cfg_w = opts->cfg ? opts->cfg_w : 0.f; o.noise = opts->noise; o.seed = opts->seed;
    int rc = check_graph(d, g);
    if (rc) return rc;
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const int n_iters = loop_iters(s, inference_ratio, max_iters);
    auto enqueue = [&](hipStream_t on) { return enqueue_loop_idx(d, g, s, inference_ratio, n_iters, idx_init, traj, idx_final, w, on, o); };
    // the capture rules of da_sample_loop_ex: eager while profiling, straight into a capture the caller has open
    if (d->prof_on || stream_is_capturing(st)) use_graph = 0;
    if (!use_graph) return enqueue(st);
    da_loop_opts ko;                    // the key's share of the discrete options (mean_type -1 marks the discrete loop)
    memset(&ko, 0, sizeof(ko));
    ko.cfg = o.cfg; ko.cfg_w = o.cfg_w; ko.noise = o.noise;
    return launch_loop_graph(d, "da_sample_loop_idx",
                             loop_key(g, s, -1, inference_ratio, n_iters, idx_init, traj, idx_final, workspace, workspace_bytes, ko, 0, 0, o.seed), enqueue, st);
}

// ---------------------------------------------------------------------------------------- discrete position + rotation variant
// every entry of the variant needs the hoisted mlp.0 product: its per-step feature share IS the addend row the embedding selects
static int require_rot(const char *who, const da_denoiser *d) {
    DA_REQUIRE(d->variant == DA_VARIANT_DISCRETE_ROT, "%s: not a discrete rot denoiser (DA_VARIANT_DISCRETE_ROT)", who);
    DA_REQUIRE(hoisted_mlp0_ok(d), "%s: the hoisted mlp.0 path is not available for this denoiser (da_denoiser_flags bit 3)", who);
    return 0;
}

int da_denoiser_set_features_rot(da_denoiser *d, const da_graph *g, const float *feats4, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    DA_REQUIRE(d && g && feats4 && workspace, "da_denoiser_set_features_rot: null argument");
    int rc = require_rot("da_denoiser_set_features_rot", d);
    if (rc || (rc = check_graph(d, g))) return rc;
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    // the F-wide hoist of da_denoiser_set_features once per image (image 0 last: comb_in's feature columns are left holding it)
    for (int r = 3; r >= 0; --r) {
        if ((rc = launch_set_feats(d->prec, g->n_real, d->F, d->D, feats4 + (size_t)r * g->n_real * d->F, w.comb_in, st))) return rc;
        rc = launch_gemm_mfma(d->prec, g->n_real, d->F, d->hidden, w.comb_in, d->D, d->mlp_w0, d->mlp_b0, DA_ACT_NONE, nullptr,
                              w.feat_proj4 + (size_t)r * w.proj4_stride * esize(d->prec), d->hidden, nullptr, st, d->D, nullptr);
        if (rc > 0) return rc;
        DA_REQUIRE(rc == 0, "da_denoiser_set_features_rot: feature projection shape not supported (F=%d)", d->F);
    }
    if (w.dense_bytes)      // padded rows / columns of the head-major buffers must be finite
        DA_CHECK_HIP(hipMemsetAsync((char *)workspace + w.dense_off, 0, w.dense_bytes, st));
    return 0;
}

int da_denoiser_forward_rot(da_denoiser *d, const da_graph *g, const int32_t *idx, const int32_t *rot_acc, const int64_t *t,
                            int64_t t_scalar, float *logits, float *rot_logits, float *alpha, int alpha_all_layers, void *workspace,
                            size_t workspace_bytes, void *stream) {
    DA_REQUIRE(d && g && idx && logits && rot_logits && workspace, "da_denoiser_forward_rot: null argument");
    int rc = require_rot("da_denoiser_forward_rot", d);
    if (rc || (rc = check_graph(d, g))) return rc;
    DA_REQUIRE(!alpha || g->edge_id, "alpha requested but graph has no edge_id");
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    DiscreteIn di{idx, w.hh, (char *)w.pz, w.head_pre, 0, 1, rot_acc};
    if ((rc = forward_impl(d, g, nullptr, t, t_scalar, nullptr, alpha, alpha_all_layers, nullptr, w, st, nullptr, false, false, &di))) return rc;
    return timed(d, DA_PROF_HEAD, st, [&] {
        return launch_d3pm_rot_tail(d->prec, g->n_real, d->c_out, w.hh, d->head_w1, d->head_b1, d->head_r_w1, d->head_r_b1, nullptr, nullptr,
                                    logits, rot_logits, nullptr, st); });
}

static int enqueue_loop_rot(da_denoiser *d, const da_graph *g, const da_schedule *s, int ratio, int n_iters, const int32_t *idx_init,
                            const int32_t *rot_init, int32_t *traj_idx, int32_t *traj_acc, int32_t *idx_final, int32_t *acc_final,
                            const Workspace &w, hipStream_t st, const da_d3pm_rot_opts &o) {
    // p_sample_loop, spatial_diffusion_discrete_rot.py:334-375.  Per step: the embedding (lookup + addend-row select by rot_acc), the shared
    // body, the 64-wide first head layer, ONE tail kernel.  State without trajectories lives in xbuf0 / xbuf1 (each entry is read and
    // written by the same wave of the tail kernel, so it is updated in place).
    const int nr = g->n_real, K = d->c_out;
    const int first = ((s->steps - 1) / ratio) * ratio;
    int32_t *const st_idx = (int32_t *)w.xbuf0, *const st_acc = st_idx + nr, *const st_rot = (int32_t *)w.xbuf1;
    const int32_t *cur = idx_init, *rot = rot_init, *acc = nullptr;          // rot_acc starts at zero: image 0
    int it = 0, rc;
    for (int i = first; i >= 0 && it < n_iters; i -= ratio, ++it) {
        int32_t *nxt = traj_idx ? traj_idx + (size_t)it * nr : st_idx;
        int32_t *nacc = traj_acc ? traj_acc + (size_t)it * nr : st_acc;
        const int32_t *in = o.x_fixed ? o.x_fixed : cur;                       // only_rotation: every step starts from the given indices
        DiscreteIn di{in, w.hh, (char *)w.pz, w.head_pre, 0, 1, acc};
        if ((rc = forward_impl(d, g, nullptr, nullptr, i, nullptr, nullptr, 0, nullptr, w, st, nullptr, false, false, &di))) return rc;
        D3pmRotStep sp;
        sp.s = to_dev(s); sp.x_t = in; sp.rot_t = rot; sp.t_scalar = i; sp.ratio = ratio; sp.iteration = it; sp.seed = o.seed;
        sp.noise_x = o.noise_x ? o.noise_x + (size_t)it * nr * K : nullptr;
        sp.noise_rot = o.noise_rot ? o.noise_rot + (size_t)it * nr * 4 : nullptr;
        sp.x_prev = nxt; sp.cold = o.cold; sp.need_prev = o.cold;              // (rot_prev and its draws only feed the state under cold diffusion)
        sp.rot_acc_in = acc; sp.rot_next = st_rot; sp.rot_acc_out = nacc;
        if ((rc = timed(d, DA_PROF_UPDATE, st, [&] {
                 return launch_d3pm_rot_tail(d->prec, nr, K, w.hh, d->head_w1, d->head_b1, d->head_r_w1, d->head_r_b1, nullptr, nullptr, nullptr,
                                             nullptr, &sp, st); }))) return rc;
        cur = nxt; acc = nacc; rot = st_rot;
    }
    if (idx_final && cur != idx_final) DA_CHECK_HIP(hipMemcpyAsync(idx_final, cur, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (acc_final && acc && acc != acc_final) DA_CHECK_HIP(hipMemcpyAsync(acc_final, acc, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return 0;
}

int da_sample_loop_rot(da_denoiser *d, const da_graph *g, const da_schedule *s, int inference_ratio, int max_iters, const int32_t *idx_init,
                       const int32_t *rot_init, int32_t *traj_idx, int32_t *traj_rot_acc, int32_t *idx_final, int32_t *rot_acc_final,
                       void *workspace, size_t workspace_bytes, int use_graph, const da_d3pm_rot_opts *opts, void *stream) {
    DA_REQUIRE(d && g && s && idx_init && rot_init && workspace && opts, "da_sample_loop_rot: null argument");
    int rc = require_rot("da_sample_loop_rot", d);
    if (rc) return rc;
    DA_REQUIRE(inference_ratio >= 1 && s->steps >= 1 && s->alphas_cumprod, "da_sample_loop_rot: bad ratio / schedule");
    da_d3pm_rot_opts o;
    memset(&o, 0, sizeof(o));
    o.cold = opts->cold ? 1 : 0; o.x_fixed = opts->x_fixed; o.noise_x = opts->noise_x; o.noise_rot = o.cold ? opts->noise_rot : nullptr;
    o.seed = opts->seed;
    DA_REQUIRE((o.noise_x && (o.noise_rot || !o.cold)) || o.seed, "da_sample_loop_rot: needs the uniforms (opts->noise_x, opts->noise_rot) or a seed (opts->seed)");
    if ((rc = check_graph(d, g))) return rc;
    Workspace w = carve(d, g, workspace);
    DA_REQUIRE(workspace_bytes >= w.total, "workspace too small: %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const int n_iters = loop_iters(s, inference_ratio, max_iters);
    auto enqueue = [&](hipStream_t on) {
        return enqueue_loop_rot(d, g, s, inference_ratio, n_iters, idx_init, rot_init, traj_idx, traj_rot_acc, idx_final, rot_acc_final, w, on, o); };
    // the capture rules of da_sample_loop_ex: eager while profiling, straight into a capture the caller has open
    if (d->prof_on || stream_is_capturing(st)) use_graph = 0;
    if (!use_graph) return enqueue(st);
    da_loop_opts ko;                    // (mean_type -2 marks the position + rotation loop)
    memset(&ko, 0, sizeof(ko));
    ko.noise = o.noise_x;
    LoopKey key = loop_key(g, s, -2, inference_ratio, n_iters, idx_init, traj_idx, idx_final, workspace, workspace_bytes, ko, 0, 0, o.seed);
    key.rot_init = rot_init; key.rot_traj = traj_rot_acc; key.rot_final = rot_acc_final; key.x_fixed = o.x_fixed; key.noise_rot = o.noise_rot;
    key.cold = o.cold;
    return launch_loop_graph(d, "da_sample_loop_rot", key, enqueue, st);
}

size_t da_attn_dense_scratch_bytes(int prec, const da_graph *g, int heads, int C) {
    if (!g) return 0;
    const size_t s = esize(prec), hc = (size_t)heads * C;
    // (+ behind the four regions, for the folded C = 144 layer: room for the Q weights' pack_w_qlast image, da_conv_dense_ex)
    return 3 * align_up(((size_t)g->n_pad + 64) * hc * s, 256) + align_up(((size_t)g->n_nodes + 64) * hc * s, 256) +
           (heads == 8 && C == 144 ? w_qlast_bytes(heads, C, 256) : 0);
}

int da_conv_dense(int prec, const da_graph *g, int heads, int C, int Din, const void *x, const void *w,
                  const float *b, const void *residual, int act, void *out, void *scratch, void *stream) {
    DA_REQUIRE(g && x && w && out && scratch, "da_conv_dense: null argument");
    DA_REQUIRE(dense_ok(g, heads, C), "da_conv_dense: graph is not dense or head width %d unsupported", C);
    hipStream_t st = (hipStream_t)stream;
    const size_t s = esize(prec), hc = (size_t)heads * C;
#ifdef DA_EXPERIMENTS
    if (!residual && !g->hybrid && conv_fused_applicable(prec, heads, C, Din, g->max_graph_nodes, (int)hc)) {
        int rf = launch_conv_fused(prec, heads, C, Din, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->dense == 2, x, Din, w,
                                   b, act, out, (int)hc, st);
        DA_REQUIRE(rf == 0, "da_conv_dense: fused conv launch failed (%d)", rf);
        return 0;
    }
#endif
    const size_t hb = align_up(((size_t)g->n_pad + 64) * hc * s, 256);
    char *base = (char *)scratch;
    QkvScatter qs;
    qs.HC = (int)hc; qs.C = C; qs.n_pad = g->n_pad; qs.row_map = g->row_map;
    qs.Q = base; qs.K = base + hb; qs.Vt = base + 2 * hb; qs.S = base + 3 * hb;
    int rc = launch_gemm_mfma(prec, g->n_nodes, Din, 4 * (int)hc, x, Din, w, b, DA_ACT_NONE, nullptr, nullptr, 0, &qs, st);
    DA_REQUIRE(rc <= 0, "da_conv_dense: projection launch failed");
    DA_REQUIRE(rc == 0, "da_conv_dense: projection shape (Din=%d, HC=%d) not supported by the MFMA kernel", Din, (int)hc);
    DenseLayout L;
    L.Q = qs.Q; L.K = qs.K; L.Vt = qs.Vt; L.S = qs.S; L.n_pad = g->n_pad;
    rc = launch_attn_dense(prec, L, heads, C, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->pad_ptr,
                           g->dense == 2, residual, act, out, st);
    DA_REQUIRE(rc == 0, "da_conv_dense: attention launch failed (%d)", rc);
    return 0;
}

int da_conv_dense_ex(int prec, const da_graph *g, int heads, int C, int Din, const void *x, const void *w, const float *b,
                     const void *residual, int act, void *out, void *scratch, int flags, void *stream) {
    DA_REQUIRE(g && x && w && out && scratch, "da_conv_dense_ex: null argument");
    DA_REQUIRE(dense_ok(g, heads, C), "da_conv_dense_ex: graph is not dense or head width %d unsupported", C);
    const bool folded = (flags & DA_CONV_FOLDED_V32) != 0;
    DA_REQUIRE(!folded || (C == 144 && !residual && act == DA_ACT_NONE), "da_conv_dense_ex: folded value heads need C = 144, no residual, no activation");
    hipStream_t st = (hipStream_t)stream;
    const size_t s = esize(prec), hc = (size_t)heads * C;
    const size_t hb = align_up(((size_t)g->n_pad + 64) * hc * s, 256);
    char *base = (char *)scratch;
    QkvScatter qs;
    qs.HC = (int)hc; qs.C = C; qs.n_pad = g->n_pad; qs.row_map = g->row_map;
    qs.Q = base; qs.K = base + hb; qs.Vt = base + 2 * hb; qs.S = folded ? nullptr : base + 3 * hb;
    qs.Cv = folded ? 32 : 0;
    const int nout = folded ? 2 * (int)hc + heads * 32 : 4 * (int)hc;
    // the layer form the sampling loop takes for hidden layers of large complete graphs (da_forward.hip: dense_layer): the projection happens in the prologue of
    // the resident attention kernel; its per-head weight fragments are packed into the scratch's (then unused, adjacent) K and V regions
    const bool qsf = attn_qsf_enabled() && !folded && !residual && !g->hybrid && g->n_nodes == g->n_real && b && w_qs_bytes(heads, Din) <= 2 * hb &&
                     attn_qsf_applicable(prec, heads, C, Din, g->n_graphs, g->max_graph_nodes, g->n_pad, (flags & DA_CONV_Q_PRESCALED) ? 1 : 0);
    void *wq_img = base + hb;                        // (the K | V regions of the scratch: K | V stay in the CU)
    // fragment-major rows are a layout of THAT kernel's prologue and epilogue: no other path reads or writes it
    DA_REQUIRE(qsf || !(flags & DA_CONV_X_FM), "da_conv_dense_ex: DA_CONV_X_FM on a call that does not take the projection in the attention kernel");
    DA_REQUIRE(qsf || !(flags & DA_CONV_OUT_FM), "da_conv_dense_ex: DA_CONV_OUT_FM on a call that does not take the projection in the attention kernel");
    // the folded last layer of complete graphs as the sampling loop runs it (disable_folds bit 256 clear): the K | V' columns only, Q projected by the
    // attention kernel in its prologue -- the scratch's Q region is neither written nor read; the Q weights' fragment image goes behind the four regions
    const bool lq = folded && attn_last_qproj_enabled() && !g->hybrid && g->n_nodes == g->n_real && b &&
                    attn_last_qproj_applicable(prec, heads, C, Din, g->n_pad, (flags & DA_CONV_Q_PRESCALED) ? 1 : 0);
    void *wq_last = base + 3 * hb + align_up(((size_t)g->n_nodes + 64) * hc * s, 256);
    int rc = 0;
    if (qsf) {
        if ((rc = pack_w_qs(heads, Din, (int)hc, w, wq_img, st))) return rc;
    } else if (lq) {
        if ((rc = pack_w_qlast(heads, C, Din, w, wq_last, st))) return rc;
        qs.col0 = (int)hc;
        rc = launch_gemm_mfma(prec, g->n_nodes, Din, nout - (int)hc, x, Din, (const char *)w + hc * (size_t)Din * s, b + hc, DA_ACT_NONE, nullptr, nullptr, 0, &qs, st);
    } else
    rc = launch_gemm_mfma(prec, g->n_nodes, Din, nout, x, Din, w, b, DA_ACT_NONE, nullptr, nullptr, 0, &qs, st);
    DA_REQUIRE(rc == 0, "da_conv_dense_ex: projection shape (Din=%d, Nout=%d) not supported by the MFMA kernels", Din, nout);
    DenseLayout L;
    L.Q = qs.Q; L.K = qs.K; L.Vt = qs.Vt; L.S = qs.S; L.n_pad = g->n_pad; L.q_prescaled = (flags & DA_CONV_Q_PRESCALED) ? 1 : 0;
    if (qsf) { L.x = x; L.ldx = Din; L.kin = Din; L.wqs = wq_img; L.bias = b; L.x_fm = (flags & DA_CONV_X_FM) != 0; L.out_fm = (flags & DA_CONV_OUT_FM) != 0; }
    if (lq) { L.Q = nullptr; L.x = x; L.ldx = Din; L.kin = Din; L.wqs = wq_last; L.bias = b; }
    DenseFold fo;
    fo.cv = 32; fo.out = out; fo.n_rows = g->n_real;
    const DenseMask mk = dense_mask_of(g);
    rc = launch_attn_dense(prec, L, heads, C, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->pad_ptr, g->dense == 2, residual, act,
                           folded ? nullptr : out, st, g->hybrid ? &mk : nullptr, folded ? &fo : nullptr);
    DA_REQUIRE(rc == 0, "da_conv_dense_ex: attention launch failed (%d)", rc);
    return 0;
}

int da_debug_counters(int64_t *out, int n, int reset) {
    // (counters are only ever ADDED behind the first eight: a caller compiled against fewer gets the ones it has room for)
    DA_REQUIRE(out && n >= 8, "da_debug_counters: need room for 8 counters (%d exist)", DA_DBG_NCOUNTERS);
    unsigned long long a[4] = {0, 0, 0, 0}, b2[2] = {0, 0};
    int rc;
    if ((rc = da::attn_dense_counters(a, reset))) return rc;
#ifdef DA_EXPERIMENTS
    if ((rc = da::attn_dual_counters(b2, reset))) return rc;          // (k_attn_dual: experiments build only; the counter reads 0 otherwise)
#endif
    for (int k = 0; k < n; ++k) out[k] = 0;
    out[DA_DBG_OPT_GEN_WORKGROUPS] = (int64_t)a[0];
    out[DA_DBG_DENSE_FAST_EXITS] = (int64_t)a[1];
    out[DA_DBG_DUAL_GEN_SLABS] = (int64_t)b2[0];
    out[DA_DBG_OPT_MASKED_GEN_WORKGROUPS] = (int64_t)a[2];
    out[DA_DBG_RES_LAUNCHES] = (int64_t)da::attn_res_launches(reset);
    out[DA_DBG_RES_PROJ_LAUNCHES] = (int64_t)da::attn_res_qsf_launches(reset);
    out[DA_DBG_RES_FM_LAUNCHES] = (int64_t)da::attn_res_fm_launches(reset);
    out[DA_DBG_VIRT_IN_LAUNCH] = (int64_t)da::attn_virt_launches(reset);
    const int64_t lq = (int64_t)da::attn_last_qproj_launches(reset);
    if (n > DA_DBG_LAST_QPROJ_LAUNCHES) out[DA_DBG_LAST_QPROJ_LAUNCHES] = lq;
    return 0;
}

int da_profile_enable(da_denoiser *d, int on) {
    DA_REQUIRE(d, "da_profile_enable: null denoiser");
    d->prof_on = on != 0;
    d->prof_used = 0;
    d->prof_cls.clear();
    return 0;
}

int da_profile_read(da_denoiser *d, float *ms, int32_t *counts) {
    DA_REQUIRE(d && ms && counts, "da_profile_read: null argument");
    for (int k = 0; k < DA_PROF_NCLASS; ++k) { ms[k] = 0.f; counts[k] = 0; }
    for (size_t k = 0; k < d->prof_cls.size(); ++k) {
        DA_CHECK_HIP(hipEventSynchronize(d->prof_ev[2 * k + 1]));
        float t = 0.f;
        DA_CHECK_HIP(hipEventElapsedTime(&t, d->prof_ev[2 * k], d->prof_ev[2 * k + 1]));
        ms[d->prof_cls[k]] += t;
        counts[d->prof_cls[k]] += 1;
    }
    d->prof_used = 0;
    d->prof_cls.clear();
    return 0;
}

int da_linear(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const float *bias, int act,
              const void *residual, void *out, int ldo, void *stream) {
    DA_REQUIRE(A && W && out, "da_linear: null argument");
    return da::linear(prec, M, K, Nout, A, lda, W, bias, act, residual, out, ldo, (hipStream_t)stream);
}

size_t da_linear_packed_bytes(int prec, int K, int Nout) {
    if (prec != DA_PREC_BF16 || (K != 128 && K != 256) || Nout < 512 || Nout > 4096 || (Nout & 31)) return 0;
    return da::xpanel_packed_bytes(K, Nout);
}

int da_linear_pack(int prec, int K, int Nout, const void *W, int ldw, void *packed, void *stream) {
    DA_REQUIRE(W && packed, "da_linear_pack: null argument");
    DA_REQUIRE(da_linear_packed_bytes(prec, K, Nout) > 0, "da_linear_pack: no packed form for prec %d, K %d, Nout %d", prec, K, Nout);
    DA_REQUIRE((((size_t)W) & 15) == 0 && (((size_t)packed) & 15) == 0 && ((ldw <= 0 ? K : ldw) & 7) == 0, "da_linear_pack: W / packed must be 16-byte aligned");
    return da::pack_w_xpanel(K, Nout, W, ldw, packed, (hipStream_t)stream);
}

int da_linear_packed(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const void *packed,
                     const float *bias, int act, const void *residual, void *out, int ldo, void *stream) {
    DA_REQUIRE(A && W && out, "da_linear_packed: null argument");
    if (!da::mfma_disabled()) {
        const int rc = da::launch_gemm_mfma(prec, M, K, Nout, A, lda, W, bias, act, residual, out, ldo, nullptr, (hipStream_t)stream, 0, nullptr,
                                            packed);
        if (rc >= 0) return rc;
    }
    return da::linear(prec, M, K, Nout, A, lda, W, bias, act, residual, out, ldo, (hipStream_t)stream);
}

int da_attn_csr(int prec, const da_graph *g, int heads, int C, const void *qkvs, const void *residual, int act,
                void *out, float *alpha, void *stream) {
    DA_REQUIRE(g && qkvs && out, "da_attn_csr: null argument");
    // (as in the forward: tiny complete graphs at C = 104 take k_attn_tiny when no attention weights are asked for)
    if (!alpha && g->dense && g->n_nodes == g->n_real && g->graph_ptr && !dense_disabled()) {
        const int rt = launch_attn_tiny(prec, g->n_graphs, g->max_graph_nodes, g->graph_ptr, g->dense == 2, heads, C, qkvs, residual, act, out, (hipStream_t)stream);
        if (rt >= 0) return rt;
    }
    return launch_attn_csr(prec, g->n_nodes, g->row_ptr, g->col_src, g->edge_id, heads, C, qkvs, residual, act, out,
                           alpha, nullptr, (hipStream_t)stream);
}

}  // extern "C"
