/*
 * diffassemble_hip.h -- C ABI of libdiffassemble_hip.so (gfx950 / MI355X).
 *
 * The reference (IIT-PAVIS/DiffAssemble) is 100 % Python and has NO FFI layer for this
 * path: its "operator interface" is Python-level.  This header is therefore
 * the boundary the build defines.  Each entry point cites the reference code it replaces
 * (paths relative to /root/reference/puzzle_diff/model/).  Conventions:
 *
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host";
 *   - the library BORROWS caller (PyTorch) storage for the duration of a call and never
 *     frees it; the only memory it owns are the packed weights of a da_denoiser;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises, nothing allocates inside a forward/step call (the caller passes a
 *     workspace sized by da_denoiser_workspace_bytes), so calls are stream-capturable;
 *   - every function returns 0 on success, nonzero on error (da_last_error() has the text);
 *   - re-entrant per (denoiser, workspace, stream).
 *
 * Tensor layouts are row-major.  "act dtype" is fp32 in DA_PREC_F32 (parity mode,
 * 1e-4 relative vs the fp32 oracle) and bf16 in DA_PREC_BF16 (perf mode, fp32 accumulate).
 */
#ifndef DIFFASSEMBLE_HIP_H
#define DIFFASSEMBLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DA_ABI_VERSION 19

enum { DA_PREC_F32 = 0, DA_PREC_BF16 = 1 };
enum { DA_VARIANT_2D = 0, DA_VARIANT_3D = 1,             /* Eff_GAT / Eff_GAT_3d            */
       DA_VARIANT_DISCRETE = 2,                          /* Eff_GAT_Discrete (below)        */
       DA_VARIANT_DISCRETE_ROT = 3 };                    /* Eff_GAT_Discrete_ROT (below)    */
enum { DA_ARCH_TRANSFORMER = 0, DA_ARCH_EXOPHORMER = 1, /* GELU between convs / none      */
       DA_ARCH_GCN = 2 };                                /* two GCNConv, GELU after each    */
enum { DA_MEAN_EPSILON = 0, DA_MEAN_START_X = 1 };       /* spatial_diffusion.py:63-66      */
enum { DA_ACT_NONE = 0, DA_ACT_GELU = 1, DA_ACT_LEAKY02 = 2 };
enum { DA_MAX_LAYERS = 8 };

int da_abi_version(void);
const char *da_last_error(void);

/* ---------------------------------------------------------------------------------------
 * The library's switches (ABI 19).  The reference has no equivalent (its knobs are Python
 * kwargs); these replace what used to be ~70 getenv calls spread over the kernels' launchers.
 * Every field is initialised ONCE per process from the environment variable named beside
 * it, can be read / changed at run time (da_config_get / da_config_set: in-process A/B
 * measurements, tests), and is consulted when a call is made -- a denoiser keeps the folds
 * it was created with, a captured sampling-loop graph keeps the kernels it recorded.
 * No other environment variable changes what the default build of the library does:
 * A/B variants that lost, ablations and probes are compiled only into the EXPERIMENTS build
 * (DA_EXPERIMENTS=1 python __graft_entry__.py; da_build_flags() bit 0), see INTEGRATION.md.
 * ------------------------------------------------------------------------------------- */
typedef struct da_config {
    int32_t struct_bytes;        /* sizeof(da_config) as the caller compiled it (checked by da_config_set)          */
    int32_t disable_mfma;        /* DA_DISABLE_MFMA=1: generic (non matrix-core) linear kernels                      */
    int32_t disable_dense;       /* DA_DISABLE_DENSE=1: every attention walks the edge list (CSR kernels)            */
    int32_t disable_folds;       /* DA_DISABLE_FOLDS=<bits>: 1 mlp.2 composed into its consumers, 2 folded last      */
                                 /* layer, 4 softmax scale inside Wq, 8 DDIM update inside the head kernel,          */
                                 /* 16 one-kernel tail, 32 virtual rows on a side stream / inside the masked         */
                                 /* attention's launch (hybrid graphs), 64 a hidden layer's Q|K|V|skip projection in */
                                 /* the prologue of its K/V-resident attention kernel (no projection kernel),        */
                                 /* 128 such layers handing their rows to the next one in MFMA operand order         */
                                 /* (fragment-major over the padded slots; needs bit 64 clear; fixed per denoiser    */
                                 /* at creation, like bit 64), 256 the folded last layer's Q projected in the        */
                                 /* prologue of its attention kernel on complete graphs (bf16, conv input 256): the  */
                                 /* projection kernel writes K | V' only, Q never exists in memory (fixed per        */
                                 /* denoiser at creation; da_conv_dense_ex asks per call)                            */
    int32_t attn_level;          /* DA_ATTN_LEVEL: 0 = the general dense kernel only, 1 = + the optimistic ring      */
                                 /* kernels, 2 = + the K/V-resident hidden-layer kernel (default)                    */
    int32_t xpanel;              /* DA_ENABLE_XPANEL: -1 = row-panel projections for large Batches (largest graph    */
                                 /* >= 512 pieces or >= 16 384 pieces in all; default), 0 never, 1 always            */
    int32_t tail_next;           /* DA_TAIL_NEXT: -1 = next step's embedding inside the tail kernel for the same     */
                                 /* large Batches (default), 0 never, 1 always                                       */
    int32_t pair_split;          /* DA_PAIR_SPLIT: 1 = the pair loop as two graphs on two streams (default), 0 = one */
    int32_t train_attn;          /* DA_TRAIN_ATTN: 0 = edge-list kernels only, 1 = grouped-GEMM attention with pair  */
                                 /* matrices, 2 = + flash-style hybrid kernels in the bf16-operand mode (default)    */
    int32_t train_side_streams;  /* DA_TRAIN_SIDE_STREAMS bits: 1 weight-gradient products, 2 hybrid virtual rows    */
} da_config;
int da_config_get(da_config *out /* host */);
int da_config_set(const da_config *in /* host */);
int da_build_flags(void);        /* bit 0: EXPERIMENTS build                                                         */

/* ---------------------------------------------------------------------------------------
 * Weights of one denoiser, fp32 device pointers in the reference's state-dict layout
 * ([out, in] like nn.Linear).  Replaces: the parameters of backbones/efficient_gat.py:57-102
 * (Eff_GAT) or backbones/efficient_gat_3d.py:99-152 (Eff_GAT_3d), incl. the PyG
 * TransformerConv lin_{query,key,value,skip} of backbones/Transformer_GNN.py:9-25 and the
 * virt_node_embedding of backbones/exophormer_gnn.py:158-159.
 * DA_ARCH_GCN replaces the GCN of backbones/gcn.py:5-22 (efficient_gat.py:65-70, efficient_gat_3d.py:114-119):
 * n_layers = 2, conv_wq[l] = module_list.l.lin.weight ([256, D] / [D, 256]), conv_bq[l] = module_list.l.bias
 * ([256] / [D]); the other conv pointers, heads and virt_nodes are not read.
 * DA_VARIANT_DISCRETE replaces Eff_GAT_Discrete (backbones/efficient_gat_discrete.py:19-51), the denoiser of the discrete position
 * diffusion: the 2D transformer body between an embedding lookup and a K-wide logits head.  c_in = 1 (one position index per
 * piece), c_out = K with 2 <= K <= 1024, arch = DA_ARCH_TRANSFORMER, pos_w1 = pos_mlp.weight [K, 32] (pos_w0 / pos_b0 / pos_b1
 * are NULL and not read), head_w1 / head_b1 = final_mlp.2 [K, 32] / [K]; da_denoiser_create checks all of it.  A discrete
 * denoiser is driven through da_denoiser_forward_idx / da_sample_loop_idx; every entry that takes float poses
 * (da_denoiser_forward, da_sample_loop*, da_ddim_step with this variant) REJECTS it with a da_last_error message and launches
 * nothing (da_ddpm_step takes neither a denoiser nor a variant: the host layer refuses it).  The layout of this struct is unchanged.
 * DA_VARIANT_DISCRETE_ROT replaces Eff_GAT_Discrete_ROT (backbones/efficient_gat_discrete_rotation.py:19-64): the weights of
 * DA_VARIANT_DISCRETE plus a second, 4-wide head, head_r_w0 / head_r_b0 = final_mlp_rot.0 [32, D] / [32] and head_r_w1 /
 * head_r_b1 = final_mlp_rot.2 [4, 32] / [4]; da_denoiser_create checks them.  It is driven through the *_rot entries
 * (da_denoiser_set_features_rot, da_denoiser_forward_rot, da_sample_loop_rot); the float-pose entries reject it like the
 * position model, and the *_idx entries reject it with a message that names the rot entries.
 * ------------------------------------------------------------------------------------- */
typedef struct da_weights {
    int32_t variant;      /* DA_VARIANT_*                                                  */
    int32_t arch;         /* DA_ARCH_*                                                     */
    int32_t steps;        /* rows of time_emb                                              */
    int32_t c_in;         /* pose channels in: 2 | 4 (2D), 7 (3D); 1 <= c_in <= 8, checked by da_denoiser_create */
    int32_t c_out;        /* pose channels out: 2 | 4 (2D); 3D heads are 3 + 3             */
    int32_t feat_dim;     /* piece-feature width F: 1088 (2D) / 768 (3D vn_dgcnn)          */
    int32_t hidden;       /* mlp hidden width: 128 (2D) / 256 (3D)                         */
    int32_t heads;        /* 8                                                             */
    int32_t n_layers;     /* 4                                                             */
    int32_t virt_nodes;   /* V (exophormer), else 0                                        */
    const float *time_emb;                  /* [steps, 32]                                  */
    const float *pos_w0, *pos_b0;           /* [16, c_in], [16]                             */
    const float *pos_w1, *pos_b1;           /* [32, 16], [32]                               */
    const float *mlp_w0, *mlp_b0;           /* [hidden, D], [hidden]      D = F + 64        */
    const float *mlp_w1, *mlp_b1;           /* [D, hidden], [D]                             */
    const float *conv_wq[DA_MAX_LAYERS], *conv_bq[DA_MAX_LAYERS];   /* [H*C_l, Din_l], [H*C_l] */
    const float *conv_wk[DA_MAX_LAYERS], *conv_bk[DA_MAX_LAYERS];
    const float *conv_wv[DA_MAX_LAYERS], *conv_bv[DA_MAX_LAYERS];
    const float *conv_ws[DA_MAX_LAYERS], *conv_bs[DA_MAX_LAYERS];
    const float *virt_emb;                  /* [V, D] or NULL                               */
    const float *head_w0, *head_b0;         /* 2D final_mlp.0 [32, D]; 3D mlp_t.0 [256, D]  */
    const float *head_w1, *head_b1;         /* 2D final_mlp.2 [c_out, 32]; 3D mlp_t.2 [3,256] */
    const float *head_r_w0, *head_r_b0;     /* 3D mlp_r.0 [256, D] (NULL in 2D); discrete rot: final_mlp_rot.0 [32, D] */
    const float *head_r_w1, *head_r_b1;     /* 3D mlp_r.2 [3, 256]; discrete rot: final_mlp_rot.2 [4, 32]              */
} da_weights;

/* ---------------------------------------------------------------------------------------
 * Piece graph of one Batch.  Replaces: the PyG `edge_index` / `batch` arguments of
 * Eff_GAT.forward_with_feats (efficient_gat.py:121-129).  Built once per Batch by the host
 * (diffassemble_amd/graph_plan.py) from edge_index[2,E] (row 0 = source j, row 1 = target i):
 *   CSR by destination: incoming edges of node i are col_src[row_ptr[i] .. row_ptr[i+1]),
 *   multi-edges kept (PyG softmax semantics); edge_id[] maps a CSR slot to its position in
 *   the caller's edge_index (for the alpha[E,H] output).  For the exophormer arch the
 *   host appends the V*G virtual rows and the quirky virtual edges of
 *   exophormer_gnn.py:167-200 before building the CSR: n_nodes counts them, n_real does not.
 *   dense != 0 declares that every graph is complete (self loops iff dense == 1, none iff
 *   dense == 2), which lets the library take the block-diagonal MFMA attention kernel;
 *   graph_ptr[G+1] are the node offsets of the graphs (required when dense != 0).
 * ------------------------------------------------------------------------------------- */
typedef struct da_graph {
    int32_t n_nodes;          /* rows processed by the convs (real + virtual)              */
    int32_t n_real;           /* real pieces (rows of x / feats / out)                     */
    int32_t n_graphs;
    int32_t dense;            /* 0 = CSR only, 1 = complete + self loops, 2 = complete w/o */
    int64_t n_edges;
    const int32_t *row_ptr;   /* [n_nodes + 1]                                             */
    const int32_t *col_src;   /* [n_edges]                                                 */
    const int32_t *edge_id;   /* [n_edges] or NULL                                         */
    const int32_t *graph_ptr; /* [n_graphs + 1] or NULL                                    */
    int32_t max_graph_nodes;  /* largest graph (dense mode tiling)                         */
    /* dense mode only: every graph gets a 64-aligned slot of rows in the head-major Q / K / V
     * buffers: pad_ptr[g] = first padded row of graph g, n_pad = pad_ptr[G], row_map[i] =
     * padded row of node i.                                                               */
    int32_t n_pad;
    const int32_t *pad_ptr;   /* [n_graphs + 1] or NULL                                    */
    const int32_t *row_map;   /* [n_nodes] or NULL                                         */
    /* training only (da_train_backward): the same edges grouped by SOURCE node, i.e. the
     * outgoing edges of node j are out_dst[out_ptr[j] .. out_ptr[j+1]); multi-edges kept.
     * Hybrid graphs (below) train on adjacency-masked grouped GEMMs over their regular edges and
     * walk only the REMAINDER edges: out_ptr / out_dst then hold the by-source orientation of
     * irr_row_ptr / irr_col_src (out_dst may be empty), and row_ptr / col_src may be NULL.   */
    const int32_t *out_ptr;   /* [n_nodes + 1] or NULL                                     */
    const int32_t *out_dst;   /* [n_edges] or NULL                                         */
    /* hybrid mode (inference): for graphs that are neither complete nor small -- the Exphander
     * expanders of puzzle_dataset.py:33-152 with the exophormer virtual nodes -- the host splits the
     * edge list: edges whose two ends are real nodes of one graph and that occur once become one bit
     * of a per-graph adjacency mask (bit j of row i of graph g = edge j -> i; rows start at byte
     * mask_ptr[g], row stride = padded slot count / 8 bytes) and run through the masked MFMA attention;
     * every other edge (virtual nodes, duplicates, cross-graph pairs) stays a CSR by destination that a
     * second kernel merges into the same softmax.  Needs pad_ptr / row_map (virtual rows of a graph get
     * the slots behind its real nodes) and graph_ptr.                                            */
    int32_t hybrid;           /* 0 / 1                                                     */
    int32_t band_degree;      /* > 0: hybrid graph in the banded Exphander layout of degree d (slot_node set, every
                               * graph n = max_graph_nodes nodes, no duplicate edges, no virtual rows): the GCN
                               * aggregates it in closed form (da_gcn.hip).  0 otherwise; the attention ignores it.  */
    const uint8_t *mask;      /* adjacency bits or NULL                                    */
    const int64_t *mask_ptr;  /* [n_graphs + 1] byte offsets                               */
    const int32_t *irr_row_ptr; /* [n_nodes + 1] remainder CSR                             */
    const int32_t *irr_col_src; /* [remainder edges]                                       */
    /* hybrid mode, optional (NULL = not given).  slot_node: the graph's padded slots may hold its nodes in any order
     * (row_map[node] = slot); slot_node[slot] = node is the inverse (-1 for padding), and the adjacency rows / bits are
     * then indexed by SLOT.  An Exphander graph (puzzle_dataset.py:115-152) laid out by its generator's permutation is a
     * circulant band in slot space.  blk_class: per graph a table of one byte per (32-slot query slab, 32-slot key block):
     * 0 = no regular edge, 1 = some, 2 = all 1024 pairs; rows of blk_class_stride bytes (a multiple of 4), graph g's table
     * at byte blk_class_ptr[g] (graphs of one shape may share a table, and mask_ptr[] entries may coincide likewise).     */
    const int32_t *slot_node;
    const uint8_t *blk_class;
    const int64_t *blk_class_ptr;
    int32_t blk_class_stride;
    int32_t reserved1;
    /* hybrid mode, optional: per padded SLOT the remainder-edge metadata the masked attention's epilogue needs, gathered
     * once per Batch so that the kernel reads ONE 16-byte record per query instead of walking slot_node -> irr_row_ptr ->
     * irr_col_src -> row_map (four dependent loads in front of every workgroup):
     *   rm_meta[slot] = { irr_row_ptr[node], irr_row_ptr[node + 1], row_map[irr_col_src[irr_row_ptr[node]]] (the slot of the
     *   first remainder source; any valid slot when there is none), node }; node = -1 for padding / virtual slots.        */
    const int32_t *rm_meta;   /* [n_pad][4] or NULL                                        */
    /* hybrid mode, optional: the remainder edges of the rows the masked attention does NOT own (the exophormer's virtual
     * nodes, exophormer_gnn.py:183-200) with duplicated (source, target) pairs merged: CSR by destination over ALL nodes (real
     * rows empty), one entry per distinct source and its multiplicity -- PyG's softmax counts a duplicated edge k times, i.e.
     * weighs exp(score) by k in numerator and denominator.  The pairing quirk of the reference makes most virtual -> virtual
     * edges duplicates (at V = 8, n = 900, 32 puzzles: 232 448 edges into virtual nodes, 29 256 distinct pairs).          */
    const int32_t *agg_row_ptr;   /* [n_nodes + 1] or NULL                                 */
    const int32_t *agg_col_src;   /* [distinct pairs]                                      */
    const float *agg_mult;        /* [distinct pairs] multiplicities                       */
} da_graph;

typedef struct da_denoiser da_denoiser;

/* Pack the weights into the library's own device buffers (act dtype; Q|K|V|skip fused per
 * layer).  Allocates (hipMalloc) -- not capturable; call once per checkpoint load.          */
int da_denoiser_create(const da_weights *w, int precision, void *stream, da_denoiser **out);
void da_denoiser_destroy(da_denoiser *d);

/* Which algebraic folds the packed denoiser uses (2D transformer arch): bit 0 = mlp.2 composed into the
 * conv-0 projection and final_mlp.0; bit 1 = last conv's value / skip projections composed with final_mlp.0
 * (32-wide value heads in the last attention).  For reporting executed vs algorithmic FLOPs.
 * bit 2 = every layer has a block-diagonal MFMA attention kernel: for complete graphs (da_graph.dense != 0)
 * row_ptr / col_src / edge_id may be NULL unless alpha is requested (the host can skip sorting the edge list).
 * bit 3 = the per-step mlp.0 runs on its hoisted form (feature columns multiplied once per Batch), which the UNCONDITIONAL pass
 * of classifier-free guidance inside the captured loops needs (da_loop_opts.cfg); clear (DA_DISABLE_MFMA=1): run guidance per step. */
int da_denoiser_flags(const da_denoiser *d);

/* Bytes of caller-provided workspace needed for a graph of this size.                      */
size_t da_denoiser_workspace_bytes(const da_denoiser *d, const da_graph *g);

/* Once per Batch (features are loop-invariant: spatial_diffusion.py:653 computes them once
 * per p_sample_loop): converts piece features [n_real, F] fp32 into the workspace and
 * writes the virtual-node rows.  Must precede da_denoiser_forward on that workspace.       */
int da_denoiser_set_features(da_denoiser *d, const da_graph *g, const float *feats,
                             void *workspace, size_t workspace_bytes, void *stream);

/* One denoiser forward == Eff_GAT.forward_with_feats (efficient_gat.py:121-146) or
 * Eff_GAT_3d.forward_with_feats (efficient_gat_3d.py:173-220), encoder bypassed.
 *   x      [n_real, c_in] fp32 noisy poses
 *   t      [n_real] int64 per-node timestep (reference contract), or NULL => t_scalar
 *   out    [n_real, c_out] fp32 (3D: [n_real, 7] = unit quaternion wxyz | translation)
 *   alpha  NULL, or fp32 attention weights in the caller's edge order (needs g->edge_id):
 *          alpha_all_layers == 0: [n_edges, heads] of the LAST conv (what Exophormer_GNN
 *          returns, exophormer_gnn.py:205-215); != 0: [n_layers, n_edges, heads], every conv
 *          (what Transformer_GNN returns, Transformer_GNN.py:32-41)
 *   pre_head    NULL or [n_real, 6] fp32 (3D only): raw (r_pred, t_pred) before exp/quat   */
int da_denoiser_forward(da_denoiser *d, const da_graph *g, const float *x, const int64_t *t,
                        int64_t t_scalar, float *out, float *alpha, int alpha_all_layers,
                        float *pre_head, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * GCN aggregation (DA_ARCH_GCN; PyG GCNConv with default settings, backbones/gcn.py:5-22):
 *   out[n_nodes, W] = act(D^-1/2 (A' + I) D^-1/2 X + bias), A' = the edges without self loops (multi-edges
 *   counted), degrees at the target.  X / out act dtype, bias fp32 [W] or NULL, W % 4 == 0.  Complete graphs
 *   (dense != 0) and banded Exphander plans (band_degree > 0) are aggregated in closed form; any other plan needs
 *   the CSR and dinv [n_nodes] fp32 from da_gcn_dinv (a no-op on the closed-form plans).  Kernel-level test entries;
 *   da_denoiser_forward runs the same kernels.
 * ------------------------------------------------------------------------------------- */
int da_gcn_dinv(const da_graph *g, float *dinv, void *stream);
int da_gcn_aggregate(int prec, const da_graph *g, int W, const float *dinv, const void *X, const float *bias, int act,
                     void *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Diffusion schedule tables (fp32 [T] device pointers) == the registered buffers of
 * GNN_Diffusion.__init__, spatial_diffusion.py:282-321.
 * ------------------------------------------------------------------------------------- */
typedef struct da_schedule {
    int32_t steps;
    const float *betas;
    const float *alphas_cumprod;
    const float *sqrt_recip_alphas;
    const float *sqrt_recip_alphas_cumprod;
    const float *sqrt_recipm1_alphas_cumprod;
    const float *sqrt_one_minus_alphas_cumprod;
    const float *posterior_variance;
} da_schedule;

/* DDIM update after the model call == p_sample_ddim, spatial_diffusion.py:555-566,603-627
 * (2D) / spatial_diffusion_3d_test_double_diffusion.py:595-685 (3D: variant = DA_VARIANT_3D,
 * c = 7, SO(3) algebra of utils_3d.py:1018-1061 for the quaternion part).
 *   x, model_out, x_prev: [n, c] fp32.  t per node or NULL => t_scalar.
 *   prev_all_nonneg: the host-evaluated `(t - ratio >= 0).all()` branch of :560.
 *   eta: 0 for DDIM; > 0 adds eta*sqrt(var)*noise ([n, c] fp32, may be NULL when eta == 0). */
int da_ddim_step(const da_schedule *s, int variant, int mean_type, int n, int c, const float *x,
                 const float *model_out, const int64_t *t, int64_t t_scalar, int inference_ratio,
                 int prev_all_nonneg, float eta, const float *noise, float *x_prev, void *stream);

/* DDPM update == p_sample_ddpm, spatial_diffusion.py:485-510 (noise NULL <=> t_index == 0). */
int da_ddpm_step(const da_schedule *s, int n, int c, const float *x, const float *model_out,
                 const int64_t *t, int64_t t_scalar, const float *noise, float *x_prev,
                 void *stream);

/* The whole sampling loop == p_sample_loop, spatial_diffusion.py:635-676 /
 * ...double_diffusion.py:688-731: for i in reversed(range(0, steps, ratio)): forward + DDIM
 * update.  x_init [n_real, c] fp32; traj (nullable) [n_iters, n_real, c] receives every
 * step's poses (the reference keeps them all), x_final (nullable) the last.  max_iters <= 0
 * runs all iterations.  With use_graph != 0 the iterations are recorded once into a hipGraph
 * (cached inside the denoiser, keyed on the arguments) and replayed with one launch.       */
int da_sample_loop(da_denoiser *d, const da_graph *g, const da_schedule *s, int mean_type,
                   int inference_ratio, int max_iters, const float *x_init, float *traj,
                   float *x_final, void *workspace, size_t workspace_bytes, int use_graph,
                   void *stream);

/* The loop's other samplers, inside the same (capturable) enqueue -- spatial_diffusion.py:485-510 (p_sample_ddpm),
 * :568-589 (classifier-free guidance: a second denoiser pass over ZERO piece features, out = (1 + w) cond - w unc) and
 * :620-627 (eta > 0: + eta sqrt(var) noise).  `noise` [n_iters, n_real, c] fp32 holds one standard-normal draw per
 * iteration (the reference calls torch.randn_like once per step; the caller fills the buffer once per loop); it is read
 * by the update kernels of the replayed graph, so refill it in place before every launch.  2D only.  opts == NULL is
 * da_sample_loop. */
typedef struct da_loop_opts {
    int32_t sampler;      /* 0 = DDIM (p_sample_ddim), 1 = DDPM (p_sample_ddpm)                       */
    float eta;            /* DDIM only; 0 = deterministic                                             */
    int32_t cfg;          /* != 0: classifier-free guidance                                           */
    float cfg_w;          /* classifier_free_w                                                        */
    const float *noise;   /* [n_iters, n_real, c] or NULL (required when sampler == 1 or eta > 0)     */
} da_loop_opts;
int da_sample_loop_ex(da_denoiser *d, const da_graph *g, const da_schedule *s, int mean_type,
                      int inference_ratio, int max_iters, const float *x_init, float *traj,
                      float *x_final, void *workspace, size_t workspace_bytes, int use_graph,
                      const da_loop_opts *opts, void *stream);

/* The same loop over TWO disjoint sets of puzzles of one Batch (the puzzles of a Batch never
 * interact: spatial_diffusion.py:635-676 runs them through one block-diagonal graph), recorded
 * as two parallel branches of one hipGraph -- each with its own da_graph, poses and workspace
 * (features staged into each with da_denoiser_set_features) -- and replayed with one launch:
 * one half's projections overlap the other half's attention.  Complete graphs only (hybrid
 * graphs already fork a side stream inside the forward); no trajectory; always a hipGraph.   */
int da_sample_loop_pair(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio,
                        int max_iters,
                        const da_graph *g_a, const float *x_init_a, float *x_final_a,
                        void *workspace_a, size_t workspace_a_bytes,
                        const da_graph *g_b, const float *x_init_b, float *x_final_b,
                        void *workspace_b, size_t workspace_b_bytes, void *stream);
/* The same two-branch loop keeping the trajectory the reference's p_sample_loop returns (spatial_diffusion.py:635-676 appends
 * every x_{t-1}): iteration i of half a / b is written to traj_a / traj_b + i * traj_stride (floats; the two halves normally are
 * row ranges of one [n_iters, N, c] buffer: traj_b = traj_a + n_real_a * c, traj_stride = N * c).  Both NULL = da_sample_loop_pair. */
int da_sample_loop_pair_traj(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio,
                             int max_iters,
                             const da_graph *g_a, const float *x_init_a, float *x_final_a,
                             void *workspace_a, size_t workspace_a_bytes,
                             const da_graph *g_b, const float *x_init_b, float *x_final_b,
                             void *workspace_b, size_t workspace_b_bytes,
                             float *traj_a, float *traj_b, size_t traj_stride, void *stream);
/* ... and with the samplers of da_sample_loop_ex on both branches (ABI 17; spatial_diffusion.py:485-510,568-589,620-627):
 * `opts` as there, with opts->noise = half a's noise rows and noise_b = half b's, iteration i read at + i * noise_stride floats
 * (normally row ranges of ONE [n_iters, N, c] draw: noise_b = opts->noise + n_real_a * c, noise_stride = N * c -- the poses then
 * equal the one-branch loop's bit for bit).  opts == NULL is da_sample_loop_pair_traj. */
int da_sample_loop_pair_ex(da_denoiser *d, const da_schedule *s, int mean_type, int inference_ratio,
                           int max_iters,
                           const da_graph *g_a, const float *x_init_a, float *x_final_a,
                           void *workspace_a, size_t workspace_a_bytes,
                           const da_graph *g_b, const float *x_init_b, float *x_final_b,
                           void *workspace_b, size_t workspace_b_bytes,
                           float *traj_a, float *traj_b, size_t traj_stride,
                           const da_loop_opts *opts, const float *noise_b, size_t noise_stride, void *stream);

/* ---------------------------------------------------------------------------------------
 * Discrete position diffusion (D3PM with the uniform transition; model/spatial_diffusion_discrete.py over
 * backbones/efficient_gat_discrete.py).  Pieces carry a position INDEX in [0, K); the denoiser returns K logits per piece.
 *
 * The reference stores Q_onestep, its transpose and overline_Q as [steps, K, K] fp32 tables and calls torch.linalg.inv on a
 * [N, K, K] batch per sampling step (:68-82, :209-212).  For Q_t = (1 - beta_t) I + beta_t / K 11^T these have a closed form:
 * overline_Q[t] = a_t I + (1 - a_t) / K 11^T with a_t = alphas_cumprod[t], and for p < t
 * overline_Q[t] overline_Q[p]^-1 = r I + (1 - r) / K 11^T with r = a_t / a_p.  The library evaluates that form in fp32 from
 * da_schedule.alphas_cumprod: no K x K object exists (documented deviation: the reference's fp32 matrix products and inverse
 * lose digits the closed form keeps).
 * ------------------------------------------------------------------------------------- */
/* One denoiser forward == Eff_GAT_Discrete.forward_with_feats (efficient_gat_discrete.py:72-97), encoder bypassed.
 *   idx    [n_real] int32 position indices; values outside [0, K) are clamped (as t is)
 *   t      [n_real] int64 or NULL => t_scalar;  logits [n_real, K] fp32;  alpha as da_denoiser_forward                    */
int da_denoiser_forward_idx(da_denoiser *d, const da_graph *g, const int32_t *idx, const int64_t *t, int64_t t_scalar,
                            float *logits, float *alpha, int alpha_all_layers, void *workspace, size_t workspace_bytes,
                            void *stream);

/* The categorical reverse step == p_sample_ddpm after the model call (spatial_diffusion_discrete.py:282-320) with
 * q_posterior_logits (:193-227).  With p = t - inference_ratio and pi = softmax(logits):
 *   t == 0 : x_prev = argmax_k logits[k]                                  (no posterior, no noise)
 *   t  > 0 : post[k] = log(r [k == x_t] + (1 - r) / K + 1e-8) + log(a_p pi[k] + (1 - a_p) / K + 1e-8)
 *            x_prev  = argmax_k (post[k] - log(-log(clip(u[k], FLT_MIN, 1))))     the lowest index wins a tie
 *   x_t [n] int32, logits [n, K] fp32, t per node or NULL => t_scalar, x_prev [n] int32; 2 <= K <= 1024.
 *   noise  [n, K] fp32 uniforms, or NULL: the step draws them itself from `seed` (device, {seed, offset}; da_d3pm_noise)
 *   post   NULL or [n, K] fp32: post[] before the Gumbel term (the logits where t == 0), for tests
 * A scalar t with 0 < t < inference_ratio is an error (t - ratio < 0 has no posterior; the reference's loop never asks for it);
 * with per-node t the same condition is a precondition the caller keeps (such a row is evaluated with p = 0).           */
int da_d3pm_step(const da_schedule *s, int n, int K, const int32_t *x_t, const float *logits, const int64_t *t,
                 int64_t t_scalar, int inference_ratio, const float *noise, const uint64_t *seed, int iteration,
                 int32_t *x_prev, float *post, void *stream);

/* The uniforms da_d3pm_step / da_sample_loop_idx draw when no noise buffer is given, written out (same device function):
 * Philox4x32-10, key = the two halves of seed[0], counter = (r K + k + seed[1] as 64 bits, iteration, a constant),
 * u = ((bits >> 8) + 1) 2^-24 in (0, 1].  u [n, K] fp32.                                                                  */
int da_d3pm_noise(const uint64_t *seed, int iteration, int n, int K, float *u, void *stream);
/* ... and of a named draw DOMAIN (additive to ABI 19): the reverse step's Gumbel uniforms (da_d3pm_noise) or the training-side
 * noising of da_d3pm_q_sample.  The two use different counter constants, so one seed never gives both the same stream.
 * (A third domain, DA_D3PM_DRAW_SAMPLING_ROT = 2, is declared with the position + rotation model below.)                  */
enum { DA_D3PM_DRAW_SAMPLING = 0, DA_D3PM_DRAW_TRAINING = 1 };
int da_d3pm_noise_ex(const uint64_t *seed, int iteration, int n, int K, int domain, float *u, void *stream);

/* The whole discrete sampling loop == p_sample_loop (spatial_diffusion_discrete.py:324-356): for i in reversed(range(0, steps,
 * ratio)): forward (a second one over zero piece features under classifier-free guidance, logits = (1 + w) cond - w uncond,
 * :285-300) and the reverse step, the K-wide head, guidance, softmax, posterior, Gumbel term and argmax in ONE kernel per step
 * (the [n_real, K] logits never reach memory).  idx_init [n_real] int32; traj (nullable) [n_iters, n_real] int32 receives every
 * step's indices, idx_final (nullable) the last.  Same hipGraph cache and capture rules as da_sample_loop_ex: recorded once,
 * keyed on the arguments, eager while profiling, enqueued directly when the caller is capturing `stream`.
 *   opts->noise  [n_iters, n_real, K] uniforms (parity tests), or NULL: drawn from opts->seed with iteration = the loop index
 *   opts->seed   device {seed, offset}, read BY THE KERNELS: a replayed graph draws fresh numbers once the host has rewritten
 *                those 16 bytes.  One of noise / seed is required.                                                        */
typedef struct da_d3pm_opts {
    int32_t cfg;          /* != 0: classifier-free guidance                                           */
    float cfg_w;          /* classifier_free_w                                                        */
    const float *noise;   /* [n_iters, n_real, K] or NULL                                             */
    const uint64_t *seed; /* device {seed, offset} or NULL                                            */
} da_d3pm_opts;
int da_sample_loop_idx(da_denoiser *d, const da_graph *g, const da_schedule *s, int inference_ratio, int max_iters,
                       const int32_t *idx_init, int32_t *traj, int32_t *idx_final, void *workspace, size_t workspace_bytes,
                       int use_graph, const da_d3pm_opts *opts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Discrete position + rotation diffusion (model/spatial_diffusion_discrete_rot.py over
 * backbones/efficient_gat_discrete_rotation.py; additive to ABI 19).  Besides its position index every piece carries a rotation
 * in {0, 1, 2, 3} with a second categorical reverse process (rot_K = 4, the same uniform transition), and the sampling loop
 * accumulates the sampled rotations into rot_acc = (rot_acc + rot) % 4.  The reference rotates the crops by -rot_acc and
 * re-encodes them every step (:353, :373); rot_acc takes four values per piece, so a Batch has FOUR feature images:
 *   feats4 [4, n_real, F] fp32, image r = visual_features(rotate_images(cond, -r))
 * da_denoiser_set_features_rot projects each image through the feature columns of mlp.0 once (the hoist of
 * da_denoiser_set_features, four times); per step the embedding kernel copies row rot_acc[piece] of those four projections into
 * the addend of the K = 64 mlp.0 product.  Denoisers / precisions without that hoisted product (da_denoiser_flags bit 3 clear)
 * are an error in every entry of this section.
 *   rot_acc  [n_real] int32 in {0..3} (values are taken mod 4), or NULL = image 0 for every piece
 *   logits [n_real, K], rot_logits [n_real, 4] fp32.  The network does not read the rotation state itself
 *   (forward_with_feats:87-115): it enters the rotation posterior only, as x_t.                                            */
int da_denoiser_set_features_rot(da_denoiser *d, const da_graph *g, const float *feats4, void *workspace, size_t workspace_bytes,
                                 void *stream);
int da_denoiser_forward_rot(da_denoiser *d, const da_graph *g, const int32_t *idx, const int32_t *rot_acc, const int64_t *t,
                            int64_t t_scalar, float *logits, float *rot_logits, float *alpha, int alpha_all_layers,
                            void *workspace, size_t workspace_bytes, void *stream);

/* p_sample_ddpm after the model call (spatial_diffusion_discrete_rot.py:288-330).  The position half is exactly da_d3pm_step
 * (x_t, logits, noise_x -> x_prev, post_x); the rotation half is the same formula with K = 4 over rot_t / rot_logits / noise_rot
 * -> rot_prev, post_rot; rot_0 = argmax of the raw rot_logits (lowest index wins).  Without noise buffers the position uniforms
 * are those of da_d3pm_noise and the rotation uniforms come from the draw domain DA_D3PM_DRAW_SAMPLING_ROT (its own counter
 * word, flat element r * 4 + k).  rot_0 / rot_prev / post_x / post_rot are nullable.                                        */
int da_d3pm_rot_step(const da_schedule *s, int n, int K, const int32_t *x_t, const int32_t *rot_t, const float *logits,
                     const float *rot_logits, const int64_t *t, int64_t t_scalar, int inference_ratio, const float *noise_x,
                     const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_prev, int32_t *rot_0,
                     int32_t *rot_prev, float *post_x, float *post_rot, void *stream);
enum { DA_D3PM_DRAW_SAMPLING_ROT = 2 };          /* da_d3pm_noise_ex: the rotation half's uniforms, [n, 4] */

/* The whole loop == p_sample_loop (spatial_diffusion_discrete_rot.py:334-375): per step the embedding (with the addend-row
 * select), the shared body, the two first head layers as one 64-wide product, and ONE tail kernel: both heads, both posteriors,
 * Gumbel terms, argmax, and the state update  rot = cold ? rot_prev : rot_0,  rot_acc = (rot_acc + rot) % 4.
 * idx_init / rot_init [n_real] int32 (the reference's two randint draws); traj_idx / traj_rot_acc (nullable) [n_iters, n_real]
 * int32 receive every step's (index, rot_acc); idx_final / rot_acc_final (nullable) the last.  hipGraph cache and capture rules
 * of da_sample_loop_idx.                                                                                                    */
typedef struct da_d3pm_rot_opts {
    int32_t cold;             /* cold_diffusion: the rotation state follows rot_prev (sampled), else rot_0 (argmax)       */
    int32_t reserved0;
    const int32_t *x_fixed;   /* [n_real] or NULL; only_rotation: every step's INPUT index (the returned one is the sample) */
    const float *noise_x;     /* [n_iters, n_real, K] or NULL                                                              */
    const float *noise_rot;   /* [n_iters, n_real, 4] or NULL (read only when cold != 0)                                   */
    const uint64_t *seed;     /* device {seed, offset}; required where a noise buffer is missing                           */
} da_d3pm_rot_opts;
int da_sample_loop_rot(da_denoiser *d, const da_graph *g, const da_schedule *s, int inference_ratio, int max_iters,
                       const int32_t *idx_init, const int32_t *rot_init, int32_t *traj_idx, int32_t *traj_rot_acc,
                       int32_t *idx_final, int32_t *rot_acc_final, void *workspace, size_t workspace_bytes, int use_graph,
                       const da_d3pm_rot_opts *opts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Measurement aid (no reference counterpart: the reference has no profiler hooks).
 * While enabled, every kernel launch of da_denoiser_forward / da_sample_loop is bracketed by
 * a hipEvent pair on the launch stream (the loop then runs eagerly, not as a hipGraph).
 * da_profile_read synchronises, returns the summed milliseconds and launch counts per class
 * and resets the pool.
 * ------------------------------------------------------------------------------------- */
enum {
    DA_PROF_EMBED = 0,        /* pose MLP + timestep lookup                                  */
    DA_PROF_LINEAR_MLP = 1,   /* mlp.0 / mlp.2                                               */
    DA_PROF_LINEAR_QKVS = 2,  /* fused Q|K|V|skip projections                                */
    DA_PROF_ATTN_HIDDEN = 3,  /* attention of convs 0..n-2 (C = 32)                          */
    DA_PROF_ATTN_LAST = 4,    /* attention of the last conv (C = D/8)                        */
    DA_PROF_HEAD = 5,         /* pose head                                                   */
    DA_PROF_UPDATE = 6,       /* DDIM / DDPM update                                          */
    DA_PROF_CONV_FUSED = 7,   /* hidden conv as ONE kernel: projection + attention (C = 32)  */
                              /* DA_ARCH_GCN: its two projections count as LINEAR_QKVS, the aggregation of conv 0
                               * as ATTN_HIDDEN and that of conv 1 as ATTN_LAST (the classes of the layer's slots)  */
    DA_PROF_NCLASS = 8
};
int da_profile_enable(da_denoiser *d, int on);
int da_profile_read(da_denoiser *d, float *ms /* [DA_PROF_NCLASS] host */,
                    int32_t *counts /* [DA_PROF_NCLASS] host */);

/* ---------------------------------------------------------------------------------------
 * Kernel-level entry points (used by the kernel parity tests and the training autograd).
 * ------------------------------------------------------------------------------------- */
/* out[M, ldo] = act(A[M, K] @ W[Nout, K]^T + bias) (+ residual[M, ldo]); A, W, out, residual
 * in act dtype `prec`, bias fp32.  Replaces torch.nn.Linear on the path.                   */
int da_linear(int prec, int M, int K, int Nout, const void *A, int lda, const void *W,
              const float *bias, int act, const void *residual, void *out, int ldo, void *stream);

/* The same layer with a constant weight packed ONCE into the fragment order of the row-panel kernel
 * (da_gemm_xpanel.hip: bf16, K in {128, 256}, 512 <= Nout <= 4096, Nout % 32 == 0) -- what the denoiser does with
 * its Q | K | V | skip projection weights at da_denoiser_create.  da_linear_packed_bytes returns 0 when the shape has
 * no packed form; da_linear_packed falls back to da_linear's kernels when the row-panel kernel does not apply (short
 * inputs, a residual) and gives the same values as da_linear up to the order of the fp32 bias addition.            */
size_t da_linear_packed_bytes(int prec, int K, int Nout);
int da_linear_pack(int prec, int K, int Nout, const void *W, int ldw /* 0 = K */, void *packed, void *stream);
int da_linear_packed(int prec, int M, int K, int Nout, const void *A, int lda, const void *W, const void *packed,
                     const float *bias, int act, const void *residual, void *out, int ldo, void *stream);

/* One PyG TransformerConv attention (Transformer_GNN.py:32,38) over a CSR graph:
 *   qkvs [n_nodes, 4*H*C] act dtype (Q | K | V | skip), out [n_nodes, H*C] act dtype
 *   out_i = sum_e softmax_i(q_i.k_j / sqrt(C)) v_j + skip_i (+ residual_i) ; act applied last.
 *   alpha (nullable) [n_edges, H] fp32 in caller edge order via g->edge_id.                */
int da_attn_csr(int prec, const da_graph *g, int heads, int C, const void *qkvs, const void *residual,
                int act, void *out, float *alpha, void *stream);

/* The same layer through the dense block-diagonal MFMA path (g->dense != 0): fused projection
 * qkvs = x[n_nodes, Din] @ w[4*H*C, Din]^T + b scattered into head-major Q / K / V, then the
 * flash-style attention kernel.  scratch: caller memory of da_attn_dense_scratch_bytes()
 * (regions Q | K | V | skip, and for C = 144 room for a weight image of da_conv_dense_ex behind them),
 * zero-filled once by the caller before first use.  Returns nonzero (and an error text) if the
 * shape is not supported by the dense kernels.                                              */
size_t da_attn_dense_scratch_bytes(int prec, const da_graph *g, int heads, int C);
int da_conv_dense(int prec, const da_graph *g, int heads, int C, int Din, const void *x, const void *w,
                  const float *b, const void *residual, int act, void *out, void *scratch, void *stream);

/* The same layer in the two forms the packed denoiser runs it in (da_denoiser_create): with the Q rows of w / b
 * PRE-SCALED by log2(e) / sqrt(C) (DA_CONV_Q_PRESCALED: the attention kernels then take their shift-free softmax paths --
 * exp2 of the raw scores, verified row sums, running-max fallback), and with the value heads FOLDED to 32 channels
 * (DA_CONV_FOLDED_V32, C = 144: w = Wq | Wk | V' [2*H*C + H*32, Din], no skip; out = [H][n_real][32] per-head normalised
 * sum_j softmax_j(q_i.k_j / sqrt(C)) v'_j in the act dtype -- the last conv of the 2D transformer arch composed with
 * final_mlp.0).  With disable_folds bit 256 clear (read per call) the folded layer of a complete graph runs as the
 * sampling loop runs it: the projection kernel writes the K | V' columns only, the attention kernel projects Q per 32-query slab
 * in its prologue -- the scratch's Q region is neither written nor read, da_debug_counters [DA_DBG_LAST_QPROJ_LAUNCHES] counts
 * the launch; bit-identical outputs.  Also takes hybrid graphs (adjacency mask + remainder CSR of g).  No reference counterpart
 * beyond da_conv_dense's (Transformer_GNN.py:32,38): kernel-level test entry for those paths.                          */
#define DA_CONV_Q_PRESCALED 1
#define DA_CONV_FOLDED_V32 2
/* Where the call takes the projection in the attention kernel's prologue (large complete graphs, disable_folds bit 64 clear), the
 * layer's rows in the MFMA operand order two such layers hand them over in inside the denoiser (disable_folds bit 128 clear):
 * 16-byte piece [16 s + 8 half .. + 7] of PADDED slot row r (plan->row_map) of a [n_pad][L] bf16 buffer at byte
 * ((r >> 5) * (L / 16) + s) * 1024 + (half * 32 + (r & 31)) * 16.  DA_CONV_X_FM: x is such a buffer (L = Din; rows behind a
 * graph inside its last 32-row slab may hold anything); DA_CONV_OUT_FM: out is written so (L = H * C; those rows as zeros, slabs
 * behind the graph's last are not touched).  Any other call with one of the two flags is an error.                              */
#define DA_CONV_X_FM 4
#define DA_CONV_OUT_FM 8
int da_conv_dense_ex(int prec, const da_graph *g, int heads, int C, int Din, const void *x, const void *w,
                     const float *b, const void *residual, int act, void *out, void *scratch, int flags,
                     void *stream);

/* Fallback bookkeeping of the shift-free softmax kernels (no reference counterpart; lets a test assert that the branch it
 * aims at really ran): out[k] = events since the last reset.  Synchronises the device.                                  */
enum {
    DA_DBG_OPT_GEN_WORKGROUPS = 0,         /* k_attn_opt workgroups whose optimistic pass failed its verification   */
    DA_DBG_DENSE_FAST_EXITS = 1,           /* k_attn_dense waves that left the shift-free FAST mode                 */
    DA_DBG_DUAL_GEN_SLABS = 2,             /* k_attn_dual query slabs that left FAST mode                            */
    DA_DBG_OPT_MASKED_GEN_WORKGROUPS = 3,  /* adjacency-masked optimistic kernel: workgroups re-run                  */
    DA_DBG_RES_LAUNCHES = 4,               /* launches of the K / V-resident hidden-layer kernel (k_attn_res; its    */
                                           /* per-WAVE re-runs count under DA_DBG_OPT_GEN_WORKGROUPS)                */
    DA_DBG_VIRT_IN_LAUNCH = 5,             /* masked hidden-layer launches that carried the exophormer's virtual rows */
    DA_DBG_RES_PROJ_LAUNCHES = 6,          /* k_attn_res launches that projected Q | K | V | skip of their layer in   */
                                           /* their own prologue (disable_folds bit 64 clear): no projection kernel   */
    DA_DBG_RES_FM_LAUNCHES = 7,            /* ... and of those, the launches that read their input rows fragment-major */
                                           /* (disable_folds bit 128 clear; DA_CONV_X_FM)                             */
    DA_DBG_LAST_QPROJ_LAUNCHES = 8,        /* launches of the folded last layer's attention kernel that projected Q   */
                                           /* in their own prologue (disable_folds bit 256 clear): the projection     */
                                           /* kernel in front wrote the K | V' columns only.  Added behind the first  */
                                           /* eight: da_debug_counters fills as many as the caller has room for (>= 8) */
    DA_DBG_NCOUNTERS = 9
};
int da_debug_counters(int64_t *out /* host [n] */, int n, int reset);

/* ---------------------------------------------------------------------------------------
 * Training: the denoiser forward with saved activations and its backward, fp32.
 * Replaces torch autograd through Eff_GAT.forward_with_feats (efficient_gat.py:121-146) as
 * driven by GNN_Diffusion.p_losses / training_step (spatial_diffusion.py:432-483,707-721); the
 * loss itself (smooth_l1 on [N, c]) and the optimizer stay with the caller, as in the reference.
 *   w      LIVE fp32 parameters (no packing, no copy): per conv layer lin_query | lin_key |
 *          lin_value | lin_skip weights must be contiguous in that order ([4*H*C, Din]), and so
 *          must their biases -- the host keeps the parameters in one flat buffer.
 *   grads  the same struct filled with the gradient pointers (same layout); the library ADDS
 *          into them (zero them per optimizer step).
 *   d_feats nullable [n_real, F]: gradient w.r.t. the piece features, for a trainable encoder.
 * Both denoisers (arch transformer / exophormer / gcn) are implemented; any graph type, through
 * the CSR attention kernels (needs g->out_ptr / g->out_dst).  DA_VARIANT_3D (Eff_GAT_3d, efficient_gat_3d.py:173-220):
 * c_in = 7, x and out are [n_real, 7] (unit quaternion wxyz | translation); mlp is Linear - LeakyReLU(0.2) - Linear -
 * LeakyReLU(0.2); the two heads run as one 512-wide hidden product, so head_w0 | head_r_w0 (mlp_t.0 | mlp_r.0, [256, D]
 * each) must be contiguous in that order and so must head_b0 | head_r_b0 -- in w and in grads; the gradients of the
 * heads go to head_w0/b0, head_w1/b1 (mlp_t) and head_r_w0/b0, head_r_w1/b1 (mlp_r); d_out [n_real, 7] is pulled back
 * through normalize(matrix_to_quaternion(exp(skew(r)))) by da_head3d_backward's kernel.  The conv stack does not depend
 * on the variant.  DA_ARCH_GCN: w->conv_wq / conv_bq per layer
 * (lin.weight, bias) only; complete graphs and banded Exphander plans aggregate in closed form, any other
 * plan over its CSR (by destination forward, by source -- out_ptr / out_dst -- backward).  The forward must precede the
 * backward on the same workspace, with the same weights: besides the activations it leaves the
 * step's weight images there (W^T of every Linear with a dX product; bf16 copies in the bf16 mode),
 * which the backward reads instead of transposing again.
 * Streams: the calls enqueue on `stream`; the weight-gradient products (leaves of the backward)
 * and the forward's weight images run on ONE side stream owned by the library (forked behind an
 * event on `stream`, joined before the call returns control of the gradients: when a forward /
 * backward / backward_stage call returns, everything it enqueued is ordered before whatever the
 * caller enqueues on `stream` next).  DA_TRAIN_SIDE_DW=0 keeps every launch on `stream`.
 * ------------------------------------------------------------------------------------- */
size_t da_train_workspace_bytes(const da_weights *w, const da_graph *g);
/* ABI 18: the size for ONE mode (da_train_workspace_bytes = the exact-fp32 mode's, the larger one).  Hybrid graphs in the
 * bf16-operand mode run flash-style and hold no [n, n] pair matrix: 16 puzzles of 900 pieces need 0.9 GB instead of 3.0 GB.
 * Forward and backward of a step must be given a workspace of at least the size of THEIR mode.                              */
size_t da_train_workspace_bytes_ex(const da_weights *w, const da_graph *g, int mma_precision);
/* mma_precision of the _ex forms: how the matrix-core GEMMs of the step (every Linear forward / dX / dW and the grouped
 * attention GEMMs of complete and hybrid graphs) take their operands.  Storage is fp32 in both modes -- parameters,
 * activations, gradients, the flat buffers the optimizer and the gradient all-reduce see.
 *   DA_TRAIN_MMA_FP32  exact fp32 products (v_mfma_f32_16x16x4_f32): the reference's precision, the mode of the gradient
 *                      fixtures; da_train_forward / da_train_backward are this mode.
 *   DA_TRAIN_MMA_BF16  operands rounded to bf16 (round to nearest even) in registers on their way into the matrix cores,
 *                      products accumulated in fp32 (v_mfma_f32_16x16x16_bf16): what autocast(bfloat16) does to the
 *                      reference's Linear / matmul calls.  Softmax, GELU, bias sums, the CSR edge kernels and the optimizer
 *                      stay fp32.  Use the same mode for the forward and the backward of a step.                       */
#define DA_TRAIN_MMA_FP32 0
#define DA_TRAIN_MMA_BF16 1
int da_train_forward(const da_weights *w, const da_graph *g, const float *x, const int64_t *t,
                     const float *feats, float *out, void *workspace, size_t workspace_bytes,
                     void *stream);
int da_train_backward(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                      const int64_t *t, const float *d_out, float *d_feats, void *workspace,
                      size_t workspace_bytes, void *stream);
int da_train_forward_ex(const da_weights *w, const da_graph *g, const float *x, const int64_t *t,
                        const float *feats, float *out, void *workspace, size_t workspace_bytes,
                        int mma_precision, void *stream);
int da_train_backward_ex(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                         const int64_t *t, const float *d_out, float *d_feats, void *workspace,
                         size_t workspace_bytes, int mma_precision, void *stream);
/* ABI 18: the backward in two halves for a BUCKETED data-parallel exchange (the reference gets this from Lightning's DDP reducer,
 * train_script.py:215-218: gradient buckets all-reduced while the rest of backward still runs).  DA_TRAIN_BWD_EARLY enqueues
 * final_mlp (3D: mlp_t / mlp_r) and the convs L-1 .. 1 -- afterwards their gradients are final and may be exchanged on another stream --,
 * DA_TRAIN_BWD_LATE conv 0, the virtual-node embedding, mlp, pos_mlp, time_emb (and d_feats).  EARLY followed by LATE on one
 * stream enqueues exactly the launches of DA_TRAIN_BWD_ALL (= da_train_backward_ex).                                       */
#define DA_TRAIN_BWD_ALL 0
#define DA_TRAIN_BWD_EARLY 1
#define DA_TRAIN_BWD_LATE 2
int da_train_backward_stage(const da_weights *w, const da_weights *grads, const da_graph *g, const float *x,
                            const int64_t *t, const float *d_out, float *d_feats, void *workspace,
                            size_t workspace_bytes, int mma_precision, int stage, void *stream);

/* The elementwise glue of p_losses as single launches (ABI 19):
 *   da_q_sample  == q_sample, spatial_diffusion.py:421-430: x_noisy = extract(sqrt_alphas_cumprod, t) * x_start
 *                   + extract(sqrt_one_minus_alphas_cumprod, t) * noise  (bit-identical to the torch expression);
 *   da_loss_grad == the loss of p_losses, spatial_diffusion.py:470-480 (kind 0 = F.l1_loss, 1 = F.mse_loss,
 *                   2 = F.smooth_l1_loss, all with mean reduction) AND its gradient with respect to the prediction
 *                   (d_pred [n], for a unit upstream gradient) -- one workgroup, fixed summation order.
 *   x_start, noise, x_noisy: [n, c] fp32; t: [n] int64; target, pred, d_pred: [n] fp32; loss: [1] fp32. */
int da_q_sample(int steps, int n, int c, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod,
                const float *x_start, const float *noise, const int64_t *t, float *x_noisy, void *stream);
int da_loss_grad(int kind, size_t n, const float *target, const float *pred, float *loss, float *d_pred, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training of the discrete position model (additive to ABI 19): spatial_diffusion_discrete.py's q_sample (:181-191), p_losses
 * (:229-273), vb_terms_bpd (:416-472) with q_posterior_logits (:193-227) at previous_t = t - 1 and categorical_kl_logits
 * (:475-488), in the closed form of the uniform transition (no [steps, K, K] table; a_t = alphas_cumprod[t]); fp32, 2 <= K <= 1024,
 * one wave per piece, indices and timesteps clamped as in da_d3pm_step.
 *
 * da_d3pm_q_sample: x_noisy[r] = argmax_k( log(a_t [k == x_start[r]] + (1 - a_t) / K + 1e-9)
 *                                          - log(-log(clip(u[r, k], FLT_MIN, 1))) ), the lowest index wins a tie, the inner
 *   -log u floored at 2^-25 as in da_d3pm_step.  noise [n, K] uniforms (parity tests), or NULL: drawn inside the kernel from
 *   `seed` (device {seed, offset}) and `iteration` in the DA_D3PM_DRAW_TRAINING domain -- no [n, K] buffer exists.
 *
 * da_d3pm_loss: the loss of p_losses AND its gradient with respect to the logits z (for a unit upstream gradient), per piece with
 *   pi = softmax(z), p = t - 1, r = a_t / a_p, c1 = ((a_p - a_t) / a_p) / K, c2 = (1 - a_p) / K, eps = 1e-8:
 *     t > 0 : m[k]  = log(r [k == x_t] + c1 + eps) + log(a_p pi[k] + c2 + eps)                 model posterior logits
 *             q~[k] = log(r [k == x_t] + c1 + eps) + log(a_p [k == x_start] + c2 + eps)       true posterior logits
 *             vb_row = KL(softmax(q~) || softmax(m)) / ln 2      (q from its at most four distinct values)
 *     t == 0: vb_row = -log_softmax(z)[x_start] / ln 2                                        (decoder NLL)
 *     ce_row = -sum_k y[k] log pi[k], y = 0.99 e_{x_start} + 0.01 / K                         (F.cross_entropy, label_smoothing 1e-2)
 *   kind DA_D3PM_LOSS_VB: mean vb_row | _CE: mean ce_row | _HYBRID: lambda mean ce_row + mean vb_row.
 *   loss [3] = {total, mean vb_row, mean ce_row} (a term the kind does not use reads 0); d_logits [n, K] = d total / d z;
 *   row_terms [n, 2] receives {vb_row, ce_row} and feeds the finishing reduction: one workgroup, fixed order, no float atomics.
 *   (The +1e-6 categorical_kl_logits adds to both logit vectors cancels inside the softmaxes and is not reproduced.)          */
enum { DA_D3PM_LOSS_VB = 0, DA_D3PM_LOSS_CE = 1, DA_D3PM_LOSS_HYBRID = 2 };
int da_d3pm_q_sample(const da_schedule *s, int n, int K, const int32_t *x_start, const int64_t *t, const float *noise,
                     const uint64_t *seed, int iteration, int32_t *x_noisy, void *stream);
int da_d3pm_loss(const da_schedule *s, int n, int K, int kind, float lambda, const float *logits, const int32_t *x_start,
                 const int32_t *x_t, const int64_t *t, float *loss, float *d_logits, float *row_terms, void *stream);
/* The discrete denoiser's training forward / backward: da_train_forward_ex / da_train_backward_stage with position indices
 * idx [n_real] int32 where the poses were.  w->variant must be DA_VARIANT_DISCRETE (c_in = 1, c_out = K, arch =
 * DA_ARCH_TRANSFORMER, pos_w1 = pos_mlp.weight [K, 32], pos_w0 / pos_b0 / pos_b1 NULL); the float-pose entries above reject that
 * variant, these reject the others.  out / d_out: logits [n_real, K] and their gradient (caller's buffers: the workspace holds
 * no [n, K] image).  The embedding gradient pos_mlp.weight.grad[idx[r]] += d comb[r, F : F + 32] has one owner per table row
 * and a fixed summation order: it is bit-reproducible.  DA_TRAIN_BWD_EARLY / _LATE keep their meaning (head early,
 * embeddings late); workspace size from da_train_workspace_bytes_ex.                                                        */
int da_train_forward_idx(const da_weights *w, const da_graph *g, const int32_t *idx, const int64_t *t, const float *feats,
                         float *logits, void *workspace, size_t workspace_bytes, int mma_precision, void *stream);
int da_train_backward_idx(const da_weights *w, const da_weights *grads, const da_graph *g, const int32_t *idx,
                          const int64_t *t, const float *d_logits, float *d_feats, void *workspace, size_t workspace_bytes,
                          int mma_precision, int stage, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training of the discrete position + rotation model (additive to ABI 19): p_losses of spatial_diffusion_discrete_rot.py
 * (:161-279).  Two D3PM processes with the uniform transition, K positions and 4 quarter turns; the formulas are those of the
 * section above, evaluated once with K and once with 4.  The network reads neither rot_noisy nor rot_start: they enter the loss.
 *
 * da_d3pm_q_sample_rot: both noisings in one launch, one wave per piece.  The position half is da_d3pm_q_sample (same
 *   expressions, same DA_D3PM_DRAW_TRAINING stream: bit-identical for the same seed); the rotation half is the same formula
 *   over four classes (rot_start taken mod 4), its uniforms noise_rot [n, 4] or drawn in the domain DA_D3PM_DRAW_TRAINING_ROT
 *   (its own counter word, flat element r * 4 + k; da_d3pm_noise_ex writes that stream out).  x_noisy == NULL skips the
 *   position half (only_rotation; x_start / noise_x are then not read).  A missing noise buffer needs `seed`.
 *
 * da_d3pm_rot_loss: both heads' loss AND its gradient with respect to both logits (for unit upstream gradients), per piece:
 *   vb_row and ce_row of da_d3pm_loss for (logits, x_start, x_t) with K classes and for (rot_logits, rot_start, rot_t) with 4.
 *   Label smoothing as the reference has it: kind _CE smooths neither cross entropy, kind _HYBRID smooths the position head's
 *   (label_smoothing 1e-2, y = 0.99 e_{x_start} + 0.01 / K) and not the rotation head's.
 *     x_loss, rot_loss = mean vb_row (_VB) | mean ce_row (_CE) | lambda mean ce_row + mean vb_row (_HYBRID), each from its head
 *   loss [6] = {x_loss, rot_loss, mean x_vb, mean x_ce, mean rot_vb, mean rot_ce} (a term the kind does not use reads 0);
 *   d_logits [n, K] = d x_loss / d logits, d_rot_logits [n, 4] = d rot_loss / d rot_logits (the 1 / n and the weights applied);
 *   row_terms [n, 4] = {x_vb, x_ce, rot_vb, rot_ce} feeds the finishing reduction: one workgroup, fixed order, no float atomics.
 *   logits == NULL (only_rotation): the position half is skipped, d_logits is not touched, loss[0], loss[2], loss[3] read 0
 *   (x_start / x_t / d_logits may then be NULL).                                                                            */
enum { DA_D3PM_DRAW_TRAINING_ROT = 3 };          /* da_d3pm_noise_ex: the rotation half of the training-side noising, [n, 4] */
int da_d3pm_q_sample_rot(const da_schedule *s, int n, int K, const int32_t *x_start, const int32_t *rot_start, const int64_t *t,
                         const float *noise_x, const float *noise_rot, const uint64_t *seed, int iteration, int32_t *x_noisy,
                         int32_t *rot_noisy, void *stream);
int da_d3pm_rot_loss(const da_schedule *s, int n, int K, int kind, float lambda, const float *logits, const float *rot_logits,
                     const int32_t *x_start, const int32_t *x_t, const int32_t *rot_start, const int32_t *rot_t, const int64_t *t,
                     float *loss, float *d_logits, float *d_rot_logits, float *row_terms, void *stream);
/* The two-head denoiser's training forward / backward.  w->variant must be DA_VARIANT_DISCRETE_ROT: everything of
 * DA_VARIANT_DISCRETE plus head_r_w0 / head_r_b0 = final_mlp_rot.0 [32, D] / [32] and head_r_w1 / head_r_b1 = final_mlp_rot.2
 * [4, 32] / [4].  The first layer of both heads is ONE [64, D] product forward and ONE dX / dW product backward, so
 * head_w0 | head_r_w0 and head_b0 | head_r_b0 must each be one gap-free slot in that order (weights, then biases), in `w` and in
 * `grads`.  logits [n_real, K] come from columns 0..31 of the post-GELU rows, rot_logits [n_real, 4] from columns 32..63, both
 * fp32 in both mma_precision modes; they and their gradients are the caller's buffers.  d_logits == NULL (only_rotation) skips
 * the position head's second-layer products and leaves the gradient slots of final_mlp.2 untouched (final_mlp.0's receive zero).
 * The float-pose and the _idx entries reject this variant, these reject every other one, before anything is launched.
 * DA_TRAIN_BWD_EARLY / _LATE keep their meaning (both heads early); workspace size from da_train_workspace_bytes_ex.       */
int da_train_forward_rot(const da_weights *w, const da_graph *g, const int32_t *idx, const int64_t *t, const float *feats,
                         float *logits, float *rot_logits, void *workspace, size_t workspace_bytes, int mma_precision, void *stream);
int da_train_backward_rot(const da_weights *w, const da_weights *grads, const da_graph *g, const int32_t *idx, const int64_t *t,
                          const float *d_logits, const float *d_rot_logits, float *d_feats, void *workspace, size_t workspace_bytes,
                          int mma_precision, int stage, void *stream);

/* The 3D model's training glue (additive to ABI 19):
 *   da_head3d_backward  the pose head's backward on its own: pre [n, 6] = [r | t] (what the head's second Linear layers
 *                       produce), d_out [n, 7] the gradient of [q | t], q = normalize(matrix_to_quaternion(exp(skew(r))))
 *                       -> d_pre [n, 6].  Closed form on the branch the forward takes (w >= 0), series below |r| = 1e-4.
 *   da_q_sample_se3     p_losses' noising, spatial_diffusion_3d_test_double_diffusion.py:421-441, one launch: x_noisy[:, 4:] =
 *                       q_sample of the translation with noise_tr; x_noisy[:, :4] = matrix_to_quaternion(so3_scale(R(x_start),
 *                       sqrt_alphas_cumprod[t]) @ N), N the IGSO(3) draw of IsotropicGaussianSO3(sqrt_one_minus_alphas_cumprod[t])
 *                       .sample() for the given axes (normalised here) and uniforms.  trap [steps, 999]: the normalised
 *                       trapezoid CDF of every timestep (diffassemble_amd.engine.igso3_trap_table, built once per schedule on
 *                       the host).  x_start, x_noisy [n, 7]; t [n] int64; noise_tr, axes [n, 3]; unif [n]; all fp32.
 *                       NOTE: piece i's rotation depends on t[0] as well as on t[i].  The reference gathers the two CDF values of
 *                       the lerp weight with an index of shape [P, 1] along dim 0 of its [999, P] table, i.e. from the FIRST
 *                       piece's column for every piece (distributions.py:516-517); the search itself uses the piece's own row.
 *                       The kernel does the same (weight from row t[0], indices from row t[i]) to reproduce the reference's
 *                       x_noisy; a caller that wants per-piece weights calls it once per distinct t[0].                     */
int da_head3d_backward(int n, const float *pre, const float *d_out, float *d_pre, void *stream);
int da_q_sample_se3(int steps, int n, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, const float *trap,
                    const float *x_start, const int64_t *t, const float *noise_tr, const float *axes, const float *unif,
                    float *x_noisy, void *stream);

/* The 3D model with use_6dof (train_3d.py --use_6dof_rot; additive to ABI 19).  A DA_VARIANT_3D denoiser with c_in = 13 is that mode:
 * pose rows are [quaternion wxyz | translation | a1 | a2] (13 wide), mlp_t.2 (head_w1 / head_b1) is [9, 256] / [9], pos_mlp.0
 * (pos_w0) is [16, 13]; c_out is not read.  da_denoiser_forward's out is [n_real, 13] and its pre_head [n_real, 12] = [r | t9];
 * da_ddim_step takes c = 13 (Gaussian update on columns 4:13, SO(3) update on 0:4); the sampling loops and the training entries
 * take and return 13-wide rows.  c_in = 7 behaves as before; any other c_in of the 3D variant is refused.
 * In this mode da_denoiser_forward's `out` does not depend on `alpha`: a layer whose weights are requested computes them in an
 * edge-list pass of its own and its rows by the kernels it takes without the request (the sampling loop's), so a per-step
 * sampler that collects attention weights reproduces the captured loop bit for bit.
 *   da_head3d_backward_ex      da_head3d_backward with the translation head's width: t_channels = 3 (the same kernel) or 9:
 *                              pre [n, 3 + t_channels], d_out [n, 4 + t_channels] -> d_pre [n, 3 + t_channels]; every translation
 *                              channel passes through.
 *   da_q_sample_se3_6d         da_q_sample_se3 for the mode (:424-431): x_start stays [n, 7]; the Gaussian part is nine wide,
 *                              [translation | R0[:, 0] | R0[:, 1]] with R0 = quaternion_to_matrix(x_start[:, :4]) (its first two
 *                              columns); noise_tr [n, 9]; x_noisy [n, 13] = [noised quaternion | the nine noised channels].
 *   da_rot6d_to_pose           the pose the loss and the evaluation read from a prediction (:480-490, :826-845): pred [n, ld],
 *                              ld >= 13, columns 4:7 (translation) and 7:13 (a1 | a2) are read -> pose7 [n, 7] =
 *                              [matrix_to_quaternion([b1 b2 b3]) | translation], b1 = a1 / max(|a1|, 1e-12), b2 = u / max(|u|, 1e-12)
 *                              with u = a2 - (a2.b1) b1, b3 = b1 x b2 (columns).  fp32, one thread per piece.
 *   da_rot6d_to_pose_backward  d_pose7 [n, 7] -> d_pred [n, 13] (contiguous): columns 0:4 zeros, 4:7 = d_pose7[:, 4:7], 7:13 through
 *                              the quaternion and the Gram-Schmidt step in ONE closed form (the four branches of
 *                              matrix_to_quaternion agree on SO(3), hence so do their differentials along it; da_so3.hip).      */
int da_head3d_backward_ex(int n, int t_channels, const float *pre, const float *d_out, float *d_pre, void *stream);
int da_q_sample_se3_6d(int steps, int n, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod, const float *trap,
                       const float *x_start, const int64_t *t, const float *noise_tr, const float *axes, const float *unif,
                       float *x_noisy, void *stream);
int da_rot6d_to_pose(int n, const float *pred, int ld, float *pose7, void *stream);
int da_rot6d_to_pose_backward(int n, const float *pred, int ld, const float *d_pose7, float *d_pred, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused Adafactor step over the flat parameter / gradient buffers (one call = one optimizer
 * step for every listed tensor, 4 launches, deterministic, no host sync).  Replaces, for the
 * live denoiser parameters, transformers.optimization.Adafactor with the defaults the reference
 * uses (spatial_diffusion.py:701-705): relative step, scale_parameter, no momentum, no decay.
 *   param_table  device array of n_params records {int64 off; int32 rows, cols, factored, pad;
 *                int64 row_off, col_off; int32 blk0, nblk; int64 colpart_off}  (56 bytes)
 *   block_table  device array of n_blocks records {int32 pid, row0, nrows}       (12 bytes)
 *   state        second-moment statistics (row/col EMAs of matrices, full EMA of vectors)
 *   scratch      >= 2*n_blocks + 4*n_params + sum(nblk*cols over matrices) floats
 *   step         1-based step count; matrices must have cols <= 1280.
 * ------------------------------------------------------------------------------------- */
int da_adafactor_step(int n_params, const void *param_table, int n_blocks, const void *block_table,
                      float *flat, const float *flat_grad, float *state, float *scratch,
                      size_t scratch_floats, int step, float eps1, float eps2, float clip_threshold,
                      float decay_rate, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused Adafactor step for any list of fp32 tensors of any rank, addressed by pointer (added under
 * ABI 19, backwards-compatible; one call = one optimizer step for every ACTIVE tensor, 4 launches
 * whatever their number, deterministic two-stage reductions, no host sync).  Replaces, for every
 * trainable tensor outside the flat buffers above (the piece encoder's 5-D group-convolution banks,
 * BatchNorm affines, linear1 / linear2; the fragment encoder), the same
 * transformers.optimization.Adafactor(self.parameters()) of spatial_diffusion.py:701-705, including
 * its treatment of a tensor [..., R, C] as prod(shape[:-2]) independent [R, C] slices for the
 * factored second moment, rms(p) / rms(u) over the whole tensor, and a step count PER tensor that
 * advances only when the tensor has a gradient.
 *   param_table  device array of n_params records {float *p; const float *g; int64 row_off, col_off,
 *                colpart_off, rowpart_off; int32 B, R, C, kind, blk0, nblk, active, rmean_off}
 *                (80 bytes).  kind 0 = unfactored (rank <= 1: B = R = 1, C = numel, v at row_off),
 *                1 = tiny slices (R C <= 64, one lane per slice), 2 = tiles of 16 rows x 1024 columns.
 *                State: row[B][R] at row_off, col[B][C] at col_off (transformers' exp_avg_sq_row /
 *                exp_avg_sq_col, flattened).  active = 0: the tensor is skipped this step.
 *   block_table  device array of n_blocks records {int32 pid, b, r0, nr, c0, nc}   (24 bytes):
 *                kind 0: nr <= 4096 elements from r0; kind 1: nr <= 256 slices from slice r0;
 *                kind 2: rows r0 .. r0+nr (r0 a multiple of 16, nr <= 16) x columns c0 .. c0+nc
 *                (c0 a multiple of 1024, nc <= 1024) of slice b.  A tensor's blocks are contiguous.
 *   job_table    device array of n_jobs records {int32 pid, b, c0}                 (12 bytes):
 *                c0 < 0: the row statistics of slice b (every tensor has the job b = 0, which also
 *                computes its learning rate); c0 >= 0 (kind 2): the 64 columns from c0 of slice b.
 *   steps        [n_params] int32 step counts, advanced here for the active tensors
 *   scratch      >= 2*n_blocks + 4*n_params + n_slices + colpart_floats + rowpart_floats, where
 *                kind-2 tensors own colpart[B][ceil(R/16)][C] and rowpart[B][ceil(C/1024)][R];
 *                scratch[2*n_blocks + 4*pid + 1] holds rms(p) of the last step (transformers' "RMS").
 * ------------------------------------------------------------------------------------- */
int da_adafactor_nd_step(int n_params, const void *param_table, int n_blocks, const void *block_table,
                         int n_jobs, const void *job_table, int *steps, float *state, float *scratch,
                         size_t scratch_floats, int n_slices, size_t colpart_floats, size_t rowpart_floats,
                         float eps1, float eps2, float clip_threshold, float decay_rate, void *stream);

/* ---------------------------------------------------------------------------------------
 * Greedy assignment of predicted positions to grid cells, one workgroup per puzzle, no host sync.
 * Replaces greedy_cost_assignment (spatial_diffusion.py:179-216) as called by validation_step /
 * test_step (:931-955).  Puzzle g owns rows ptr1[g]..ptr1[g+1] of pos1 (row stride ld1 floats, x
 * and y in the first two columns) and rows ptr2[g]..ptr2[g+1] of pos2.  out[ptr1[g] + k] =
 * (row, column, (int64)distance) of the k-th assignment, in the order the reference makes them;
 * indices are local to the puzzle.  Ties: first in row-major order, like the reference.
 * ------------------------------------------------------------------------------------- */
int da_greedy_assign(int n_puzzles, const float *pos1, int ld1, const float *pos2, int ld2,
                     const int32_t *ptr1, const int32_t *ptr2, int max_n, int max_m, long long *out,
                     void *stream);

/* ---------------------------------------------------------------------------------------
 * Puzzle and piece accuracy of a whole 2D Batch in ONE launch, one workgroup per puzzle, no host sync.
 * Replaces the per-puzzle scoring of validation_step / test_step (spatial_diffusion.py:775-856, 915-955): two
 * greedy_cost_assignment calls per puzzle (ground truth -> grid, prediction -> grid), the two sorts by row, the comparison
 * of the assigned cells and, with rotation, the cosine test of columns 2..3.  Puzzle g owns rows ptr_piece[g] ..
 * ptr_piece[g + 1] of pred and gt (row strides ld_pred / ld_gt floats: x, y, then cos, sin) and rows ptr_cell[g] ..
 * ptr_cell[g + 1] of grid (its cell centres; x and y in the first two columns).  Both assignments are da_greedy_assign's,
 * bit for bit: the same fp32 distance, ties -> first in row-major order (smallest piece, then smallest cell), like the
 * reference.  PRECONDITION n_g <= m_g (pieces <= cells) for every puzzle: max_n > max_m is refused here; a puzzle that
 * breaks it inside a ragged Batch gets per_puzzle[g][0] = -1 and none of its other outputs is written.
 * cell_pred / cell_gt [N]: the cell (local index) assigned to each piece, either may be NULL; piece_ok [N] = same cell (and,
 * with rotation, cosine_similarity(pred[i, 2:4], gt[i, 2:4]) > (float)cos(pi / 4), each norm clamped at 1e-8, NaN -> 0);
 * per_puzzle [n_puzzles, 4] = (all_correct, n_ok, n_pos_ok, n_rot_ok).  No allocation, no atomics, launched on `stream`.
 * ------------------------------------------------------------------------------------- */
int da_score2d(int n_puzzles, const float *pred, int ld_pred, const float *gt, int ld_gt, const float *grid, int ld_grid,
               const int32_t *ptr_piece, const int32_t *ptr_cell, int max_n, int max_m, int rotation,
               int32_t *cell_pred, int32_t *cell_gt, uint8_t *piece_ok, int32_t *per_puzzle, void *stream);

/* ---------------------------------------------------------------------------------------
 * The assembled puzzles of a 2D Batch as RGBA pictures: every requested (step, puzzle) frame in ONE launch, one workgroup
 * per 32x32 canvas tile, no atomics, no host sync, no allocation (it borrows every buffer).  Replaces the per-piece PIL
 * compositing of create_image_from_patches (spatial_diffusion.py:1204-1234), which test_step and predict_step call once per
 * loop step and puzzle when save_eval_images is set (:957-971, :1170-1202).
 * Per puzzle g, `puzzles` [n_puzzles, 8] int32 holds: first piece, pieces, rows, cols, the fp32 bits of the x scale
 * (float)(1 - 1 / rows) and of the y scale (float)(1 - 1 / cols) -- rows scales x: the reference's pairing --, and the low
 * and high word of the frame's byte offset inside one step (a multiple of 16).  The canvas is [32 * rows, 32 * cols, 4]
 * uint8, zeros where no piece lies.  Piece p (row p of `patches` [n_pieces, 3, 32, 32] fp32, colour = uint8(trunc(v * 255)),
 * alpha 255) is padded by 7 transparent pixels to 46x46, rotated, and pasted with its alpha as the mask at
 * x_pos = int((pos0 * xscale + 1) * W / 2) - 23, y_pos likewise with pos1, yscale and H (fp32, this order, no FMA, int()
 * truncating toward zero); later pieces lie over earlier ones; everything is clipped.  A piece with a non-finite position is
 * not drawn (the reference raises there).  `poses`: row p of step k starts at poses + k * step_stride + p * ld_pose floats.
 * `coef` [n_steps, n_pieces, 6] int32, or NULL for no rotation: the 16.16 fixed-point inverse map of PIL's nearest-neighbour
 * Image.rotate about (23, 23), a0 .. a5 with source x = (a2 + a0 * dx + a1 * dy) >> 16, source y = (a5 + a3 * dx + a4 * dy)
 * >> 16 for the pixel (dx, dy) of the rotated tile; made on the host (fp64 cos / sin rounded to 15 decimals).
 * `out`: step k's frames start at out + k * step_bytes.  max_tiles = max over the puzzles of rows * cols.
 * da_render2d_frame_bytes: the bytes of one rows x cols frame (0 for a non-positive size).
 * ------------------------------------------------------------------------------------- */
long long da_render2d_frame_bytes(int rows, int cols);
int da_render2d(int n_steps, int n_puzzles, int n_pieces, int max_tiles, const float *patches, const float *poses, int ld_pose,
                long long step_stride, const int32_t *coef, const int32_t *puzzles, long long step_bytes, uint8_t *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * A 2D Batch from whole images: every per-piece tensor in ONE launch, one workgroup per output piece, no atomics, no host
 * sync, no allocation.  Replaces the host loops of dataset/puzzle_dataset.py: divide_images_into_patches (:175-190) and the
 * get() of Puzzle_Dataset (:257-300), Puzzle_Dataset_Pad (zero_margin :326-332), Puzzle_Dataset_ROT_MP (:403-485),
 * Puzzle_Dataset_MP (:507-544) and Puzzle_Dataset_ROT (:580-700) -- per piece an Image.fromarray, a .rotate(r * 90), an
 * np.array and a / 255.  Nothing is drawn here: the turns and the kept cells arrive in `pieces`.
 * `images`: the puzzles' pictures, uint8 HWC RGB of [32 * rows, 32 * cols, 3], image_bytes in all.  `puzzles` [n_puzzles, 8]
 * int32: the low and high word of the picture's byte offset (a multiple of 16), rows, cols, first output piece, pieces
 * present, and the starts of linspace(-1, 1, cols) and linspace(-1, 1, rows) inside `lin` [n_lin] fp32 (torch.linspace's own
 * values: it is not -1 + i * step in fp32).  `pieces` [n_pieces, 4] int32 per OUTPUT piece: puzzle, source cell i * cols + j,
 * quarter turns r in 0 .. 3, 0.  `unit` [256] fp32: uint8 / 255 as torch computes it.
 * patches [n_pieces, views, 3, 32, 32] fp32 (views = 1 or 4): view k = the cell's crop turned counter-clockwise by
 * (r + k) % 4 quarter turns (np.rot90 = PIL.Image.rotate(90 t) of a square tile), colour = unit[byte], then the `padding`
 * outermost pixels (0 .. 16) of every side zeroed.  x [n_pieces, x_cols] fp32 (x_cols = 2 or 4): (x_j, y_i) and, with 4,
 * (cos, sin) = rot as floats.  rot [n_pieces, 2] int64 = one_hot(r) @ [[1, 0], [0, 1], [-1, 0], [0, -1]]; rot_index, indexes
 * (= the cell), batch (= the puzzle): [n_pieces] int64.  Every element of every output is written.  A table entry that
 * points outside the buffers writes nothing for its piece.
 * da_complete_edges: edge_index [2, n_edges] int64 of the Batch's complete graphs with self loops, in the order of
 * dense_to_sparse(torch.ones(n, n)) per puzzle (:280-284, :472-473: source-major), shifted by the puzzle's first piece.
 * `table` [n_puzzles, 3] int64: first edge, first piece, pieces n_g; n_edges = the sum of n_g * n_g.
 * ------------------------------------------------------------------------------------- */
int da_puzzle_batch(int n_puzzles, int n_pieces, const uint8_t *images, long long image_bytes, const int32_t *puzzles,
                    const int32_t *pieces, const float *lin, int n_lin, const float *unit, int padding, int views, int x_cols,
                    float *patches, float *x, long long *rot, long long *rot_index, long long *indexes, long long *batch,
                    void *stream);
int da_complete_edges(int n_puzzles, const long long *table, long long n_edges, long long *edge_index, void *stream);

/* ---------------------------------------------------------------------------------------
 * Resize a Batch's pictures: PIL.Image.resize(size, resample, box) for 8-bit RGB, byte for byte, all pictures in one call, no
 * atomics, no host sync, no allocation, no floating point.  Replaces the img.resize((32 cols, 32 rows)) at the head of every
 * get() of dataset/puzzle_dataset.py (:266, :344, :413, :517 bicubic, :590 Lanczos) and, with `flip` and a second call with a
 * box, the RandomHorizontalFlip / RandomCropAndResizedToOriginal of its augmentations (:155-172).  PIL's method: a horizontal,
 * then a vertical pass, each output byte = clamp((2^21 + sum of byte * coefficient) >> 22, 0, 255) in int32 (arithmetic shift),
 * the horizontal result stored as uint8 before the vertical pass reads it.
 * `src` / `dst`: the packed uint8 HWC RGB pictures, src_bytes / dst_bytes in all.  `tables` [n_table] int32: per axis of a
 * picture a bound table [out, 2] = (first source index, count) and a coefficient table [out, ksize], count <= ksize, made on
 * the host in fp64 (resize2d.py states the rule); a pass that PIL skips is the identity table (first = the index, count 1,
 * coefficient 2^22).  The bounds do not decrease with the output index.
 * `pictures` [n_pictures, 24] int32: 0-1 the low and high word of the picture's byte offset in src, 2 source height, 3 source
 * width, 4-5 byte offset in dst, 6 output height, 7 output width, 8 flip (the OUTPUT is mirrored left to right), 9-11 the
 * horizontal tables: start of the bounds, start of the coefficients (ints into `tables`), ksize, 12-14 the same for the
 * vertical tables, 15 first tile of the fused route, 16 tiles per tile row = ceil(width / 32) (a tile is 64 rows x 32 columns),
 * 17 / 18 first block of the two-pass route's horizontal / vertical launch (256 pixels a block, of [20] x width and of height
 * x width pixels), 19-20 the first source row the vertical pass reads and how many, 21-22 byte offset of the picture's
 * horizontal result [rows [20]][width][3] in the workspace (a multiple of 16), 23 zero.
 * route DA_RESIZE_FUSED: one launch of n_tiles workgroups; every tile's vertical window (source rows) must be at most
 * da_resize2d_window_rows() = 256, a tile whose window is larger writes nothing.  route DA_RESIZE_TWO_PASS: two launches
 * (n_hblocks, n_vblocks) through `workspace`; da_resize2d_workspace_bytes(n, HOST copy of `pictures`) = the sum of
 * 3 * [20] * [7] rounded up to 16 each.  Both routes give the same bytes.  A descriptor that points outside the buffers
 * writes nothing for its picture.
 * ------------------------------------------------------------------------------------- */
#define DA_RESIZE_FUSED 0
#define DA_RESIZE_TWO_PASS 1
int da_resize2d_window_rows(void);
size_t da_resize2d_workspace_bytes(int n_pictures, const int32_t *pictures_host);
int da_resize2d(int n_pictures, const uint8_t *src, long long src_bytes, const int32_t *pictures, const int32_t *tables,
                long long n_table, uint8_t *dst, long long dst_bytes, uint8_t *workspace, size_t workspace_bytes, int route,
                long long n_tiles, long long n_hblocks, long long n_vblocks, void *stream);

/* ---------------------------------------------------------------------------------------
 * A 3D Batch from fragment meshes: the surface samples, the centring, the turn, the shuffle and the fp32 layout of every part in
 * two launches, no atomics, no host sync, no allocation.  Replaces the per-part host loop of dataset/breakingbad_dt.py
 * (:113-149: trimesh.sample.sample_surface, _recenter_pc, _rotate_pc, _shuffle_pc, _pad_data) in fp64 numpy.  Nothing is drawn
 * here: the picks, the barycentric pairs, the turns and the point order are arguments.  All arithmetic is fp64, unfused.
 * The meshes: `vertices` [n_vertices, 3] fp64, `faces` [n_faces, 3] int32 with indices LOCAL to the part, `vert_ptr` / `face_ptr`
 * [n_parts + 1] int64: part s owns the rows vert_ptr[s] .. vert_ptr[s + 1] - 1 (at least one of each).  A face index outside
 * the part is clamped into it; a part whose rows lie outside the buffers is skipped (nothing is written for it).
 * da_mesh_cum_area: cum [n_faces] fp64, per part the inclusive running sum of 0.5 * |(v1 - v0) x (v2 - v0)|, summed in chunks
 * of 256 faces with a carry, in an order that depends on the face count alone (the same bits on every run; not the bits of a
 * sequential sum).
 * da_fragment_batch: one workgroup per OUTPUT part k; `parts` [n_out, 2] int32 = (input part s, object).  The draws are indexed
 * by the INPUT part: u_face [n_parts, n_points] fp64, u_len [n_parts, n_points, 2] fp64, rot [n_parts, 9] fp64 (row-major),
 * perm [n_parts, n_points] int32 (a gather index list, clamped to 0 .. n_points - 1).
 * Point i: pick = u_face[i] * cum[last], face = the first with cum >= pick (NaN ordered last, as numpy.searchsorted does: a
 * non-finite vertex makes the part's points NaN as on the host), clamped to the last; (a, b) = u_len[i], replaced
 * by (|a - 1|, |b - 1|) when a + b > 1; point = (a (v1 - v0) + b (v2 - v0)) + v0.  centroid = (sum of the points, in a fixed
 * order) / n_points.  pcds [n_out, n_points, 3] fp32: row j = fp32(rot @ (point[perm[j]] - centroid)).  x [n_out, 7] fp32 =
 * fp32 of the scalar-first quaternion of rot^T (scipy's from_matrix branch choice and sign), fp32(centroid).  batch [n_out] int64 = the object.  face_index [n_out, n_points] int32 or NULL: the face of point i.
 * n_points is 1 .. 2048: the points wait in LDS as fp64, 24 bytes each, beside 6 KiB of reduction scratch.
 * ------------------------------------------------------------------------------------- */
int da_mesh_cum_area(int n_parts, const double *vertices, long long n_vertices, const int32_t *faces, long long n_faces,
                     const long long *vert_ptr, const long long *face_ptr, double *cum, void *stream);
int da_fragment_batch(int n_out, int n_parts, int n_points, const double *vertices, long long n_vertices, const int32_t *faces,
                      long long n_faces, const long long *vert_ptr, const long long *face_ptr, const double *cum,
                      const int32_t *parts, const double *u_face, const double *u_len, const double *rot,
                      const int32_t *perm, float *pcds, float *x, long long *batch, int32_t *face_index, void *stream);

/* ---------------------------------------------------------------------------------------
 * 2D piece encoder: the P4 group-equivariant ResNet-18 the reference builds
 * for model='resnet18equiv', eval-mode BatchNorm.  Replaces Eff_GAT.visual_features
 * (backbones/efficient_gat.py:149-189) = normalise + ResNet.forward (backbones/resnet_equivariant.py:
 * 93-112) + cat(linear1(out3), linear2(out4)), whose convolutions are groupy's SplitGConv2D
 * (backbones/groupy/gconv/pytorch_gconv/splitgconv2d.py:15-22,70-92).
 *
 * da_encoder_weights holds the PACKED weights (device pointers; built once per checkpoint by the
 * host, diffassemble_amd/encoder.py, from the reference's state-dict tensors):
 *   stem_w [128][27] fp32   rotated filter bank of conv1 (channel o*4+r; taps c*9+ky*3+kx), bn1 folded
 *   stem_b [128]     fp32   folded bn1 bias
 *   conv_w[i] [Cout*4][k*k*Cin*4] act dtype, i in state-dict order (layerL.B.conv1, conv2[, shortcut.0]):
 *             filter bank with the BatchNorm scale folded, K ordered tap-major / channel-minor (NHWC)
 *   conv_b[i] [Cout*4] fp32
 *   lin1_w [544][10*10*256], lin2_w [544][6*6*512] act dtype: linear1 / linear2 re-indexed from the
 *             reference's NCHW flatten to the zero-haloed NHWC maps (halo columns are zero); biases fp32.
 * ------------------------------------------------------------------------------------- */
enum { DA_ENCODER_CONVS = 19, DA_ENCODER_FEATS = 1088 };
typedef struct da_encoder_weights {
    int32_t n_convs;                         /* DA_ENCODER_CONVS                              */
    int32_t reserved0;
    const float *stem_w, *stem_b;
    const void *conv_w[DA_ENCODER_CONVS];
    const float *conv_b[DA_ENCODER_CONVS];
    const void *lin1_w; const float *lin1_b;
    const void *lin2_w; const float *lin2_b;
} da_encoder_weights;

/* Workspace for n_patches pieces processed `chunk` at a time (activations of one chunk + the
 * layer-3 / layer-4 maps of all pieces). */
size_t da_encoder_workspace_bytes(int precision, int n_patches, int chunk);

/* patches [n_patches, 3, 32, 32] fp32 in [0, 1] -> feats [n_patches, 1088] (act dtype, row stride
 * ld_feats elements).  The feature maps carry a zero halo that the kernels never write: pass
 * zero_workspace != 0 on the first call with a (new or foreign-written) workspace, 0 afterwards
 * as long as (precision, n_patches, chunk) stay the same.  Stream-capturable. */
int da_encoder_forward(int precision, const da_encoder_weights *w, int n_patches, const float *patches,
                       void *feats, int ld_feats, void *workspace, size_t workspace_bytes, int chunk,
                       int zero_workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * 3D piece encoder: the reference's vector-neuron DGCNN, eval-mode BatchNorm.
 * Replaces Eff_GAT_3d.pcd_features -> VN_DGCNN.forward (backbones/vnn/vn_dgcnn.py:34-74) with
 * get_graph_feature / knn (:84-120) and VNLinearLeakyReLU / VNBatchNorm (backbones/vnn/vn_layers.py:50-91,
 * 133-154); all fp32.  A stage = kNN(20) in the current feature space -> first VN layer on cat(x_j - x_i, x_i)
 * -> [second VN layer] -> mean over the neighbours; three stages, then conv6 + mean over the points.
 *
 * da_pcd_encoder_weights holds PACKED fp32 device pointers (host: diffassemble_amd/pcd_encoder.py, from the
 * reference's state-dict tensors; Cin = 1, 21, 21 for the three stages, W = map_to_feat / map_to_dir of the
 * stage's first layer, columns [:Cin] act on x_j - x_i and [Cin:] on x_i):
 *   premap[s] [4][21][Cin]    Wf[:, :Cin], Wd[:, :Cin], Wf[:, Cin:] - Wf[:, :Cin], Wd[:, Cin:] - Wd[:, :Cin]
 *   bn_a[s]   [2][21]         eval BatchNorm of the norm as  norm * scale + shift
 *   conv_b[s] [2][21][22] + [2][21]   second layer of the stage: feature map, direction map (rows zero-padded to
 *                             22), then scale, shift; NULL for stage 3 (conv5 stands alone)
 *   conv6     [feat_dim][63] + [63] + [2][feat_dim]   feature map, the ONE shared direction map, scale, shift
 *   linear0   [2 feat_dim][3] + [2 feat_dim]          only read for the invariant output (may be NULL otherwise)
 * ------------------------------------------------------------------------------------- */
enum { DA_PCD_K = 20, DA_PCD_C = 21, DA_PCD_ROW = 64, DA_PCD_STAGES = 3 };
typedef struct da_pcd_encoder_weights {
    int32_t feat_dim;                        /* conv6 output channels (128 in the reference)  */
    int32_t reserved0;
    const float *premap[DA_PCD_STAGES];
    const float *bn_a[DA_PCD_STAGES];
    const float *conv_b[DA_PCD_STAGES];
    const float *conv6;
    const float *linear0;
} da_pcd_encoder_weights;

/* Workspace for fragments of n_points points processed `chunk` at a time. */
size_t da_pcd_encoder_workspace_bytes(int n_points, int chunk, int feat_dim);

/* points [n_parts, n_points, 3] fp32 -> out [n_parts, 6 feat_dim] (inv == 0: the pooled equivariant map twice,
 * vn_dgcnn.py:62-73) or [n_parts, 2 feat_dim] (inv != 0: linear0 path, :68-69); row stride ld_out floats.
 * n_points >= 20.  Stream-capturable. */
int da_pcd_encoder_forward(const da_pcd_encoder_weights *w, int n_parts, int n_points, const float *points, int inv,
                           float *out, int ld_out, void *workspace, size_t workspace_bytes, int chunk, void *stream);

/* The encoder's neighbour search on its own (vn_dgcnn.py:114-120): for every point of every cloud the k nearest
 * points of the same cloud (itself included), nearest first, ties towards the lower index -> idx [n_clouds,
 * n_points, k] (cloud-local).  x rows: dim == 3 with stride ldx >= 3, or 4 <= dim <= 64 as zero-padded 64-float rows. */
int da_knn(int n_clouds, int n_points, int dim, const float *x, int ldx, int k, int32_t *idx, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training path of the 3D piece encoder (SURVEY.md 8f rank 4 in train() mode): VN_DGCNN.forward with batch-statistics
 * BatchNorm (backbones/vnn/vn_dgcnn.py:34-74, vnn/vn_layers.py:50-91 VNLinearLeakyReLU, :133-154 VNBatchNorm: BatchNorm2d
 * over the P*N*20 edges for conv1..conv5, BatchNorm1d over the P*N points for conv6 and over the P fragments for VnInv's
 * vn1 / vn2, :176-240, whose result vn_dgcnn.py:67 discards) and torch autograd through it, down to the point clouds.
 * fp32 throughout; every per-channel sum runs in a fixed order (fp64 across blocks): bitwise reproducible.
 * Layer index l: 0..4 conv1..conv5, 5 conv6, 6 VnInv.vn1, 7 VnInv.vn2.
 * ------------------------------------------------------------------------------------- */
enum { DA_PCD_TRAIN_LAYERS = 8 };
typedef struct da_pcd_train_weights {
    int32_t feat_dim;                        /* conv6 output channels                                     */
    int32_t reserved0;
    const float *premap[DA_PCD_STAGES];      /* as da_pcd_encoder_weights                                 */
    float *bn_a[DA_PCD_STAGES];              /* as da_pcd_encoder_weights; the scale / shift slots of     */
    float *conv_b[DA_PCD_STAGES];            /*   bn_a, conv_b and conv6 are WRITTEN by the train forward */
    float *conv6;                            /*   (batch statistics of the call)                          */
    const float *linear0;                    /* [2 feat][3] + [2 feat]; read for inv only                 */
    const float *gamma[DA_PCD_TRAIN_LAYERS], *beta[DA_PCD_TRAIN_LAYERS];       /* BatchNorm affine           */
    const float *running_mean[DA_PCD_TRAIN_LAYERS], *running_var[DA_PCD_TRAIN_LAYERS];
    float momentum[DA_PCD_TRAIN_LAYERS], eps[DA_PCD_TRAIN_LAYERS];
    const float *inv_wf[2], *inv_wd[2];      /* VnInv.vn{1,2}.map_to_feat / map_to_dir [cout][cin]         */
} da_pcd_train_weights;

/* Parameter gradients in the modules' own layouts ([cout][cin] maps, per-channel affine); every output is ADDED to. */
typedef struct da_pcd_train_grads {
    float *wf[6], *wd[6];                    /* conv1..conv6 map_to_feat / map_to_dir                     */
    float *gamma[6], *beta[6];               /* conv1..conv6 BatchNorm weight / bias                      */
    float *linear0_w, *linear0_b;            /* inv only (may be NULL otherwise)                          */
    float *points;                           /* [n_parts][n_points][3], may be NULL                       */
} da_pcd_train_grads;

/* Saved state of one train forward (what its backward reads): neighbour lists, pooled maps, batch statistics. */
size_t da_pcd_train_state_bytes(int n_parts, int n_points, int feat_dim);
/* Scratch of the forward and of the backward; the backward's per-edge buffers cover `chunk` fragments at a time. */
size_t da_pcd_train_workspace_bytes(int n_parts, int n_points, int chunk, int feat_dim);

/* vn_dgcnn.py:34-74 in train(): points [n_parts, n_points, 3] -> out as da_pcd_encoder_forward.  n_parts >= 2
 * (BatchNorm1d of VnInv over the fragments needs two), n_points >= 20.  run_out [8][2][256]: the updated running mean
 * (row 2 l) and running variance (row 2 l + 1, unbiased batch variance) of layer l, momentum / eps from `w`. */
int da_pcd_train_forward(const da_pcd_train_weights *w, int n_parts, int n_points, const float *points, int inv, float *out,
                         int ld_out, float *run_out, void *state, size_t state_bytes, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Backward of that call (torch autograd of vn_dgcnn.py:34-74 with batch-statistics BatchNorm): grad_out [n_parts, ld_g]
 * -> the parameter and point gradients of `g` (added to).  `w` and `state` as left by the forward (the backward writes
 * its BatchNorm sums into the state's records). */
int da_pcd_train_backward(const da_pcd_train_weights *w, int n_parts, int n_points, const float *points, int inv,
                          const float *grad_out, int ld_g, void *state, const da_pcd_train_grads *g, void *workspace,
                          size_t workspace_bytes, int chunk, void *stream);

/* ---------------------------------------------------------------------------------------
 * Passes of the 3D encoder's training path: ONE pass of da_pcd_train_forward / da_pcd_train_backward on caller-supplied
 * device buffers, through the launch code those two run (same kernel instantiations, same grids).  For kernel-level
 * tests (tests/test_gpu_pcd_train_kernels.py, contracts in tests/golden/pcd_train_kernel_refs.py) and for rewrites of
 * single passes.  No allocation, no synchronisation, every launch on `stream`.  pts = n_parts * n_points; edge e =
 * point * 20 + rank; idx [pts][20] int32, cloud-local.  Layouts (all fp32 unless noted):
 *   T       premap rows [pts][A | Ad | U | Ud], 4 x 64 floats per point, each segment 21 x 3 values (channel-major,
 *           component-minor) + one zero pad: A = Wf[:, :cin] x, Ad = Wd[:, :cin] x, U = (Wf[:, cin:] - Wf[:, :cin]) x, Ud alike;
 *           an edge's first-layer input is p = A_j + U_i, d = Ad_j + Ud_i
 *   rec     stat record of a layer [6][256]: rows mean, rstd, gamma, beta (written by BN_FIN_FWD), mean(dy), mean(dy xhat)
 *           (written by BN_FIN_BWD) of the BatchNorm of the vector norm
 *   partial block partials [block][2][C] in fp64: the two per-channel sums of the block's 256 points (C = 21 for the edge
 *           passes, feat for conv6); a block covers points [256 b, 256 b + 256) of the call
 *   dX      component-major gradient map [pts][3][64]: row (point, k) holds component k of the 21 channels, column 21 is
 *           zero where a pass writes the map; dX_in is the gradient of a stage's POOLED output (the mean over 20 edges)
 *   Gb      [edge * 3 + k][44]: dp_b (21) | dd_b (21) | 2 unwritten;  Hb [edge * 3 + k][24]: layer b's input h (21) | 3 unwritten
 *   E       [edge][128]: dp_a (63: channel-major, component-minor) | 0 | dd_a (63) | 0   (gradients of p, d of layer a)
 *   dTc     [point * 3 + k][84]: the gradient of T's four segments, component-major;  Xc [point * 3 + k][24]: x, cin used
 *   G6      [point * 3 + k][ld_g6], ld_g6 = (feat + 4) & ~3: dp6 (feat) | dd6 (1) | unwritten;  F [point * 3 + k][64]:
 *           cat(x1, x2, x3) component-major (63) | 0
 *   wb      conv_b blob of da_pcd_encoder_weights: [21][22] feature map, [21][22] direction map (+ scale / shift slots)
 *   w6      conv6 blob: [feat][63] feature map, [63] direction map (+ scale / shift slots)
 * Every pass reads only the fields its line names; the others may be NULL / 0.
 * ------------------------------------------------------------------------------------- */
enum {
    DA_PCD_PASS_PREMAP = 0,      /* x (ld_x, cin), w = premap blob [4][21][cin] -> T                                       */
    DA_PCD_PASS_EDGE_STAT_A,     /* T, idx -> partial: sums of |p_a|+eps and its square (has_b selects the instantiation)  */
    DA_PCD_PASS_EDGE_STAT_B,     /* T, idx, rec_a, w = wb -> partial: the same for layer b (has_b must be 1)               */
    DA_PCD_PASS_EDGE_BWD1,       /* T, idx, rec_a[, rec_b, w = wb], dX_in -> partial: sums of dy, dy xhat of the LAST layer */
    DA_PCD_PASS_EDGE_BWD2,       /* (has_b) ... rec_b with its backward means -> Gb, Hb, partial: sums of layer a          */
    DA_PCD_PASS_EDGE_BWD3,       /* ... both records complete -> E                                                         */
    DA_PCD_PASS_C6_STAT,         /* X1, X2, X3 [pts][64], w = w6, feat -> partial [block][2][feat]                         */
    DA_PCD_PASS_C6_BWD1,         /* ... rec_a, dm [n_parts][feat][3] (gradient of the mean over points) -> partial         */
    DA_PCD_PASS_C6_BWD2,         /* ... rec_a complete -> G6 (ld_g), F                                                     */
    DA_PCD_PASS_C6_DX,           /* G6 (ld_g), w = w6, feat -> dX1, dX2, dX3 (written)                                     */
    DA_PCD_PASS_BN_FIN_FWD,      /* partial, nblk, channels, count, gamma, beta, momentum, eps, running_mean, running_var
                                    -> rec_a rows 0..3, run_out [2][256] (mean, unbiased variance blended), ss (may be NULL):
                                    ss[c] = gamma rstd, ss[ld_m + c] = beta - mean gamma rstd                              */
    DA_PCD_PASS_BN_FIN_BWD,      /* partial, nblk, channels, count -> rec_a rows 4, 5; dgamma += sum dy xhat, dbeta += sum dy */
    DA_PCD_PASS_REV_ADJ,         /* idx -> cnt, ptr [pts], rev [pts * 20] (cur [pts]: scratch): for every point the edges
                                    that END in it, ascending; ptr = start in rev, cnt = how many                          */
    DA_PCD_PASS_GATHER,          /* E, cnt, ptr, rev, w = premap blob, x (ld_x, cin) -> dTc, Xc (written), dXp (ADDED to):
                                    cin == 1: [pts][3]; cin == 21: component-major map                                     */
    DA_PCD_PASS_PREMAP_WGRAD,    /* dWm [4][21][cin] -> dwf, dwd [21][2 cin] (ADDED to)                                    */
    DA_PCD_PASS_HEAD_BWD,        /* grad_out [n_parts][ld_g], inv, feat, w = linear0 (inv) -> dm [n_parts][feat][3]        */
    DA_PCD_PASS_LIN0_GRAD,       /* grad_out (ld_g), x = pooled map M (ld_x), feat -> dwf [2 feat][3], dwd [2 feat] (ADDED) */
    DA_PCD_PASS_VN_LIN,          /* x [n_parts] rows of ld_x = [vn_cin][3], w, w2 = map_to_feat / map_to_dir [channels][vn_cin]
                                    -> vP, vD [n_parts][channels][3]                                                       */
    DA_PCD_PASS_VN_STAT,         /* vP -> partial [2][channels] (one block partial)                                        */
    DA_PCD_PASS_VN_APPLY         /* vP, vD, rec_a -> vY [n_parts][channels][3]                                             */
};
typedef struct da_pcd_pass_args {
    int32_t n_parts, n_points;   /* clouds in the buffers, points per cloud (>= 20 for the passes that read idx)          */
    int32_t cin;                 /* channels of the stage's input: 1 (the points, stage 1) or 21                          */
    int32_t feat;                /* conv6 output channels, 2..128                                                         */
    int32_t has_b, inv;
    int32_t channels, nblk;      /* finalisers / VnInv: channel count (<= 256), number of block partials                  */
    int32_t ld_x, ld_g, ld_m;    /* row strides in floats                                                                 */
    int32_t vn_cin;
    double count;                /* finalisers: elements per channel                                                      */
    float momentum, eps;
    const float *x, *w, *w2;
    float *T;
    const int32_t *idx;
    float *rec_a, *rec_b;
    const float *dX_in;
    double *partial;
    float *Gb, *Hb, *E;
    const float *X1, *X2, *X3, *dm_in;
    float *G6, *F, *dX1, *dX2, *dX3;
    const float *gamma, *beta, *running_mean, *running_var;
    float *run_out, *ss, *dgamma, *dbeta;
    int32_t *cnt, *ptr, *cur, *rev;
    float *dXp, *dTc, *Xc;
    const float *dWm;
    float *dwf, *dwd;
    const float *grad_out;
    float *dm;
    float *vP, *vD, *vY;
} da_pcd_pass_args;
int da_pcd_train_pass(int pass, const da_pcd_pass_args *args, void *stream);

/* Nearest-neighbour squared distances both ways (chamfer_distance.py:148-149 = pytorch3d knn_points K = 1, used by
 * utils_3d.py:1089-1129 calc_part_acc): a [n_clouds, n, 3], b [n_clouds, m, 3] -> d_ab [n_clouds, n],
 * d_ba [n_clouds, m]; either output may be NULL. */
int da_nearest_sq(int n_clouds, int n, int m, const float *a, const float *b, float *d_ab, float *d_ba, void *stream);

/* The pose metrics of a whole 3D Batch in two launches (utils_3d.py:362-383 trans_metrics, :415-450 rot_metrics 'rmse' and
 * 'geodesic', :916-945 geodesic_distance, :1089-1129 calc_part_acc, as called per object at
 * spatial_diffusion_3d_test_double_diffusion.py:895-960, 1036-1080).  pred / gt: pose rows (quaternion wxyz | translation)
 * of n_parts parts, row strides ld_pred / ld_gt >= 7; pcds [n_parts, n_points, 3] or NULL; ptr int32 [n_objects + 1]: the
 * parts of object g are rows ptr[g] .. ptr[g + 1] - 1 (ragged; clamped to 0 .. n_parts).
 * per_part [n_parts, 4] = (rmse_t, rmse_r in degrees, gd_r, two-sided mean squared Chamfer distance between the fragment
 * posed with pred and with gt); per_object [n_objects, 4] = the mean over the object's parts of columns 0 .. 2 and
 * part_acc = #{chamfer < thr} / parts.  With pcds == NULL no search runs and both fourth columns are NaN; an object
 * without parts gets a NaN row.  The posed clouds never reach memory.  fp32, no allocation, no synchronisation, both
 * launches on `stream`, no floating-point atomics: bitwise reproducible. */
int da_metrics3d(int n_parts, int n_points, int n_objects, const float *pred, int ld_pred, const float *gt, int ld_gt,
                 const float *pcds, const int32_t *ptr, float thr, float *per_part, float *per_object, void *stream);

/* ---------------------------------------------------------------------------------------
 * The 3D assembly losses of loss_type="all" (model/utils_3d.py:585-890 as called at
 * spatial_diffusion_3d_test_double_diffusion.py:500-562): trans_l2_loss, shape_cd_loss and rot_cosine_loss per shape,
 * and the gradient with respect to the predicted poses.  pts [n_pieces, n_points, 3] (the fragments' own clouds),
 * pred / gt [n_pieces, 7] (quaternion wxyz | translation), piece_map int32 [n_pieces][2] = (shape, slot): the pieces of
 * one shape are consecutive rows with ascending slots, slots 0 .. n_parts - 1 (n_parts <= 64), slots without a piece are
 * the padded parts.  Quaternions go through Rotation3D._process_zero_quat (norm <= 0.5 -> identity, no gradient) and
 * are applied as pytorch3d quaternion_apply does, without normalisation.  The poses are applied inside the kernels;
 * padded parts are not searched: they enter as the single candidate (1e3, 1e3, 1e3).
 * `terms`: which losses to compute (the others read 0); the shape term alone needs pts / dist / idx.
 * No allocation, no synchronisation, every launch on `stream`; no floating-point atomics: bitwise reproducible.
 * ------------------------------------------------------------------------------------- */
enum { DA_LOSS3D_TRANS = 1, DA_LOSS3D_SHAPE_CD = 2, DA_LOSS3D_ROT = 4, DA_LOSS3D_ALL = 7 };
size_t da_loss3d_workspace_bytes(int n_batch, int n_parts, int n_points);
/* dist / idx [2][n_pieces, n_points]: for every point of every piece, the squared distance to the nearest point of the
 * other shape and that point's index slot * n_points + point (ties: lowest index); [0] predicted -> target, [1] target ->
 * predicted.  out [3][n_batch] = trans_l2_loss, shape_cd_loss, rot_cosine_loss per shape, then out[3 n_batch + k] =
 * weight k x the mean of row k over the shapes (3 n_batch + 3 floats; w_trans, w_shape_cd, w_rot: the loss weights).  Sums
 * run in fp64 in a fixed order, each output is rounded once.  The workspace is read again by the backward. */
int da_loss3d_forward(int n_pieces, int n_points, int n_batch, int n_parts, int terms, const float *pts, const float *pred,
                      const float *gt, const int32_t *piece_map, float w_trans, float w_shape_cd, float w_rot, float *dist,
                      int32_t *idx, float *out, void *workspace, size_t workspace_bytes, void *stream);
/* grad_out [3][n_batch] (gradient of the per-shape rows of `out`) -> grad_pred [n_pieces, 7] (overwritten); idx and the
 * workspace as the forward of the same inputs left them.  The target receives no gradient, as in the reference. */
int da_loss3d_backward(int n_pieces, int n_points, int n_batch, int n_parts, int terms, const float *pts, const float *pred,
                       const float *gt, const int32_t *piece_map, const int32_t *idx, const float *grad_out, float *grad_pred,
                       const void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training path of the 2D piece encoder (the encoder runs in EVERY training step,
 * model/spatial_diffusion.py:450): fp32 primitives over the zero-haloed NHWC maps [B][H+2][H+2][C4]
 * (C4 = planes * 4, channel = plane * 4 + rotation; the halo must be zero and is never written).  Together
 * they replace ResNet.forward in train() mode (backbones/resnet_equivariant.py:14-38,93-112: BatchNorm3d on
 * batch statistics) and torch autograd through it, including SplitGConv2D's conv2d / trans_filter
 * (backbones/groupy/gconv/pytorch_gconv/splitgconv2d.py:15-22,70-92).  The network walk is host logic
 * (diffassemble_amd/encoder_train.py).  `scratch`: da_enc_train_scratch_bytes(n_patches) bytes.
 * ------------------------------------------------------------------------------------- */
size_t da_enc_train_scratch_bytes(int n_patches);

/* Y = conv(X, W) + bias [+ res] [ReLU]: the inference kernel unfused.  X [B][Hi+2][Hi+2][Cin], W [Cout][k*k*Cin]
 * (tap-major, channel-minor), Y [B][Hi/stride+2][..][Cout]; k in {1, 3}.  Also the DGRAD of a stride-1
 * convolution when W holds the flipped / transposed bank; `res` (may alias Y) accumulates other paths. */
int da_enc_conv(int precision, int B, const void *X, int Cin, int Hi, const void *W, const float *bias, const void *res,
                void *Y, int Cout, int ksize, int stride, int relu, void *stream);
/* The map-shaped primitives below take `precision` = the STORAGE type of the maps (DA_PREC_F32: the parity mode;
 * DA_PREC_BF16: activations and activation gradients in bf16, all arithmetic and every parameter gradient in fp32). */
/* stem: normalise + P4ConvZ2(3 -> 128 channels, 3x3) + bias [ReLU], patches [B,3,32,32] fp32 -> Y [B][34][34][128] */
int da_enc_stem(int precision, int B, const float *patches, const float *w, const float *bias, void *Y, int relu, void *stream);
/* the stem's input as GEMM rows for its weight gradient: cols [B][34][34][32] (27 taps + zero pad; zero halo) */
int da_enc_stem_im2col(int precision, int B, const float *patches, void *cols, void *stream);
/* nn.BatchNorm3d batch statistics: mean / biased variance per plane over (B, 4, H, W) */
int da_enc_bn_stats(int precision, int B, int H, int C4, const void *Y, float *mean, float *var, void *scratch, void *stream);
/* Z = (Y - mean) * (rsqrt(var + 1e-5) * gamma) + beta [+ res] [ReLU] */
int da_enc_bn_apply(int precision, int B, int H, int C4, const void *Y, const float *mean, const float *var, const float *gamma,
                    const float *beta, const void *res, int relu, void *Z, void *stream);
/* backward of that unit: g = dZ [masked by Z > 0]; dgamma += sum g xhat; dbeta += sum g;
 * dY = gamma rstd (g - mean(g) - xhat mean(g xhat)); dRes = g when non-NULL (gradient of the added tensor) */
int da_enc_bn_backward(int precision, int B, int H, int C4, const void *dZ, const void *Z, const void *Y, const float *mean,
                       const float *var, const float *gamma, int relu, float *dgamma, float *dbeta, void *dY,
                       void *dRes, void *scratch, void *stream);
/* zero-stuffing of a gradient map to twice the resolution (stride-2 layers are differentiated as stride 1) */
int da_enc_upsample2(int precision, int B, int H, int C4, const void *S, void *Up, void *stream);
/* C += A^T B over rows: A [M, N] (lda), B [M, K] (ldb), C [N, K] (ldc); fp32 MFMA, deterministic split over rows.
 * One call per filter tap is a convolution's weight gradient (dY's zero halo makes the haloed maps plain
 * GEMM operands).  scratch: 64 MB. */
int da_gemm_tn_f32(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                   void *scratch, void *stream);
/* the same with bf16 operands (fp32 accumulation and output): v_mfma_f32_32x32x16_bf16, tiles transposed on their way
 * into LDS.  lda / ldb multiples of 8, 16-byte aligned bases. */
int da_gemm_tn_bf16(int M, int N, int K, const void *A, int lda, const void *B, int ldb, float *C, int ldc,
                    void *scratch, void *stream);
/* out[c] += sum_m A[m][c]; scratch: ceil(M / 128) * N floats */
int da_colsum_f32(int M, int N, const float *A, int lda, float *out, void *scratch, void *stream);
/* dW[i] += sum_{r<4} dBank[table[4 i + r]]: backward of the filter-bank gather (trans_filter) */
int da_enc_bank_grad(int n, const int32_t *table, const float *dbank, float *dW, void *stream);

/* ---------------------------------------------------------------------------------------
 * PointNet fragment encoder (backbone="pointnet"; the reference's backbones/pointnet.py:8-43): five 1x1 convolutions
 * 3 -> 64 -> 64 -> 64 -> 128 -> feat_dim without bias, a BatchNorm1d after each, ReLU after the first four, max over
 * the points of a fragment.  fp32 throughout; the 64 / 128-wide layers run on v_mfma_f32_32x32x2_f32 with this wave's
 * weight columns held in registers.  feat_dim: a multiple of 32, at most 128 (the training path: 128).
 * Layer l = 0..4 is conv{l+1} / bn{l+1}; widths DA_PN_WIDTH = 3, 64, 64, 64, 128, feat_dim.
 * ------------------------------------------------------------------------------------- */
enum { DA_PN_LAYERS = 5 };
typedef struct da_pointnet_weights {
    int32_t feat_dim;
    int32_t reserved0;
    const float *w[DA_PN_LAYERS];            /* [cout][cin] row-major, eval BatchNorm's scale folded into the rows */
    const float *b[DA_PN_LAYERS];            /* [cout]: the folded shift  beta - mean * gamma / sqrt(var + eps)   */
} da_pointnet_weights;

/* Scratch of da_pointnet_forward: the partial maxima of fragments that span several workgroups (may be 0). */
size_t da_pointnet_workspace_bytes(int n_parts, int n_points, int feat_dim);

/* eval(): points [n_parts, n_points, 3] fp32 -> out [n_parts, feat_dim], row stride ld_out floats.  n_parts >= 0,
 * n_points >= 1.  ONE launch runs a 64-point tile through all five layers inside the CU and reduces the maximum over a
 * workgroup's points; a fragment cut over several workgroups is finished by a small second pass over `workspace`
 * (no floating-point atomics; the maxima start from -inf).  Stream-capturable. */
int da_pointnet_forward(const da_pointnet_weights *w, int n_parts, int n_points, const float *points, float *out, int ld_out,
                        void *workspace, size_t workspace_bytes, void *stream);

typedef struct da_pointnet_train_weights {
    int32_t feat_dim;
    int32_t reserved0;
    const float *w[DA_PN_LAYERS];            /* conv weights [cout][cin]                                           */
    const float *wt[DA_PN_LAYERS];           /* the same transposed, [cin][cout] (the backward's dX = dY W); wt[0] unused */
    const float *gamma[DA_PN_LAYERS], *beta[DA_PN_LAYERS];
    const float *running_mean[DA_PN_LAYERS], *running_var[DA_PN_LAYERS];
    float momentum[DA_PN_LAYERS], eps[DA_PN_LAYERS];
} da_pointnet_train_weights;

/* Parameter gradients in the module's layouts; every output is ADDED to. */
typedef struct da_pointnet_train_grads {
    float *w[DA_PN_LAYERS], *gamma[DA_PN_LAYERS], *beta[DA_PN_LAYERS];
} da_pointnet_train_grads;

/* Saved state of one train forward: per layer mean / inverse standard deviation / scale / shift, the arg-max point of
 * every (fragment, channel), and the pre-normalisation activations of all five layers (448 floats per point). */
size_t da_pointnet_train_state_bytes(int n_parts, int n_points, int feat_dim);
/* Scratch of the train forward and backward (the backward's two gradient maps, one activation map, split-GEMM partials). */
size_t da_pointnet_train_workspace_bytes(int n_parts, int n_points, int feat_dim);

/* train(): BatchNorm on the statistics of this call's M = n_parts * n_points >= 2 points (mean and biased variance;
 * per-workgroup Welford partials in fp32, combined in one fixed order), out as da_pointnet_forward.  run_out [5][2][128]:
 * the updated running mean (row 2 l) and running variance (row 2 l + 1, from the unbiased batch variance) of layer l.
 * Ties of the maximum go to the lowest point index.  Bitwise reproducible. */
int da_pointnet_train_forward(const da_pointnet_train_weights *w, int n_parts, int n_points, const float *points, float *out,
                              int ld_out, float *run_out, void *state, size_t state_bytes, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Backward of that call: grad_out [n_parts, ld_g] -> the gradients of the five conv weights and (gamma, beta) pairs (added
 * to `g`).  The points get no gradient.  Every row reduction runs in a fixed order: bitwise reproducible. */
int da_pointnet_train_backward(const da_pointnet_train_weights *w, int n_parts, int n_points, const float *points,
                               const float *grad_out, int ld_g, const void *state, const da_pointnet_train_grads *g,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * PointNet++ fragment encoder (backbone="pointnet_plus"; the eval forward of the reference's PointNetPlus with
 * normal_channel=False, backbones/pointnet.py:200-256): sa1 = 512 centres by farthest point sampling, balls of radius 0.2
 * with 32 samples, rows [x_n - centre | x_n] through 6 -> 64 -> 64 -> 128, max per ball; sa2 = 128 centres of those 512,
 * radius 0.4, 64 samples, rows [relative xyz | sa1 feature] through 131 -> 128 -> 128 -> 256; sa3 = all 128 points, rows
 * [xyz | sa2 feature] through 259 -> 256 -> 512 -> 1024, max; head 1024 -> 512 -> 256.  Every layer is followed by an eval
 * BatchNorm (folded into it by the caller) and a ReLU.  fp32 throughout, the products on v_mfma_f32_32x32x2_f32.
 *
 * The selection rule (discrete, hence exact): with d* = fl(p* - q*), d2(p, q) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)).
 * Sampling: dist[n] = 1e10, far = start; for i < npoint: idx[i] = far, dist[n] = min(dist[n], d2(x_n, x_far)), far = the
 * lowest n attaining max dist.  Ball: the members of centre c are the n for which d2(c, x_n) > float(radius^2) is false;
 * the first nsample of them in ascending n, the remaining slots filled with the first member.
 * ------------------------------------------------------------------------------------- */
enum { DA_PNP_LAYERS = 11, DA_PNP_MAX_POINTS = 2048, DA_PNP_OUT = 256 };
typedef struct da_pointnet_plus_weights {
    /* layer 3 s + i = sa{s+1}.mlp_convs.i with mlp_bns.i folded in; 9 = fc1 / bn1, 10 = fc2 / bn2.  w [cout][kp] row-major
     * with the input columns in the kernels' order, zero-padded to kp: sa1.0 [rel xyz | xyz | 0 0] (kp 8); sa2.0 [feature
     * (128) | rel xyz | 0 x 5] (kp 136); sa3.0 [feature (256) | xyz | 0 x 5] (kp 264); every other layer kp = cin. */
    const float *w[DA_PNP_LAYERS];
    const float *b[DA_PNP_LAYERS];           /* [cout]: folded bias (conv bias - mean) * gamma / sqrt(var + eps) + beta */
} da_pointnet_plus_weights;

/* Farthest point sampling of npoint indices out of each fragment's n_points (1 .. 2048) points [n_parts, n_points, 3];
 * start int32 [n_parts] (clamped into range), idx int32 [n_parts, npoint].  One workgroup per fragment. */
int da_pnp_fps(int n_parts, int n_points, int npoint, const float *points, const int32_t *start, int32_t *idx, void *stream);
/* Ball query: centre int32 [n_parts, n_centres] = the centres' indices among the fragment's points;
 * grp int32 [n_parts, n_centres, nsample]. */
int da_pnp_ball_query(int n_parts, int n_points, int n_centres, int nsample, double radius, const float *points,
                      const int32_t *centre, int32_t *grp, void *stream);

/* Scratch of da_pointnet_plus_forward (indices, sa1 / sa2 features, sa3 partial maxima of at most 1024 fragments at a time). */
size_t da_pointnet_plus_workspace_bytes(int n_parts, int n_points);
/* Where the stage tensors of min(n_parts, chunk) fragments lie in that scratch, in bytes from its start: fps1 int32 [.,512],
 * grp1 int32 [.,512,32], fps2 int32 [.,128] (indices among the 512), grp2 int32 [.,128,64] (likewise), l1 f32 [.,512,128],
 * l2 f32 [.,128,256], part f32 [.,4,1024] (sa3's maxima per tile of 32 points) -- the layout the kernels use, for tests that
 * run one stage alone.  Returns the chunk (fragments per pass over the scratch); offsets untouched when n_parts <= 0.
 * (additive to ABI 19) */
int da_pointnet_plus_workspace_offsets(int n_parts, size_t offsets[7]);

/* points [n_parts, n_points, 3] fp32 -> out [n_parts, 256], row stride ld_out floats.  start1 / start2 int32 [n_parts]: the
 * first index of sa1's sampling (among n_points) and of sa2's (among 512).  n_parts == 0 is a no-op; n_points outside
 * 1 .. 2048 is refused.  Allocates nothing, no atomics, bitwise reproducible, a fragment's row independent of n_parts.
 * Stream-capturable. */
int da_pointnet_plus_forward(const da_pointnet_plus_weights *w, int n_parts, int n_points, const float *points,
                             const int32_t *start1, const int32_t *start2, float *out, int ld_out, void *workspace,
                             size_t workspace_bytes, void *stream);
/* The same restricted to the stages of the bit set `stages` (1 sampling-1, 2 ball-1, 4 sa1, 8 sampling-2, 16 ball-2, 32 sa2,
 * 64 sa3, 128 head), on the workspace an earlier full call left: for timing one stage alone. */
int da_pointnet_plus_stages(const da_pointnet_plus_weights *w, int n_parts, int n_points, const float *points,
                            const int32_t *start1, const int32_t *start2, float *out, int ld_out, void *workspace,
                            size_t workspace_bytes, int stages, void *stream);

/* ---------------------------------------------------------------------------------------
 * EfficientNet-B0 piece encoder (model="efficientnet_b0", the default of the reference's train_script.py; what
 * backbones/efficient_gat.py:149-189 keeps of timm's efficientnet_b0 under features_only=True): the eval forward of the stem
 * (3x3 stride 2, 3 -> 32) and of blocks.0 .. blocks.4 over 32 x 32 crops, feature maps 2 (blocks.2.1: 40 x 4 x 4) and 3
 * (blocks.4.2: 112 x 2 x 2) flattened in NCHW order into one row of 640 + 448 = 1088 values.  Every BatchNorm is eval mode,
 * folded into the convolution in front of it by the caller; every activation is SiLU; SE(x) = x sigmoid(W_e SiLU(W_r mean_HW(x)
 * + b_r) + b_e) on the activated depthwise output; a block with stride 1 and equal widths adds its input.  fp32 throughout.
 *
 * Blocks in order (input -> expansion -> output, depthwise kernel / stride, squeeze width, input size): 0 = blocks.0.0
 * 32 -> (none) -> 16, 3 / 1, 8, 16; 1 = 1.0 16 -> 96 -> 24, 3 / 2, 4, 16; 2 = 1.1 24 -> 144 -> 24, 3 / 1, 6, 8; 3 = 2.0
 * 24 -> 144 -> 40, 5 / 2, 6, 8; 4 = 2.1 40 -> 240 -> 40, 5 / 1, 10, 4; 5 = 3.0 40 -> 240 -> 80, 3 / 2, 10, 4; 6, 7 = 3.1, 3.2
 * 80 -> 480 -> 80, 3 / 1, 20, 2; 8 = 4.0 80 -> 480 -> 112, 5 / 1, 20, 2; 9, 10 = 4.1, 4.2 112 -> 672 -> 112, 5 / 1, 28, 2.
 * Below, p(c) = c rounded up to a multiple of 16 (24 -> 32, 40 -> 48); padding rows, columns and biases are ZERO.
 * ------------------------------------------------------------------------------------- */
enum { DA_EFFNET_BLOCKS = 11, DA_EFFNET_OUT = 1088 };
enum { DA_EFFNET_CHUNK = 0, DA_EFFNET_PW_ROWS = 1, DA_EFFNET_PW_COLS = 2 };      /* da_effnet_constant */
typedef struct da_effnet_weights {
    const float *stem_w;                      /* [32][27], column c * 9 + ky * 3 + kx; bn1 folded */
    const float *stem_b;                      /* [32] */
    const float *exp_w[DA_EFFNET_BLOCKS];     /* conv_pw + bn1: [p(mid)][p(in)]; NULL for block 0 */
    const float *exp_b[DA_EFFNET_BLOCKS];     /* [p(mid)] */
    const float *dw_w[DA_EFFNET_BLOCKS];      /* conv_dw + its BatchNorm: [k * k][p(mid)], tap ky * k + kx (block 0: mid = 32) */
    const float *dw_b[DA_EFFNET_BLOCKS];      /* [p(mid)] */
    const float *se_rw[DA_EFFNET_BLOCKS];     /* se.conv_reduce: [r][p(mid)] */
    const float *se_rb[DA_EFFNET_BLOCKS];     /* [r] */
    const float *se_ew[DA_EFFNET_BLOCKS];     /* se.conv_expand TRANSPOSED: [r][p(mid)] */
    const float *se_eb[DA_EFFNET_BLOCKS];     /* [p(mid)] */
    const float *prj_w[DA_EFFNET_BLOCKS];     /* conv_pwl + bn3 (block 0: conv_pw + bn2): [p(out)][p(mid)] */
    const float *prj_b[DA_EFFNET_BLOCKS];     /* [p(out)] */
} da_effnet_weights;

/* The kernels' tiling constants: DA_EFFNET_CHUNK crops per pass over the workspace, DA_EFFNET_PW_ROWS x DA_EFFNET_PW_COLS the
 * output tile of a workgroup of the 1x1 convolutions (rows = crops * H * W).  -1 for an unknown name. */
int da_effnet_constant(int which);

/* Scratch of da_effnet_forward: the activations of at most DA_EFFNET_CHUNK crops, so it stops growing there. */
size_t da_effnet_workspace_bytes(int n_crops);

/* crops [n_crops, 3, 32, 32] fp32 in [0, 1], NOT normalised (the stem subtracts Eff_GAT's mean and divides by its std; the
 * convolution pads the normalised image with zeros) -> out [n_crops, 1088], row stride ld_out floats.  quarter_turns 0 .. 3: the
 * stem reads every crop turned clockwise by that many quarter turns (torch.rot90(crops, -quarter_turns, (2, 3))), bit-equal to
 * encoding the turned crops.  n_crops == 0 is a no-op.  Allocates nothing, no atomics, bitwise reproducible, a crop's row
 * independent of n_crops and of its position in the batch.  Stream-capturable. */
int da_effnet_forward(const da_effnet_weights *w, int n_crops, const float *crops, int quarter_turns, float *out, int ld_out,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same, also writing the eleven block outputs as NCHW taps (taps: HOST array of DA_EFFNET_BLOCKS device pointers, tap b
 * [n_crops, out_b, H_b, W_b] unpadded; NULL = none), restricted to the stages of the bit set `stages` (1 stem, 2 << b block b,
 * 4096 the output row) on the workspace an earlier full call left: for parity per block and for timing one stage alone. */
int da_effnet_forward_taps(const da_effnet_weights *w, int n_crops, const float *crops, int quarter_turns, float *out,
                           int ld_out, void *workspace, size_t workspace_bytes, float *const *taps, int stages, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exphander graphs (dataset/puzzle_dataset.py:115-152 generate_random_regular_graph): the adjacency
 * bit rows of da_graph.mask for n_graphs graphs of n nodes and degree d, from the permutations the generator draws
 * (perms int64 [n_graphs, n]): bit j of row i of graph g = edge j -> i, rows of row_bytes bytes, graph g at
 * g * n * row_bytes.  pos: int32 scratch [n_graphs * n] (receives the inverse permutations).  Two launches. */
int da_expander_mask(int n_graphs, int n, int degree, const int64_t *perms, int32_t *pos, int row_bytes,
                     unsigned char *mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFASSEMBLE_HIP_H */
