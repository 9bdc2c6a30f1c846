"""ctypes binding of libdiffassemble_hip.so (C ABI: include/diffassemble_hip.h).

The product path has NO fallback: if the HIP library is missing or fails to load, every
operator raises.  ``import torch`` happens first on purpose -- PyTorch-ROCm bundles its own
libamdhip64 (SONAME libamdhip64.so.7); loading ours afterwards makes the dynamic loader
bind our DT_NEEDED entry to that already-loaded runtime, so streams and device pointers are
shared with torch instead of living in a second HIP runtime.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

LIB_PATH = os.environ.get("DA_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libdiffassemble_hip.so")
# (DA_LIB_PATH: an alternate BUILD of the same library -- compile-flag A/Bs, tools/build_ab.sh; never a different implementation)
DA_MAX_LAYERS = 8
ABI_VERSION = 19
PREC_F32, PREC_BF16 = 0, 1
VARIANT_2D, VARIANT_3D, VARIANT_DISCRETE, VARIANT_DISCRETE_ROT = 0, 1, 2, 3
ARCH_TRANSFORMER, ARCH_EXOPHORMER, ARCH_GCN = 0, 1, 2
MEAN_EPSILON, MEAN_START_X = 0, 1
ACT_NONE, ACT_GELU, ACT_LEAKY02 = 0, 1, 2
CONV_Q_PRESCALED, CONV_FOLDED_V32 = 1, 2
CONV_X_FM, CONV_OUT_FM = 4, 8          # da_conv_dense_ex: x is / out is written fragment-major over the padded slots (DA_CONV_X_FM / DA_CONV_OUT_FM)
FOLD_ATTN_PROJ, FOLD_X_FM = 64, 128    # da_config.disable_folds: set = keep the projection kernel / keep the hidden layers' rows row-major between them
FOLD_LAST_QPROJ = 256                  # ... set = the folded last layer's projection kernel keeps its Q columns (DA_FOLD_LAST_QPROJ)
TRAIN_MMA_FP32, TRAIN_MMA_BF16 = 0, 1
TRAIN_BWD_ALL, TRAIN_BWD_EARLY, TRAIN_BWD_LATE = 0, 1, 2
D3PM_DRAW_SAMPLING, D3PM_DRAW_TRAINING, D3PM_DRAW_SAMPLING_ROT, D3PM_DRAW_TRAINING_ROT = 0, 1, 2, 3
D3PM_LOSS = {"vb": 0, "cross_entropy": 1, "hybrid": 2}
DBG_COUNTERS = ("opt_gen_workgroups", "dense_fast_exits", "dual_gen_slabs", "opt_masked_gen_workgroups")          # fallback events (indices 0 .. 3)
DBG_LAUNCH_COUNTERS = {"resident_launches": 4, "virtual_rows_in_launch": 5,           # which kernel took a layer (DA_DBG_RES_LAUNCHES, DA_DBG_VIRT_IN_LAUNCH,
                       "resident_projection_launches": 6, "resident_fm_input_launches": 7,     # DA_DBG_RES_PROJ_LAUNCHES, DA_DBG_RES_FM_LAUNCHES,
                       "last_qproj_launches": 8}                                               # DA_DBG_LAST_QPROJ_LAUNCHES)
PROF_CLASSES = ("embed", "linear_mlp", "linear_qkvs", "attn_hidden", "attn_last", "head", "update", "conv_fused")

_fp = C.c_void_p        # device pointers travel as integers
_FPL = _fp * DA_MAX_LAYERS


class DaWeights(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("arch", C.c_int32), ("steps", C.c_int32), ("c_in", C.c_int32),
        ("c_out", C.c_int32), ("feat_dim", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32),
        ("n_layers", C.c_int32), ("virt_nodes", C.c_int32),
        ("time_emb", _fp),
        ("pos_w0", _fp), ("pos_b0", _fp), ("pos_w1", _fp), ("pos_b1", _fp),
        ("mlp_w0", _fp), ("mlp_b0", _fp), ("mlp_w1", _fp), ("mlp_b1", _fp),
        ("conv_wq", _FPL), ("conv_bq", _FPL), ("conv_wk", _FPL), ("conv_bk", _FPL),
        ("conv_wv", _FPL), ("conv_bv", _FPL), ("conv_ws", _FPL), ("conv_bs", _FPL),
        ("virt_emb", _fp),
        ("head_w0", _fp), ("head_b0", _fp), ("head_w1", _fp), ("head_b1", _fp),
        ("head_r_w0", _fp), ("head_r_b0", _fp), ("head_r_w1", _fp), ("head_r_b1", _fp),
    ]


class DaGraph(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("n_real", C.c_int32), ("n_graphs", C.c_int32), ("dense", C.c_int32),
        ("n_edges", C.c_int64),
        ("row_ptr", _fp), ("col_src", _fp), ("edge_id", _fp), ("graph_ptr", _fp),
        ("max_graph_nodes", C.c_int32), ("n_pad", C.c_int32),
        ("pad_ptr", _fp), ("row_map", _fp),
        ("out_ptr", _fp), ("out_dst", _fp),
        ("hybrid", C.c_int32), ("band_degree", C.c_int32),
        ("mask", _fp), ("mask_ptr", _fp), ("irr_row_ptr", _fp), ("irr_col_src", _fp),
        ("slot_node", _fp), ("blk_class", _fp), ("blk_class_ptr", _fp), ("blk_class_stride", C.c_int32), ("reserved1", C.c_int32),
        ("rm_meta", _fp), ("agg_row_ptr", _fp), ("agg_col_src", _fp), ("agg_mult", _fp),
    ]


class DaLoopOpts(C.Structure):
    """da_loop_opts: sampler 0 = DDIM / 1 = DDPM, eta, classifier-free guidance switch + weight, per-iteration noise."""
    _fields_ = [("sampler", C.c_int32), ("eta", C.c_float), ("cfg", C.c_int32), ("cfg_w", C.c_float), ("noise", C.c_void_p)]


class DaD3pmOpts(C.Structure):
    """da_d3pm_opts: classifier-free guidance switch + weight, injected uniforms [n_iters, n_real, K] or the device {seed, offset} pair."""
    _fields_ = [("cfg", C.c_int32), ("cfg_w", C.c_float), ("noise", C.c_void_p), ("seed", C.c_void_p)]


class DaD3pmRotOpts(C.Structure):
    """da_d3pm_rot_opts: cold diffusion switch, the fixed input indices of ``only_rotation``, injected uniforms [n_iters, n_real, K] /
    [n_iters, n_real, 4], the device {seed, offset} pair."""
    _fields_ = [("cold", C.c_int32), ("reserved0", C.c_int32), ("x_fixed", C.c_void_p), ("noise_x", C.c_void_p), ("noise_rot", C.c_void_p),
                ("seed", C.c_void_p)]


class DaSchedule(C.Structure):
    _fields_ = [
        ("steps", C.c_int32),
        ("betas", _fp), ("alphas_cumprod", _fp), ("sqrt_recip_alphas", _fp),
        ("sqrt_recip_alphas_cumprod", _fp), ("sqrt_recipm1_alphas_cumprod", _fp),
        ("sqrt_one_minus_alphas_cumprod", _fp), ("posterior_variance", _fp),
    ]


ENCODER_CONVS, ENCODER_FEATS = 19, 1088


class DaEncoderWeights(C.Structure):
    _fields_ = [
        ("n_convs", C.c_int32), ("reserved0", C.c_int32),
        ("stem_w", _fp), ("stem_b", _fp),
        ("conv_w", _fp * ENCODER_CONVS), ("conv_b", _fp * ENCODER_CONVS),
        ("lin1_w", _fp), ("lin1_b", _fp), ("lin2_w", _fp), ("lin2_b", _fp),
    ]


PCD_STAGES, PCD_K = 3, 20


class DaPcdEncoderWeights(C.Structure):
    _fields_ = [
        ("feat_dim", C.c_int32), ("reserved0", C.c_int32),
        ("premap", _fp * PCD_STAGES), ("bn_a", _fp * PCD_STAGES), ("conv_b", _fp * PCD_STAGES),
        ("conv6", _fp), ("linear0", _fp),
    ]


LOSS3D_TRANS, LOSS3D_SHAPE_CD, LOSS3D_ROT, LOSS3D_ALL = 1, 2, 4, 7
PCD_TRAIN_LAYERS = 8      # conv1..conv6, VnInv.vn1, VnInv.vn2


class DaPcdTrainWeights(C.Structure):
    _fields_ = [
        ("feat_dim", C.c_int32), ("reserved0", C.c_int32),
        ("premap", _fp * PCD_STAGES), ("bn_a", _fp * PCD_STAGES), ("conv_b", _fp * PCD_STAGES),
        ("conv6", _fp), ("linear0", _fp),
        ("gamma", _fp * PCD_TRAIN_LAYERS), ("beta", _fp * PCD_TRAIN_LAYERS),
        ("running_mean", _fp * PCD_TRAIN_LAYERS), ("running_var", _fp * PCD_TRAIN_LAYERS),
        ("momentum", C.c_float * PCD_TRAIN_LAYERS), ("eps", C.c_float * PCD_TRAIN_LAYERS),
        ("inv_wf", _fp * 2), ("inv_wd", _fp * 2),
    ]


class DaPcdTrainGrads(C.Structure):
    _fields_ = [
        ("wf", _fp * 6), ("wd", _fp * 6), ("gamma", _fp * 6), ("beta", _fp * 6),
        ("linear0_w", _fp), ("linear0_b", _fp), ("points", _fp),
    ]


PN_LAYERS = 5             # conv1 / bn1 .. conv5 / bn5 of the PointNet encoder


class DaPointnetWeights(C.Structure):
    _fields_ = [("feat_dim", C.c_int32), ("reserved0", C.c_int32), ("w", _fp * PN_LAYERS), ("b", _fp * PN_LAYERS)]


class DaPointnetTrainWeights(C.Structure):
    _fields_ = [
        ("feat_dim", C.c_int32), ("reserved0", C.c_int32),
        ("w", _fp * PN_LAYERS), ("wt", _fp * PN_LAYERS), ("gamma", _fp * PN_LAYERS), ("beta", _fp * PN_LAYERS),
        ("running_mean", _fp * PN_LAYERS), ("running_var", _fp * PN_LAYERS),
        ("momentum", C.c_float * PN_LAYERS), ("eps", C.c_float * PN_LAYERS),
    ]


PNP_LAYERS = 11           # sa{1,2,3}.mlp_convs.{0,1,2}, fc1, fc2 of the PointNet++ encoder (BatchNorm folded)


class DaPointnetPlusWeights(C.Structure):
    _fields_ = [("w", _fp * PNP_LAYERS), ("b", _fp * PNP_LAYERS)]


EFFNET_BLOCKS, EFFNET_OUT = 11, 1088       # stem + blocks.0.0 .. blocks.4.2 of the EfficientNet-B0 encoder; its output row
EFFNET_CHUNK, EFFNET_PW_ROWS, EFFNET_PW_COLS = 0, 1, 2     # names of da_effnet_constant


class DaEffnetWeights(C.Structure):
    _fields_ = [("stem_w", _fp), ("stem_b", _fp)] + [
        (k, _fp * EFFNET_BLOCKS) for k in ("exp_w", "exp_b", "dw_w", "dw_b", "se_rw", "se_rb", "se_ew", "se_eb", "prj_w", "prj_b")]


class DaPointnetTrainGrads(C.Structure):
    _fields_ = [("w", _fp * PN_LAYERS), ("gamma", _fp * PN_LAYERS), ("beta", _fp * PN_LAYERS)]


# passes of da_pcd_train_pass (include/diffassemble_hip.h, "Passes of the 3D encoder's training path"), enum order
PCD_PASSES = ("PREMAP", "EDGE_STAT_A", "EDGE_STAT_B", "EDGE_BWD1", "EDGE_BWD2", "EDGE_BWD3", "C6_STAT", "C6_BWD1", "C6_BWD2", "C6_DX",
              "BN_FIN_FWD", "BN_FIN_BWD", "REV_ADJ", "GATHER", "PREMAP_WGRAD", "HEAD_BWD", "LIN0_GRAD", "VN_LIN", "VN_STAT", "VN_APPLY")
PCD_PASS = {n: i for i, n in enumerate(PCD_PASSES)}


class DaPcdPassArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("n_parts", "n_points", "cin", "feat", "has_b", "inv", "channels", "nblk", "ld_x", "ld_g", "ld_m",
                                         "vn_cin")]
                + [("count", C.c_double), ("momentum", C.c_float), ("eps", C.c_float)]
                + [(n, _fp) for n in ("x", "w", "w2", "T", "idx", "rec_a", "rec_b", "dX_in", "partial", "Gb", "Hb", "E", "X1", "X2", "X3", "dm_in",
                                      "G6", "F", "dX1", "dX2", "dX3", "gamma", "beta", "running_mean", "running_var", "run_out", "ss",
                                      "dgamma", "dbeta", "cnt", "ptr", "cur", "rev", "dXp", "dTc", "Xc", "dWm", "dwf", "dwd", "grad_out",
                                      "dm", "vP", "vD", "vY")])


def pcd_train_pass(name, stream=None, **fields):
    """Run one pass of the 3D encoder's training path (da_pcd_train_pass): tensors become device pointers, the rest plain fields."""
    a = DaPcdPassArgs()
    keys = dict(DaPcdPassArgs._fields_)
    for k, v in fields.items():
        if k not in keys:
            raise DaError(f"da_pcd_pass_args has no field {k!r}")
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    check(lib().da_pcd_train_pass(PCD_PASS[name], C.byref(a), stream if stream is not None else stream_ptr()))


class DaConfig(C.Structure):
    """include/diffassemble_hip.h `da_config`: the library's switches (one environment variable each, settable at run time)."""
    _fields_ = [(n, C.c_int32) for n in ("struct_bytes", "disable_mfma", "disable_dense", "disable_folds", "attn_level", "xpanel", "tail_next",
                                         "pair_split", "train_attn", "train_side_streams")]


# name -> (restype, argtypes); every symbol include/diffassemble_hip.h declares
PROTOTYPES = {
    "da_abi_version": (C.c_int, []),
    "da_last_error": (C.c_char_p, []),
    "da_config_get": (C.c_int, [C.POINTER(DaConfig)]),
    "da_config_set": (C.c_int, [C.POINTER(DaConfig)]),
    "da_build_flags": (C.c_int, []),
    "da_denoiser_create": (C.c_int, [C.POINTER(DaWeights), C.c_int, _fp, C.POINTER(_fp)]),
    "da_denoiser_destroy": (None, [_fp]),
    "da_denoiser_flags": (C.c_int, [_fp]),
    "da_gcn_dinv": (C.c_int, [C.POINTER(DaGraph), _fp, _fp]),
    "da_gcn_aggregate": (C.c_int, [C.c_int, C.POINTER(DaGraph), C.c_int, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "da_denoiser_workspace_bytes": (C.c_size_t, [_fp, C.POINTER(DaGraph)]),
    "da_denoiser_set_features": (C.c_int, [_fp, C.POINTER(DaGraph), _fp, _fp, C.c_size_t, _fp]),
    "da_denoiser_forward": (C.c_int, [_fp, C.POINTER(DaGraph), _fp, _fp, C.c_int64, _fp, _fp, C.c_int, _fp, _fp,
                                      C.c_size_t, _fp]),
    "da_ddim_step": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp,
                               C.c_int64, C.c_int, C.c_int, C.c_float, _fp, _fp, _fp]),
    "da_ddpm_step": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, C.c_int64, _fp, _fp, _fp]),
    "da_sample_loop": (C.c_int, [_fp, C.POINTER(DaGraph), C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int,
                                 _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]),
    "da_sample_loop_ex": (C.c_int, [_fp, C.POINTER(DaGraph), C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int,
                                    _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, C.POINTER(DaLoopOpts), _fp]),
    "da_sample_loop_pair": (C.c_int, [_fp, C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int,
                                      C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t,
                                      C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t, _fp]),
    "da_sample_loop_pair_traj": (C.c_int, [_fp, C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int,
                                           C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t,
                                           C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t, _fp, _fp, C.c_size_t, _fp]),
    "da_sample_loop_pair_ex": (C.c_int, [_fp, C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int,
                                         C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t,
                                         C.POINTER(DaGraph), _fp, _fp, _fp, C.c_size_t, _fp, _fp, C.c_size_t,
                                         C.POINTER(DaLoopOpts), _fp, C.c_size_t, _fp]),
    "da_denoiser_forward_idx": (C.c_int, [_fp, C.POINTER(DaGraph), _fp, _fp, C.c_int64, _fp, _fp, C.c_int, _fp, C.c_size_t, _fp]),
    "da_d3pm_step": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, C.c_int64, C.c_int, _fp, _fp, C.c_int, _fp, _fp, _fp]),
    "da_d3pm_noise": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "da_d3pm_noise_ex": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp]),
    "da_d3pm_q_sample": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "da_d3pm_loss": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int, C.c_float, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "da_train_forward_idx": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]),
    "da_train_backward_idx": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp,
                                        _fp, C.c_size_t, C.c_int, C.c_int, _fp]),
    "da_d3pm_q_sample_rot": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, _fp, _fp, _fp]),
    "da_d3pm_rot_loss": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, C.c_int, C.c_float, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                   _fp, _fp, _fp]),
    "da_train_forward_rot": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]),
    "da_train_backward_rot": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp, _fp,
                                        _fp, C.c_size_t, C.c_int, C.c_int, _fp]),
    "da_sample_loop_idx": (C.c_int, [_fp, C.POINTER(DaGraph), C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_size_t,
                                     C.c_int, C.POINTER(DaD3pmOpts), _fp]),
    "da_denoiser_set_features_rot": (C.c_int, [_fp, C.POINTER(DaGraph), _fp, _fp, C.c_size_t, _fp]),
    "da_denoiser_forward_rot": (C.c_int, [_fp, C.POINTER(DaGraph), _fp, _fp, _fp, C.c_int64, _fp, _fp, _fp, C.c_int, _fp, C.c_size_t, _fp]),
    "da_d3pm_rot_step": (C.c_int, [C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, C.c_int64, C.c_int, _fp, _fp, _fp, C.c_int,
                                   _fp, _fp, _fp, _fp, _fp, _fp]),
    "da_sample_loop_rot": (C.c_int, [_fp, C.POINTER(DaGraph), C.POINTER(DaSchedule), C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                     C.c_size_t, C.c_int, C.POINTER(DaD3pmRotOpts), _fp]),
    "da_profile_enable": (C.c_int, [_fp, C.c_int]),
    "da_profile_read": (C.c_int, [_fp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "da_linear": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, C.c_int, _fp, _fp,
                            C.c_int, _fp]),
    "da_linear_packed_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_linear_pack": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp]),
    "da_linear_packed": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, _fp, C.c_int, _fp, _fp,
                                   C.c_int, _fp]),
    "da_attn_csr": (C.c_int, [C.c_int, C.POINTER(DaGraph), C.c_int, C.c_int, _fp, _fp, C.c_int, _fp, _fp, _fp]),
    "da_attn_dense_scratch_bytes": (C.c_size_t, [C.c_int, C.POINTER(DaGraph), C.c_int, C.c_int]),
    "da_conv_dense": (C.c_int, [C.c_int, C.POINTER(DaGraph), C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int,
                                _fp, _fp, _fp]),
    "da_conv_dense_ex": (C.c_int, [C.c_int, C.POINTER(DaGraph), C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int,
                                   _fp, _fp, C.c_int, _fp]),
    "da_debug_counters": (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "da_train_workspace_bytes": (C.c_size_t, [C.POINTER(DaWeights), C.POINTER(DaGraph)]),
    "da_train_workspace_bytes_ex": (C.c_size_t, [C.POINTER(DaWeights), C.POINTER(DaGraph), C.c_int]),
    "da_train_forward": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]),
    "da_train_forward_ex": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, _fp]),
    "da_train_backward_ex": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp,
                                       _fp, C.c_size_t, C.c_int, _fp]),
    "da_train_backward_stage": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp,
                                          _fp, C.c_size_t, C.c_int, C.c_int, _fp]),
    "da_q_sample": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "da_loss_grad": (C.c_int, [C.c_int, C.c_size_t, _fp, _fp, _fp, _fp, _fp]),
    "da_head3d_backward": (C.c_int, [C.c_int, _fp, _fp, _fp, _fp]),
    "da_q_sample_se3": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    # the 3D model with use_6dof (additive to ABI 19)
    "da_head3d_backward_ex": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
    "da_q_sample_se3_6d": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "da_rot6d_to_pose": (C.c_int, [C.c_int, _fp, C.c_int, _fp, _fp]),
    "da_rot6d_to_pose_backward": (C.c_int, [C.c_int, _fp, C.c_int, _fp, _fp, _fp]),
    "da_adafactor_step": (C.c_int, [C.c_int, _fp, C.c_int, _fp, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, C.c_float,
                                    C.c_float, C.c_float, C.c_float, _fp]),
    "da_adafactor_nd_step": (C.c_int, [C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, _fp, _fp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t,
                                       C.c_float, C.c_float, C.c_float, C.c_float, _fp]),
    "da_greedy_assign": (C.c_int, [C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, C.c_int, C.c_int, _fp, _fp]),
    "da_score2d": (C.c_int, [C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    "da_render2d_frame_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "da_render2d": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, C.c_int64, _fp, _fp, C.c_int64, _fp, _fp]),
    "da_puzzle_batch": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int64, _fp, _fp, _fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp,
                                  _fp, _fp, _fp]),
    "da_complete_edges": (C.c_int, [C.c_int, _fp, C.c_int64, _fp, _fp]),
    "da_resize2d_window_rows": (C.c_int, []),
    "da_resize2d_workspace_bytes": (C.c_size_t, [C.c_int, _fp]),
    "da_resize2d": (C.c_int, [C.c_int, _fp, C.c_int64, _fp, _fp, C.c_int64, _fp, C.c_int64, _fp, C.c_size_t, C.c_int, C.c_int64, C.c_int64,
                              C.c_int64, _fp]),
    "da_mesh_cum_area": (C.c_int, [C.c_int, _fp, C.c_int64, _fp, C.c_int64, _fp, _fp, _fp, _fp]),
    "da_fragment_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int64, _fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                    _fp, _fp, _fp]),
    "da_encoder_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_encoder_forward": (C.c_int, [C.c_int, C.POINTER(DaEncoderWeights), C.c_int, _fp, _fp, C.c_int, _fp, C.c_size_t,
                                     C.c_int, C.c_int, _fp]),
    "da_pcd_encoder_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_pcd_encoder_forward": (C.c_int, [C.POINTER(DaPcdEncoderWeights), C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp,
                                         C.c_size_t, C.c_int, _fp]),
    "da_pcd_train_state_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_pcd_train_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "da_pcd_train_forward": (C.c_int, [C.POINTER(DaPcdTrainWeights), C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp,
                                       C.c_size_t, _fp, C.c_size_t, _fp]),
    "da_pcd_train_backward": (C.c_int, [C.POINTER(DaPcdTrainWeights), C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp,
                                        C.POINTER(DaPcdTrainGrads), _fp, C.c_size_t, C.c_int, _fp]),
    "da_pcd_train_pass": (C.c_int, [C.c_int, C.POINTER(DaPcdPassArgs), _fp]),
    "da_pointnet_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_pointnet_forward": (C.c_int, [C.POINTER(DaPointnetWeights), C.c_int, C.c_int, _fp, _fp, C.c_int, _fp, C.c_size_t, _fp]),
    "da_pointnet_train_state_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_pointnet_train_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_pointnet_train_forward": (C.c_int, [C.POINTER(DaPointnetTrainWeights), C.c_int, C.c_int, _fp, _fp, C.c_int, _fp, _fp, C.c_size_t,
                                            _fp, C.c_size_t, _fp]),
    "da_pointnet_train_backward": (C.c_int, [C.POINTER(DaPointnetTrainWeights), C.c_int, C.c_int, _fp, _fp, C.c_int, _fp,
                                             C.POINTER(DaPointnetTrainGrads), _fp, C.c_size_t, _fp]),
    "da_pnp_fps": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp]),
    "da_pnp_ball_query": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _fp, _fp, _fp, _fp]),
    "da_pointnet_plus_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "da_pointnet_plus_workspace_offsets": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),      # additive to ABI 19
    "da_pointnet_plus_forward": (C.c_int, [C.POINTER(DaPointnetPlusWeights), C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, _fp, C.c_size_t, _fp]),
    "da_pointnet_plus_stages": (C.c_int, [C.POINTER(DaPointnetPlusWeights), C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, _fp, C.c_size_t,
                                          C.c_int, _fp]),
    "da_effnet_constant": (C.c_int, [C.c_int]),
    "da_effnet_workspace_bytes": (C.c_size_t, [C.c_int]),
    "da_effnet_forward": (C.c_int, [C.POINTER(DaEffnetWeights), C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_size_t, _fp]),
    "da_effnet_forward_taps": (C.c_int, [C.POINTER(DaEffnetWeights), C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_size_t,
                                         C.POINTER(_fp * EFFNET_BLOCKS), C.c_int, _fp]),
    "da_knn": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, _fp]),
    "da_nearest_sq": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    "da_metrics3d": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _fp]),
    "da_loss3d_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "da_loss3d_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_float, C.c_float, C.c_float, _fp, _fp, _fp,
                                    _fp, C.c_size_t, _fp]),
    "da_loss3d_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_size_t, _fp]),
    "da_enc_train_scratch_bytes": (C.c_size_t, [C.c_int]),
    "da_enc_conv": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp]),
    "da_enc_stem": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp, _fp, C.c_int, _fp]),
    "da_enc_stem_im2col": (C.c_int, [C.c_int, C.c_int, _fp, _fp, _fp]),
    "da_enc_bn_stats": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    "da_enc_bn_apply": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, _fp, _fp]),
    "da_enc_bn_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int, _fp, _fp, _fp, _fp, _fp, _fp]),
    "da_enc_upsample2": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp]),
    "da_gemm_tn_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp]),
    "da_gemm_tn_bf16": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, _fp]),
    "da_colsum_f32": (C.c_int, [C.c_int, C.c_int, _fp, C.c_int, _fp, _fp, _fp]),
    "da_enc_bank_grad": (C.c_int, [C.c_int, _fp, _fp, _fp, _fp]),
    "da_expander_mask": (C.c_int, [C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, _fp, _fp]),
    "da_train_backward": (C.c_int, [C.POINTER(DaWeights), C.POINTER(DaWeights), C.POINTER(DaGraph), _fp, _fp, _fp, _fp,
                                    _fp, C.c_size_t, _fp]),
}

_lib = None


class DaError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DaError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  diffassemble_amd has no CPU / eager fallback.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.da_abi_version() != ABI_VERSION:
            raise DaError(f"ABI mismatch: library reports {h.da_abi_version()}")
        _lib = h
    return _lib


def config():
    """The library's current switches as a ``DaConfig``."""
    c = DaConfig()
    check(lib().da_config_get(C.byref(c)))
    return c


def set_config(**fields):
    """Change switches at run time (``set_config(xpanel=0, tail_next=0)``); returns the previous ``DaConfig``.  Takes effect for the calls
    that follow: a denoiser keeps the folds it was created with, a captured loop graph is recorded again under the new switches."""
    old = config()
    new = DaConfig.from_buffer_copy(old)
    for k, v in fields.items():
        if k == "struct_bytes" or k not in dict(DaConfig._fields_):
            raise DaError(f"da_config has no field {k!r}")
        setattr(new, k, int(v))
    check(lib().da_config_set(C.byref(new)))
    return old


def experiments_build():
    """True when the loaded library is the EXPERIMENTS build (DA_EXPERIMENTS=1 python __graft_entry__.py; DA_LIB_PATH=.../lib_exp/...)."""
    return bool(lib().da_build_flags() & 1)


def check(rc):
    if rc != 0:
        raise DaError(f"libdiffassemble_hip error {rc}: {lib().da_last_error().decode(errors='replace')}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
