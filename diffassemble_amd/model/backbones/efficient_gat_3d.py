"""Counterpart of puzzle_diff/model/backbones/efficient_gat_3d.py (``Eff_GAT_3d``)."""
import torch
import torch.nn as nn
from torch import Tensor

from ._denoiser_base import DenoiserBase
from .exophormer_gnn import Exophormer_GNN
from .gcn import GCN
from .Transformer_GNN import Transformer_GNN

_FEAT_DIM = {"pointnet_inv": 1024, "pointnet": 128, "pointnet_plus": 256, "vn_dgcnn": 768,
             "vn_dgcnn_inv": 256, "vnn": 2104}


class Eff_GAT_3d(DenoiserBase):
    variant = "3d"

    def __init__(self, steps, input_channels=7, t_channels=3, r_channels=3, n_layers=4,
                 architecture="transformer", virt_nodes=8, backbone="pointnet", freeze_backbone=False,
                 use_vn_dgcnn_equiv_inv_mp=False, return_attentions=True) -> None:
        super().__init__()
        if use_vn_dgcnn_equiv_inv_mp:
            raise NotImplementedError("use_vn_dgcnn_equiv_inv_mp is False in train_3d.py; not on the path")
        if backbone not in _FEAT_DIM:
            raise Exception(f"Backbone not implemented {backbone}")
        self.use_vn_dgcnn_equiv_inv_mp = False
        # point-cloud encoders (efficient_gat_3d.py:73-97): once per sampling loop, not per step.  The
        # vector-neuron DGCNN the 3D configuration trains with (train_3d.py: backbone="vn_dgcnn") runs in the HIP library
        # (da_pcd_encoder_forward, eval mode), and so do the plain PointNet (da_pointnet_forward; its own default
        # here) and PointNet++ (da_pointnet_plus_forward, eval mode only); pointnet_inv / vnn are not built: pass pcd_feats.
        # `pcd_backbone` is the encoder the training step differentiates and the optimizer steps (pcd_features_train,
        # GNN_Diffusion.configure_optimizers).  PointNet++ has no train() mode yet, so it is no such encoder: it sits in
        # `pcd_encoder`, the inference-only slot, and `pcd_backbone` stays None for it as for the backbones without an encoder.
        # Checkpoints keep the reference's keys either way (`pcd_backbone.*`: the three hooks below).
        self.pcd_backbone = None
        self.pcd_encoder = None
        if backbone in ("vn_dgcnn", "vn_dgcnn_inv"):
            from .vnn.vn_dgcnn import VN_DGCNN
            self.pcd_backbone = VN_DGCNN(feat_dim=128, inv=(backbone == "vn_dgcnn_inv"))
        elif backbone == "pointnet":                   # efficient_gat_3d.py: PointNet(feat_dim=128)
            from .pointnet import PointNet
            self.pcd_backbone = PointNet(feat_dim=128)
        elif backbone == "pointnet_plus":              # efficient_gat_3d.py: PointNetPlus()
            from .pointnet import PointNetPlus
            self.pcd_encoder = PointNetPlus()
            self._register_state_dict_hook(self._encoder_keys_out)
            self._register_load_state_dict_pre_hook(self._encoder_keys_in)
            self.register_load_state_dict_post_hook(self._encoder_keys_reported)
        feat_dim = _FEAT_DIM[backbone]
        self.combined_features_dim = feat_dim + 32 + 32
        self.gnn_feat_dim = self.combined_features_dim
        self.input_channels = input_channels
        self.freeze_backbone = freeze_backbone
        self.return_attentions = return_attentions
        D = self.gnn_feat_dim
        if D % 64 != 0:
            raise NotImplementedError(f"feature width {D} must be a multiple of 64 for 8 heads x C%8==0")
        if architecture == "transformer":
            self.gnn_backbone = Transformer_GNN(D, n_layers=n_layers, hidden_dim=32 * 8, heads=8, output_size=D)
        elif architecture == "exophormer":
            self.gnn_backbone = Exophormer_GNN(D, n_layers=n_layers, hidden_dim=32 * 8, heads=8, output_size=D,
                                               virt_nodes=virt_nodes)
        elif architecture == "gcn":                    # efficient_gat_3d.py:114-119
            self.gnn_backbone = GCN(D, hidden_dim=32 * 8, output_size=D)
        else:
            raise NotImplementedError(f"architecture={architecture!r}: not one of transformer / gcn / exophormer")
        self.time_emb = nn.Embedding(steps, 32)
        self.pos_mlp = nn.Sequential(nn.Linear(input_channels, 16), nn.GELU(), nn.Linear(16, 32))
        self.mlp = nn.Sequential(nn.Linear(D, 256), nn.LeakyReLU(0.2), nn.Linear(256, D), nn.LeakyReLU(0.2))
        self.mlp_t = nn.Sequential(nn.Linear(D, 256), nn.GELU(), nn.Linear(256, t_channels))
        self.mlp_r = nn.Sequential(nn.Linear(D, 256), nn.GELU(), nn.Linear(256, r_channels))

    @staticmethod
    def _encoder_keys_out(module, state_dict, prefix, local_metadata):
        """state_dict(): the inference-only encoder under the reference's name, ``pcd_backbone.*``."""
        Eff_GAT_3d._swap_prefix(state_dict, prefix + "pcd_encoder", prefix + "pcd_backbone")

    def _encoder_keys_in(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """load_state_dict(): a checkpoint's ``pcd_backbone.*`` (the reference's name, and what state_dict() writes) feeds ``pcd_encoder``."""
        self._swap_prefix(state_dict, prefix + "pcd_backbone", prefix + "pcd_encoder")

    @staticmethod
    def _encoder_keys_reported(module, incompatible_keys):
        """Missing keys are reported under the name a checkpoint would hold them by."""
        incompatible_keys.missing_keys[:] = [k.replace("pcd_encoder.", "pcd_backbone.", 1) for k in incompatible_keys.missing_keys]

    @staticmethod
    def _swap_prefix(state_dict, old, new):
        """In place and in order: entries of module ``old`` (keys ``old.*``; in ``_metadata`` also ``old`` itself) become ``new``'s."""
        for d in (state_dict, getattr(state_dict, "_metadata", None)):
            if d is None:
                continue
            items = [(new + k[len(old):] if k == old or k.startswith(old + ".") else k, v) for k, v in d.items()]
            d.clear()
            d.update(items)

    def forward(self, xy_pos, time, pcd, edge_index, batch):
        return self.forward_with_feats(xy_pos, time, edge_index, pcd_feats=self.pcd_features(pcd), batch=batch)

    def forward_with_feats(self, xy_pos: Tensor, time: Tensor, edge_index: Tensor, pcd_feats: Tensor, batch):
        """efficient_gat_3d.py:173-220 -> (hstack(unit quaternion wxyz, mlp_t's outputs) [P, 4 + t_channels], attentions): [P, 7], or
        with ``input_channels=13, t_channels=9`` (use_6dof) [P, 13] = quaternion | translation | a1 | a2."""
        if self._wants_grad():       # training: da_train_forward now, da_train_backward under autograd (no attention weights)
            return self._run_train(xy_pos, time, edge_index, pcd_feats, batch)
        return self._run(xy_pos, time, edge_index, pcd_feats, batch, self.return_attentions)

    def pcd_features(self, pcd):
        """efficient_gat_3d.py:230-236: pcd [P, N, 3] -> pcd_feats [P, feat_dim]."""
        if self.pcd_backbone is None and self.pcd_encoder is not None:        # PointNet++: inference only
            if self.pcd_encoder.training:
                raise NotImplementedError(self.pcd_encoder.TRAIN_MESSAGE)      # its train() mode is the follow-up
            with torch.no_grad():
                return self.pcd_encoder(pcd)
        if self.pcd_backbone is None:
            raise NotImplementedError(
                "the point-cloud encoders built are backbone='vn_dgcnn' / 'vn_dgcnn_inv' / 'pointnet' / 'pointnet_plus'; "
                "'pointnet_inv' and 'vnn' have none: pass pcd_feats")
        if self.freeze_backbone:
            # no gradient, but the backbone keeps its mode: in train() its BatchNorms still use and update batch statistics
            with torch.no_grad():
                return self.pcd_backbone(pcd)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.pcd_backbone.parameters()):
            # a trainable backbone is reached through the 3D model's own training step: GNN_Diffusion.p_losses calls
            # pcd_features_train, whose output carries the encoder's autograd graph into the denoiser backward's d_feats
            raise NotImplementedError(
                "pcd_features is the inference-side encoder call: a trainable backbone trains through GNN_Diffusion.p_losses "
                "(pcd_features_train); set freeze_backbone=True or run pcd_features under torch.no_grad() for features alone")
        return self.pcd_backbone(pcd)

    def pcd_features_train(self, pcd):
        """The encoder call of ``p_losses`` (efficient_gat_3d.py:230-236 inside the training step): with a trainable backbone the
        differentiable ``VN_DGCNN`` (HIP forward and backward in train() mode), so that ``d_feats`` of the denoiser backward
        flows into the encoder through autograd; with ``freeze_backbone`` the no-grad ``pcd_features``.  The inference-only
        PointNet++ goes through ``pcd_features`` too: in train() that raises (its train() mode is the follow-up)."""
        if self.pcd_backbone is None or self.freeze_backbone:
            return self.pcd_features(pcd)
        return self.pcd_backbone(pcd)
