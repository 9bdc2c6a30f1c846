"""Counterpart of puzzle_diff/model/backbones/efficient_gat_discrete.py (``Eff_GAT_Discrete``): the denoiser of the discrete
position diffusion.  Same constructor arguments, attribute and state-dict names; ``forward_with_feats`` runs as ONE call into
the HIP library (embedding lookup -> mlp -> 4x graph attention -> residual -> K-wide logits head).  Under grad (``train()`` mode
with trainable parameters) the forward and its backward run through ``DenoiserTrainFn`` over da_train_forward_idx /
da_train_backward_idx: the indices get no gradient, ``patch_feats`` get theirs when they require it."""
import torch
import torch.nn as nn
from torch import Tensor

from ._denoiser_base import DenoiserBase
from .efficient_gat import hip_patch_features, hip_piece_encoder
from .efficientnet import EfficientNetB0Features
from .Transformer_GNN import Transformer_GNN


class Eff_GAT_Discrete(DenoiserBase):
    variant = "discrete"

    def __init__(self, steps, input_channels, output_channels, use_hip_encoder=False) -> None:
        super().__init__()
        # piece encoder (efficient_gat_discrete.py:22-24): not on the per-timestep path; built only when timm is importable,
        # otherwise callers pass patch_feats (as in Eff_GAT) -- unless use_hip_encoder asks for the in-tree EfficientNet-B0
        self.use_hip_encoder = use_hip_encoder
        if use_hip_encoder:
            self.visual_backbone = hip_piece_encoder("efficientnet_b0")
        else:
            try:
                import timm
                self.visual_backbone = timm.create_model("efficientnet_b0", pretrained=True, features_only=True)
            except Exception:  # noqa: BLE001  (timm absent / no weights / no network)
                self.visual_backbone = None
        self.input_channels, self.output_channels = input_channels, output_channels
        self.combined_features_dim = 1088 + 32 + 32
        D = self.combined_features_dim
        self.gnn_backbone = Transformer_GNN(D, hidden_dim=32 * 8, heads=8, output_size=D)
        self.time_emb = nn.Embedding(steps, 32)
        self.pos_mlp = nn.Embedding(input_channels, 32)
        self.mlp = nn.Sequential(nn.Linear(D, 128), nn.GELU(), nn.Linear(128, D))
        self.final_mlp = nn.Sequential(nn.Linear(D, 32), nn.GELU(), nn.Linear(32, output_channels))
        self.register_buffer("mean", torch.tensor([0.4850, 0.4560, 0.4060])[None, :, None, None])
        self.register_buffer("std", torch.tensor([0.2290, 0.2240, 0.2250])[None, :, None, None])
        self.return_attentions = False

    def forward(self, xy_pos, time, patch_rgb, edge_index, batch):
        patch_feats = self.visual_features(patch_rgb)
        return self.forward_with_feats(xy_pos, time, patch_rgb, edge_index, patch_feats=patch_feats, batch=batch)

    def forward_with_feats(self, xy_pos: Tensor, time: Tensor, patch_rgb: Tensor, edge_index: Tensor, patch_feats: Tensor, batch):
        """efficient_gat_discrete.py:72-97 -> (logits [N, K] fp32, attentions).  ``xy_pos``: position indices [N]."""
        if self._wants_grad():
            return self._run_train(xy_pos, time, edge_index, patch_feats, batch)
        with torch.no_grad():
            return self._run_idx(xy_pos, time, edge_index, patch_feats, batch)

    def _run_idx(self, xy_pos, time, edge_index, patch_feats, batch):
        eng = self.engine(xy_pos.device)
        plan = self._plan_for(eng, edge_index, batch)
        self._stage_features(eng, plan, patch_feats)
        if self.return_attentions:
            out, alpha = eng.forward_idx(plan, xy_pos, time, None, return_alpha=True)
            return out, [(plan.edge_index, alpha[l]) for l in range(alpha.shape[0])]
        return eng.forward_idx(plan, xy_pos, time, None), None

    def visual_features(self, patch_rgb):
        """efficient_gat_discrete.py:99-114: normalise, piece encoder, concat feature maps 2 and 3 -> [N, 1088]."""
        if self.visual_backbone is None:
            raise NotImplementedError("no piece encoder available (timm is outside the hot path): pass precomputed patch_feats [N, 1088]")
        if isinstance(self.visual_backbone, EfficientNetB0Features):      # use_hip_encoder: da_effnet_forward
            return hip_patch_features(self.visual_backbone, patch_rgb)
        patch_rgb = (patch_rgb - self.mean) / self.std
        feats = self.visual_backbone.forward(patch_rgb)
        n = patch_rgb.shape[0]
        return torch.cat([feats[2].reshape(n, -1), feats[3].reshape(n, -1)], -1)
