"""Counterpart of puzzle_diff/model/backbones/efficient_gat_discrete_rotation.py (``Eff_GAT_Discrete_ROT``): the denoiser of the
discrete position + rotation diffusion -- ``Eff_GAT_Discrete`` with a second, 4-wide head ``final_mlp_rot``.  Same constructor
arguments, attribute and state-dict names; ``forward_with_feats`` runs as ONE call into the HIP library and returns
``(logits [N, K], rot_logits [N, 4])``.  Under grad (``train()`` mode with trainable parameters) the forward and its backward run
through ``DenoiserTrainFn2`` over da_train_forward_rot / da_train_backward_rot, on ROCm tensors only: the first layer of both heads is
one 64-wide product each way, and a head whose logits take no part in the loss costs no second-layer products.

Differences from the reference, on purpose:
* the reference's ``forward_with_feats`` raises as shipped (:106-110 adds the ``(x, attentions)`` pair ``Transformer_GNN`` returns to
  a tensor); this module computes what it computes once the pair is unpacked, as ``Eff_GAT_Discrete`` does;
* ``patch_feats`` may be the FOUR feature images of the Batch, [4, N, 1088] (image r: the crops rotated by -r quarter turns), with a
  ``rot_acc`` keyword [N] in {0..3} that picks each piece's image -- what the reference obtains by rotating and re-encoding the crops
  inside its sampling loop.  [N, 1088] is image 0 for every piece;
* the three constructor arguments are optional so that the bare import placeholder of earlier versions keeps raising
  ``NotImplementedError`` when called without them.
"""
import torch
import torch.nn as nn
from torch import Tensor

from ...train import DenoiserTrainFn2
from ._denoiser_base import _Held
from .efficient_gat import hip_patch_features
from .efficient_gat_discrete import Eff_GAT_Discrete
from .efficientnet import EfficientNetB0Features

_NOT_BUILT = "discrete-rotation training is not built yet"
_OFF_DEVICE = _NOT_BUILT + " off the device: it runs on ROCm tensors only (diffassemble_amd has no CPU path)"


class Eff_GAT_Discrete_ROT(Eff_GAT_Discrete):
    variant = "discrete_rot"

    def __init__(self, steps=None, input_channels=None, output_channels=None, rotation_channels=4, use_hip_encoder=False) -> None:
        if steps is None or input_channels is None or output_channels is None:
            raise NotImplementedError("Eff_GAT_Discrete_ROT needs steps, input_channels and output_channels")
        if rotation_channels != 4:
            raise NotImplementedError("Eff_GAT_Discrete_ROT: rotation_channels must be 4 (quarter turns)")
        super().__init__(steps, input_channels, output_channels, use_hip_encoder=use_hip_encoder)
        self.rotation_channels = rotation_channels
        self.final_mlp_rot = nn.Sequential(nn.Linear(self.combined_features_dim, 32), nn.GELU(), nn.Linear(32, rotation_channels))

    def forward(self, xy_pos, rot, time, patch_rgb, edge_index, batch):
        patch_feats = self.visual_features(patch_rgb)
        return self.forward_with_feats(xy_pos, rot, time, patch_rgb, edge_index, patch_feats=patch_feats, batch=batch)

    def forward_with_feats(self, xy_pos: Tensor, rot: Tensor, time: Tensor, patch_rgb: Tensor, edge_index: Tensor, patch_feats: Tensor,
                           batch, rot_acc=None):
        """efficient_gat_discrete_rotation.py:87-115 -> (logits [N, K], rot_logits [N, 4]) fp32.  ``rot`` is not read (the reference's
        network does not read it either); ``rot_acc`` needs ``patch_feats`` [4, N, 1088].  Under grad: the training route, one feature
        image ``patch_feats`` [N, 1088] and no ``rot_acc`` (the reference's p_losses encodes the unrotated crops once); both outputs
        require grad."""
        if self._wants_grad():
            if not all(torch.is_tensor(v) and v.is_cuda for v in (xy_pos, time, edge_index, patch_feats)):
                raise NotImplementedError(_OFF_DEVICE)
            if rot_acc is not None or patch_feats.dim() != 2:
                raise ValueError("training reads one feature image: patch_feats [N, 1088] and rot_acc=None")
            return self._run_train2(xy_pos, time, edge_index, patch_feats, batch)
        if rot_acc is not None and patch_feats.dim() != 3:
            raise ValueError("rot_acc needs the four feature images: patch_feats [4, N, 1088]")
        with torch.no_grad():
            eng = self.engine(xy_pos.device)
            plan = self._plan_for(eng, edge_index, batch)
            self._stage_features(eng, plan, patch_feats)
            return eng.forward_rot(plan, xy_pos, time, None, rot_acc=rot_acc)

    def _run_train2(self, xy_pos, time, edge_index, feats, batch):
        """``DenoiserBase._run_train`` with two outputs."""
        te = self.train_engine(xy_pos.device)
        key = getattr(self, "_tplan_key", None)
        if key is None or not key.matches((edge_index, batch), (id(te),)):
            from ...graph_plan import build_plan
            self._tplan = build_plan(edge_index.to(te.device), batch.to(te.device), te.virt_nodes).with_source_csr()
            self._tplan_key = _Held((edge_index, batch), (id(te),))
        return DenoiserTrainFn2.apply(te, self._tplan, xy_pos, time, feats, te.anchor)

    def _stage_features(self, eng, plan, feats):
        key = getattr(self, "_feat_key", None)
        if key is None or not key.matches((feats,), (id(plan),)):
            eng.set_features_rot(plan, feats)
            self._feat_key = _Held((feats,), (id(plan),))

    def visual_features4(self, patch_rgb):
        """[4, N, 1088]: image r = ``visual_features(rotate_images(patch_rgb, -r))`` (spatial_diffusion_discrete_rot.py:353, :373,
        :542-546).  Needs the piece encoder (timm) and kornia; the table itself is the input contract of the HIP path.  On the in-tree
        encoder (``use_hip_encoder``) no kornia: image r is the encoder reading the crops through r CLOCKWISE quarter turns --
        ``Rotate(-90 r, mode="nearest")`` on a 32 x 32 crop is an exact quarter turn, and kornia documents positive angles as
        counter-clockwise."""
        if self.visual_backbone is None:
            raise NotImplementedError("no piece encoder available (timm is outside the hot path): pass precomputed patch_feats [4, N, 1088]")
        if isinstance(self.visual_backbone, EfficientNetB0Features):
            return torch.stack([hip_patch_features(self.visual_backbone, patch_rgb, quarter_turns=r) for r in range(4)])
        try:
            from kornia.geometry.transform import Rotate
        except Exception as e:  # noqa: BLE001
            raise NotImplementedError("no piece encoder available (kornia is outside the hot path): pass precomputed patch_feats "
                                      "[4, N, 1088]") from e
        n = patch_rgb.shape[0]
        imgs = [self.visual_features(patch_rgb)]
        for r in (1, 2, 3):
            angles = torch.full((n,), -90.0 * r, device=patch_rgb.device)
            imgs.append(self.visual_features(Rotate(angles, mode="nearest")(patch_rgb)))
        return torch.stack(imgs)
