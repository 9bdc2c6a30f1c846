"""Module surface of the reference's default piece encoder, timm's ``efficientnet_b0`` built with ``features_only=True``
(puzzle_diff/model/backbones/efficient_gat.py:37-42): the same state-dict keys in timm's registration order (``conv_stem.weight``,
``bn1.*``, ``blocks.S.B.{conv_pw, bn1, conv_dw, bn2, se.conv_reduce, se.conv_expand, conv_pwl, bn3}.*``; ``blocks.0.0`` is the
depthwise-separable ``conv_dw, bn1, se, conv_pw, bn2``), so a reference checkpoint's ``visual_backbone.*`` loads with ``strict=True``.

The modules only HOLD parameters.  The arithmetic of the eval-mode feature forward -- stem through ``blocks.4``, feature maps 2 and 3,
what ``Eff_GAT.visual_features`` keeps -- runs in libdiffassemble_hip.so through ``diffassemble_amd.efficientnet_encoder.EfficientNetEngine``
(da_efficientnet.hip; BatchNorm folded, fp32).  ``blocks.5`` / ``blocks.6`` are held because a checkpoint carries them and never read
(like ``linear1`` / ``linear2`` of ``Eff_GAT``).  No torch fallback; train() mode (batch-statistics BatchNorm, the backward) is not built.

The table is written from timm's published architecture; timm itself is not a dependency and was not available to check it against.
"""
import math

import torch
import torch.nn as nn

from ...efficientnet_encoder import EfficientNetEngine

# timm's efficientnet_b0 stages: (blocks, kernel, stride, expansion, out channels); squeeze width = block input / 4
_STAGES = ((1, 3, 1, 1, 16), (2, 3, 2, 6, 24), (2, 5, 2, 6, 40), (3, 3, 2, 6, 80), (3, 5, 1, 6, 112), (4, 5, 2, 6, 192), (1, 3, 1, 6, 320))


def _conv(cin, cout, k, stride=1, groups=1, bias=False):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, groups=groups, bias=bias)


class _SqueezeExcite(nn.Module):
    def __init__(self, channels, reduced):
        super().__init__()
        self.conv_reduce = _conv(channels, reduced, 1, bias=True)
        self.conv_expand = _conv(reduced, channels, 1, bias=True)


class _DepthwiseSeparable(nn.Module):
    """timm's DepthwiseSeparableConv: conv_dw, bn1, act, se, conv_pw, bn2 (no activation after bn2)."""

    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.conv_dw = _conv(cin, cin, k, stride, groups=cin)
        self.bn1 = nn.BatchNorm2d(cin)
        self.se = _SqueezeExcite(cin, cin // 4)
        self.conv_pw = _conv(cin, cout, 1)
        self.bn2 = nn.BatchNorm2d(cout)


class _InvertedResidual(nn.Module):
    """timm's InvertedResidual: conv_pw, bn1, act, conv_dw, bn2, act, se, conv_pwl, bn3."""

    def __init__(self, cin, cout, k, stride, expansion):
        super().__init__()
        mid = cin * expansion
        self.conv_pw = _conv(cin, mid, 1)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv_dw = _conv(mid, mid, k, stride, groups=mid)
        self.bn2 = nn.BatchNorm2d(mid)
        self.se = _SqueezeExcite(mid, cin // 4)
        self.conv_pwl = _conv(mid, cout, 1)
        self.bn3 = nn.BatchNorm2d(cout)


class EfficientNetB0Features(nn.Module):
    TRAIN_MESSAGE = ("EfficientNetB0Features in train() mode: train-mode BatchNorm and the backward are not built; set "
                     "frozen_eval_stats = True for a frozen encoder, or call .eval() (a trainable EfficientNet is the follow-up)")

    def __init__(self):
        super().__init__()
        self.conv_stem = _conv(3, 32, 3, stride=2)
        self.bn1 = nn.BatchNorm2d(32)
        cin, stages = 32, []
        for n, k, stride, expansion, cout in _STAGES:
            blocks = []
            for b in range(n):
                s = stride if b == 0 else 1
                blocks.append(_DepthwiseSeparable(cin, cout, k, s) if expansion == 1 else _InvertedResidual(cin, cout, k, s, expansion))
                cin = cout
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        # timm's initialisation of this family: conv weights N(0, 2 / fan_out), fan_out = k k out / groups; BatchNorm 1 / 0; biases 0
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
                nn.init.normal_(m.weight, 0.0, math.sqrt(2.0 / fan_out))
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        self._engine = None
        self._engine_key = None
        # Set to True to run a FROZEN encoder on its RUNNING statistics while the LightningModule is in train mode.  Without it
        # train() mode would mean batch statistics (the reference's behaviour under model.train()), which is not built here.
        self.frozen_eval_stats = False

    def engine(self):
        """Packed weights, rebuilt when a parameter / buffer was replaced or modified in place."""
        sd = self.state_dict()
        key = tuple((t.data_ptr(), t._version) for t in sd.values())
        if self._engine is None or self._engine_key != key:
            self._engine = EfficientNetEngine(sd, eps=self.bn1.eps, device=self.conv_stem.weight.device)
            self._engine_key = key
        return self._engine

    def patch_features(self, patch_rgb, quarter_turns=0):
        """[N, 3, 32, 32] in [0, 1], NOT normalised (the stem kernel normalises) -> [N, 1088] = cat(map 2, map 3) flattened, the two
        maps Eff_GAT.visual_features keeps.  ``quarter_turns`` r: the crops turned clockwise by r quarter turns."""
        if self.training and not self.frozen_eval_stats:
            raise NotImplementedError(self.TRAIN_MESSAGE)
        return self.engine().forward(patch_rgb, quarter_turns=quarter_turns)

    def forward(self, x):
        raise NotImplementedError(
            "EfficientNetB0Features.forward on pre-normalised input is not exposed: Eff_GAT.visual_features calls patch_features "
            "(normalisation is fused into the stem kernel)")
