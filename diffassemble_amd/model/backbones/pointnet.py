"""Module surface of the reference's plain PointNet (/root/reference/puzzle_diff/model/backbones/pointnet.py:8-43):
``PointNet(feat_dim, global_feat=True)`` with the same state-dict keys (``conv{1..5}.weight [out, in, 1]``,
``bn{1..5}.{weight,bias,running_mean,running_var,num_batches_tracked}``), so checkpoints load unchanged.

The module only HOLDS parameters; the forward runs in libdiffassemble_hip.so (da_pointnet.hip; no torch fallback):
* eval(): ``diffassemble_amd.pointnet_encoder.PointNetEngine`` -- BatchNorm on the running statistics, folded into the layers;
* train(): ``diffassemble_amd.pointnet_encoder.PointNetTrainEngine`` -- BatchNorm on the batch statistics of the call's P * N
  points, every BatchNorm buffer updated in place with the module's momentum / eps, and, under grad, one autograd node
  (``PointNetTrainFunction``) whose backward gives the gradients of the five conv weights and the five (gamma, beta) pairs.
  The points are data and get no gradient; a single point raises the ValueError torch's BatchNorm raises.

``PointNetPlus`` (pointnet.py:200-256 of the same file) is the module surface of PointNet++: eval mode only, see its docstring."""
import torch
import torch.nn as nn

from ...pointnet_encoder import PointNetEngine, PointNetTrainEngine
from ...pointnet_plus_encoder import PointNetPlusEngine


class PointNet(nn.Module):
    def __init__(self, feat_dim, global_feat=True):
        super().__init__()
        if not global_feat:
            raise NotImplementedError("PointNet(global_feat=False): the per-point output is never built by the reference's models")
        self.conv1 = nn.Conv1d(3, 64, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv3 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv4 = nn.Conv1d(64, 128, kernel_size=1, bias=False)
        self.conv5 = nn.Conv1d(128, feat_dim, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(64)
        self.bn3 = nn.BatchNorm1d(64)
        self.bn4 = nn.BatchNorm1d(128)
        self.bn5 = nn.BatchNorm1d(feat_dim)
        self.global_feat = global_feat
        self._engine, self._engine_key = None, None
        self._train_engine = None

    def engine_key(self):
        """What the packed eval weights depend on: every parameter / buffer's storage and version."""
        return tuple((t.data_ptr(), t._version) for t in self.state_dict().values())

    def engine(self):
        """Packed, folded eval weights, rebuilt when a parameter / buffer was replaced or modified in place."""
        key = self.engine_key()
        if self._engine is None or self._engine_key != key:
            self._engine = PointNetEngine(self.state_dict(), eps=[getattr(self, f"bn{l}").eps for l in range(1, 6)],
                                          device=self.conv1.weight.device)
            self._engine_key = key
        return self._engine

    def train_engine(self):
        """The train-mode engine (packs the live parameters on every call)."""
        if self._train_engine is None:
            self._train_engine = PointNetTrainEngine(self)
        return self._train_engine

    def forward(self, x):
        """pointnet.py:31-43.  x [P, N, 3] -> [P, feat_dim]."""
        if self.training:
            return self.train_engine().forward(x)
        return self.engine().forward(x)


class _SetAbstraction(nn.Module):
    """Parameter holder of one set-abstraction level (pointnet.py:406-419): ``mlp_convs.{i}`` Conv2d(1x1, with bias) and
    ``mlp_bns.{i}`` BatchNorm2d."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel


class PointNetPlus(nn.Module):
    """Module surface of the reference's ``PointNetPlus`` (pointnet.py:200-256) with the same state-dict keys
    (``sa{1,2,3}.mlp_convs.{0,1,2}.{weight [out, in, 1, 1], bias}``, ``sa{1,2,3}.mlp_bns.{0,1,2}.*``, ``fc1.*``, ``bn1.*``,
    ``fc2.*``, ``bn2.*``), so checkpoints load with ``strict=True``.  It only HOLDS parameters: the eval forward runs in
    libdiffassemble_hip.so (da_pointnet_plus.hip through ``pointnet_plus_encoder.PointNetPlusEngine``; no torch fallback).

    train() mode -- batch-statistics BatchNorm over the grouped rows, active dropout, the backward through gather and group
    max -- is the follow-up and raises ``NotImplementedError``; inference needs ``.eval()``."""

    TRAIN_MESSAGE = ("PointNetPlus in train() mode (batch-statistics BatchNorm over the grouped rows, active dropout, the backward through "
                     "gather and group max) is the follow-up to the eval encoder and is not built: inference needs .eval(); to train the "
                     "denoiser on this backbone's features, freeze it in eval mode and pass pcd_feats")

    def __init__(self, normal_channel=False):
        super().__init__()
        if normal_channel:
            raise NotImplementedError("PointNetPlus(normal_channel=True): the reference's models build it without normals (6 input channels)")
        self.normal_channel = False
        self.sa1 = _SetAbstraction(6, [64, 64, 128])
        self.sa2 = _SetAbstraction(128 + 3, [128, 128, 256])
        self.sa3 = _SetAbstraction(256 + 3, [256, 512, 1024])
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self._engine, self._engine_key = None, None

    def engine_key(self):
        """What the packed eval weights depend on: every parameter / buffer's storage and version."""
        return tuple((t.data_ptr(), t._version) for t in self.state_dict().values())

    def _bn_eps(self):
        return [bn.eps for sa in (self.sa1, self.sa2, self.sa3) for bn in sa.mlp_bns] + [self.bn1.eps, self.bn2.eps]

    def engine(self):
        """Packed, folded eval weights, rebuilt when a parameter / buffer was replaced or modified in place."""
        key = self.engine_key()
        if self._engine is None or self._engine_key != key:
            self._engine = PointNetPlusEngine(self.state_dict(), eps=self._bn_eps(), device=self.fc1.weight.device)
            self._engine_key = key
        return self._engine

    @staticmethod
    def draw_fps_start(n_parts, n_points):
        """The first indices of the two levels' farthest point sampling as the reference draws them (pointnet.py:322): HOST generator,
        sa1 (among the n_points points) first, then sa2 (among sa1's 512 centres)."""
        return (torch.randint(0, n_points, (n_parts,), dtype=torch.long), torch.randint(0, 512, (n_parts,), dtype=torch.long))

    def forward(self, x, fps_start=None):
        """pointnet.py:225-255 in eval mode.  x [P, N, 3] -> [P, 256]; ``fps_start``: optional (start1 [P], start2 [P])."""
        if self.training:
            raise NotImplementedError(self.TRAIN_MESSAGE)
        if fps_start is None:
            fps_start = self.draw_fps_start(int(x.shape[0]), int(x.shape[1]))
        return self.engine().forward(x, fps_start)
