"""Module surface of the reference's plain PointNet (/root/reference/puzzle_diff/model/backbones/pointnet.py:8-43):
``PointNet(feat_dim, global_feat=True)`` with the same state-dict keys (``conv{1..5}.weight [out, in, 1]``,
``bn{1..5}.{weight,bias,running_mean,running_var,num_batches_tracked}``), so checkpoints load unchanged.

The module only HOLDS parameters; the forward runs in libdiffassemble_hip.so (da_pointnet.hip; no torch fallback):
* eval(): ``diffassemble_amd.pointnet_encoder.PointNetEngine`` -- BatchNorm on the running statistics, folded into the layers;
* train(): ``diffassemble_amd.pointnet_encoder.PointNetTrainEngine`` -- BatchNorm on the batch statistics of the call's P * N
  points, every BatchNorm buffer updated in place with the module's momentum / eps, and, under grad, one autograd node
  (``PointNetTrainFunction``) whose backward gives the gradients of the five conv weights and the five (gamma, beta) pairs.
  The points are data and get no gradient; a single point raises the ValueError torch's BatchNorm raises."""
import torch.nn as nn

from ...pointnet_encoder import PointNetEngine, PointNetTrainEngine


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
