"""Host side of the PointNet++ fragment encoder (``backbone="pointnet_plus"``; the eval forward of the reference's
puzzle_diff/model/backbones/pointnet.py:200-256): packs a ``PointNetPlus`` state dict into the fp32 tensors
``da_pointnet_plus_forward`` reads (include/diffassemble_hip.h) -- eval BatchNorm folded into every layer in fp64, the first
layer of each level with its input columns in the kernels' order [features | xyz | zero padding].  No torch arithmetic on the data
path, no CPU fallback."""
import ctypes as C
import math

import torch

from . import _lib

LEVELS = 3
OUT_DIM = 256
MAX_POINTS = 2048
S1, S2 = 512, 128                                    # centres of sa1 / sa2
SA_WIDTHS = ((6, 64, 64, 128), (131, 128, 128, 256), (259, 256, 512, 1024))
STAGES = {"fps1": 1, "ball1": 2, "sa1": 4, "fps2": 8, "ball2": 16, "sa2": 32, "sa3": 64, "head": 128}
# the workspace's stage tensors per fragment, in the order of da_pointnet_plus_workspace_offsets
WORKSPACE_TENSORS = (("fps1", torch.int32, (512,)), ("grp1", torch.int32, (512, 32)), ("fps2", torch.int32, (128,)),
                     ("grp2", torch.int32, (128, 64)), ("l1", torch.float32, (512, 128)), ("l2", torch.float32, (128, 256)),
                     ("part", torch.float32, (4, 1024)))


def _fold(w, b, sd, bn, eps):
    """eval BatchNorm folded into the layer before it (fp64): W' = diag(s) W, b' = (b - mean) s + beta, s = gamma / sqrt(var + eps)."""
    s = sd[f"{bn}.weight"].double() / torch.sqrt(sd[f"{bn}.running_var"].double() + eps)
    return w.double() * s[:, None], (b.double() - sd[f"{bn}.running_mean"].double()) * s + sd[f"{bn}.bias"].double()


def _columns(w, level):
    """The first layer's input columns [xyz (3) | features] -> the kernels' [features | xyz | 0 ...] with K padded to a multiple of 8
    (sa1: the six columns as they are, + 0 0)."""
    cin = w.shape[1]
    kp = (cin + 7) // 8 * 8
    out = torch.zeros(w.shape[0], kp, dtype=w.dtype, device=w.device)
    if level == 0:
        out[:, :cin] = w
    else:
        out[:, :cin - 3] = w[:, 3:]
        out[:, cin - 3:cin] = w[:, :3]
    return out


class PointNetPlusEngine:
    """Packed, folded eval PointNet++.  ``sd``: state dict with the reference's ``PointNetPlus()`` keys (``pcd_backbone.*`` of an
    ``Eff_GAT_3d`` checkpoint with the prefix stripped); ``eps``: BatchNorm eps of the eleven layers (sa1.0 .. sa3.2, bn1, bn2)."""

    def __init__(self, sd, *, eps=(1e-5,) * _lib.PNP_LAYERS, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.DaError("PointNetPlusEngine needs a ROCm device (no CPU path in diffassemble_amd)")
        self.lib = _lib.lib()
        sd = {k: v.detach().to(self.device) for k, v in sd.items() if v.is_floating_point()}
        self._keep = []
        w = _lib.DaPointnetPlusWeights()
        l = 0
        for s in range(LEVELS):
            for i in range(3):
                cw = sd[f"sa{s + 1}.mlp_convs.{i}.weight"]
                assert tuple(cw.shape) == (SA_WIDTHS[s][i + 1], SA_WIDTHS[s][i], 1, 1), (s, i, tuple(cw.shape))
                wf, bf = _fold(cw.reshape(cw.shape[0], -1), sd[f"sa{s + 1}.mlp_convs.{i}.bias"], sd, f"sa{s + 1}.mlp_bns.{i}", float(eps[l]))
                if i == 0:
                    wf = _columns(wf, s)
                self._put(w, l, wf, bf)
                l += 1
        for j, (cin, cout) in enumerate(((1024, 512), (512, 256))):
            fw = sd[f"fc{j + 1}.weight"]
            assert tuple(fw.shape) == (cout, cin), (j, tuple(fw.shape))
            self._put(w, l, *_fold(fw, sd[f"fc{j + 1}.bias"], sd, f"bn{j + 1}", float(eps[l])))
            l += 1
        self.w = w
        self._ws = None
        self.chunk = int(self.lib.da_pointnet_plus_workspace_offsets(0, None))      # fragments per pass over the workspace

    def _put(self, w, l, wf, bf):
        wf, bf = wf.float().contiguous(), bf.float().contiguous()
        self._keep += [wf, bf]
        w.w[l], w.b[l] = wf.data_ptr(), bf.data_ptr()

    def _starts(self, fps_start, P):
        out = []
        for t in fps_start:
            t = torch.as_tensor(t).to(self.device, torch.int32).contiguous()
            assert t.shape == (P,), (tuple(t.shape), P)
            out.append(t)
        assert len(out) == 2
        return out

    def _call(self, points, fps_start, out, stages):
        if points.device.type != "cuda":
            raise _lib.DaError("PointNetPlusEngine.forward: the point clouds must live on the ROCm device")
        assert points.dim() == 3 and points.shape[2] == 3, tuple(points.shape)
        x = points.detach().to(torch.float32).contiguous()
        P, N = int(x.shape[0]), int(x.shape[1])
        if out is None:
            out = torch.empty(P, OUT_DIM, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.shape == (P, OUT_DIM) and (P == 0 or out.stride(1) == 1)
        if P == 0:
            _lib.check(self.lib.da_pointnet_plus_forward(self.w, 0, N, None, None, None, None, OUT_DIM, None, 0, _lib.stream_ptr(self.device)))
            return out
        s1, s2 = self._starts(fps_start, P)
        need = self.lib.da_pointnet_plus_workspace_bytes(P, N)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        args = (self.w, P, N, _lib.ptr(x), _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(out), out.stride(0), _lib.ptr(self._ws), self._ws.numel())
        if stages is None:
            _lib.check(self.lib.da_pointnet_plus_forward(*args, _lib.stream_ptr(self.device)))
        else:
            _lib.check(self.lib.da_pointnet_plus_stages(*args, int(stages), _lib.stream_ptr(self.device)))
        return out

    def forward(self, points, fps_start, out=None):
        """points [P, N, 3] fp32 (device), P >= 0, 1 <= N <= 2048; fps_start = (start1 [P] in [0, N), start2 [P] in [0, 512)): the
        first index of each level's farthest point sampling -> [P, 256] fp32 (``out``: any row stride, unit column stride)."""
        return self._call(points, fps_start, out, None)

    def run_stages(self, points, fps_start, out, stages):
        """Only the stages of the bit set (``STAGES``), on the workspace the last ``forward`` of the same shape left: for timing,
        and for tests of one stage on inputs written through ``workspace_views``."""
        return self._call(points, fps_start, out, stages)

    def workspace_views(self, P):
        """Typed views of the stage tensors in the workspace (``da_pointnet_plus_workspace_offsets``), valid after a ``forward`` /
        ``run_stages`` of P <= ``chunk`` fragments (a larger call reuses the workspace chunk by chunk): what a stage wrote, or -- written
        into before ``run_stages`` with one stage's bit -- what it reads.  The kernels do not bounds-check the indices: fps1 / grp1 in
        [0, N), fps2 / grp2 in [0, 512)."""
        P = int(P)
        if not 1 <= P <= self.chunk:
            raise _lib.DaError(f"PointNetPlusEngine.workspace_views: P = {P} (need 1 .. {self.chunk}, one pass over the workspace)")
        off = (C.c_size_t * len(WORKSPACE_TENSORS))()
        self.lib.da_pointnet_plus_workspace_offsets(P, off)
        if self._ws is None or self._ws.numel() < self.lib.da_pointnet_plus_workspace_bytes(P, 1):
            raise _lib.DaError(f"PointNetPlusEngine.workspace_views: no workspace of {P} fragments yet (run forward first)")
        views = {}
        for (name, dtype, shape), o in zip(WORKSPACE_TENSORS, off):
            n = P * math.prod(shape)
            views[name] = self._ws[o:o + 4 * n].view(dtype).view(P, *shape)
        return views


def fps(points, npoint, start):
    """da_pnp_fps: points [P, N, 3] fp32 (device), start [P] -> int32 [P, npoint]."""
    x = points.detach().to(torch.float32).contiguous()
    P, N = int(x.shape[0]), int(x.shape[1])
    s = torch.as_tensor(start).to(x.device, torch.int32).contiguous()
    idx = torch.empty(P, npoint, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().da_pnp_fps(P, N, npoint, _lib.ptr(x), _lib.ptr(s), _lib.ptr(idx), _lib.stream_ptr(x.device)))
    return idx


def ball_query(points, centre, radius, nsample):
    """da_pnp_ball_query: points [P, N, 3] fp32 (device), centre int [P, S] (indices into the N points) -> int32 [P, S, nsample]."""
    x = points.detach().to(torch.float32).contiguous()
    P, N = int(x.shape[0]), int(x.shape[1])
    c = centre.to(x.device, torch.int32).contiguous()
    grp = torch.empty(P, c.shape[1], nsample, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().da_pnp_ball_query(P, N, int(c.shape[1]), nsample, float(radius), _lib.ptr(x), _lib.ptr(c), _lib.ptr(grp),
                                            _lib.stream_ptr(x.device)))
    return grp
