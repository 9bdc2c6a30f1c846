"""Host side of the PointNet fragment encoder (``backbone="pointnet"``; the reference's
puzzle_diff/model/backbones/pointnet.py:8-43): packs a ``PointNet`` state dict into the fp32 tensors ``da_pointnet_forward``
reads (include/diffassemble_hip.h) -- eval BatchNorm folded into every layer in fp64 -- and drives the train-mode forward /
backward (``da_pointnet_train_forward`` / ``_backward``: batch-statistics BatchNorm, gradients of the five conv weights and
the five (gamma, beta) pairs).  No torch arithmetic on the data path, no CPU fallback."""
import torch

from . import _lib

LAYERS = 5
WIDTHS_IN = (3, 64, 64, 64, 128)


def _fold(sd, l):
    """eval BatchNorm l folded into conv l (fp64): W' = diag(gamma / sqrt(var + eps)) W, b' = beta - mean gamma / sqrt(var + eps).
    gamma may be negative: the fold is exact because the max over the points comes after the affine."""
    conv, bn = f"conv{l + 1}", f"bn{l + 1}"
    w = sd[f"{conv}.weight"].double().reshape(sd[f"{conv}.weight"].shape[0], -1)
    scale = sd[f"{bn}.weight"].double() / torch.sqrt(sd[f"{bn}.running_var"].double() + sd[f"{bn}.eps"])
    return (w * scale[:, None]).float().contiguous(), (sd[f"{bn}.bias"].double() - sd[f"{bn}.running_mean"].double() * scale).float().contiguous()


class PointNetEngine:
    """Packed, folded eval PointNet.  ``sd``: state dict with the reference's ``PointNet(feat_dim)`` keys (``pcd_backbone.*`` of an
    ``Eff_GAT_3d`` checkpoint with the prefix stripped); ``eps``: the five BatchNorm eps values."""

    def __init__(self, sd, *, eps=(1e-5,) * LAYERS, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.DaError("PointNetEngine needs a ROCm device (no CPU path in diffassemble_amd)")
        self.lib = _lib.lib()
        sd = {k: v.detach().to(self.device) for k, v in sd.items() if v.is_floating_point()}
        for l in range(LAYERS):
            sd[f"bn{l + 1}.eps"] = float(eps[l])
        self.feat_dim = int(sd["conv5.weight"].shape[0])
        self._keep = []
        w = _lib.DaPointnetWeights()
        w.feat_dim = self.feat_dim
        for l in range(LAYERS):
            cw = sd[f"conv{l + 1}.weight"]
            assert cw.shape[1] == WIDTHS_IN[l] and cw.shape[0] == (WIDTHS_IN[l + 1] if l < 4 else self.feat_dim), (l, tuple(cw.shape))
            wf, bf = _fold(sd, l)
            self._keep += [wf, bf]
            w.w[l], w.b[l] = wf.data_ptr(), bf.data_ptr()
        self.w = w
        self._ws = None

    def forward(self, points, out=None):
        """points [P, N, 3] fp32 (device), P >= 0, N >= 1 -> [P, feat_dim] fp32 (``out``: any row stride, unit column stride)."""
        if points.device.type != "cuda":
            raise _lib.DaError("PointNetEngine.forward: the point clouds must live on the ROCm device")
        assert points.dim() == 3 and points.shape[2] == 3, tuple(points.shape)
        x = points.detach().to(torch.float32).contiguous()
        P, N = int(x.shape[0]), int(x.shape[1])
        if out is None:
            out = torch.empty(P, self.feat_dim, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.shape == (P, self.feat_dim) and (P == 0 or out.stride(1) == 1)
        if P == 0:
            return out
        need = self.lib.da_pointnet_workspace_bytes(P, N, self.feat_dim)
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.da_pointnet_forward(self.w, P, N, _lib.ptr(x), _lib.ptr(out), out.stride(0),
                                                _lib.ptr(self._ws) if need else None, self._ws.numel() if need else 0,
                                                _lib.stream_ptr(self.device)))
        return out


class PointNetTrainEngine:
    """Train-mode PointNet of a live ``PointNet`` module.  The parameters are packed from their CURRENT values on every call (they
    change every optimizer step); the saved state of a call belongs to that call's autograd context."""

    def __init__(self, net):
        self.net = net
        self.lib = _lib.lib()
        self._ws = None

    def params(self):
        """The tensors the autograd Function differentiates, in its argument order: per layer conv weight, BatchNorm weight, bias."""
        out = []
        for l in range(LAYERS):
            bn = getattr(self.net, f"bn{l + 1}")
            out += [getattr(self.net, f"conv{l + 1}").weight, bn.weight, bn.bias]
        return out

    def _bns(self):
        bns = [getattr(self.net, f"bn{l + 1}") for l in range(LAYERS)]
        for l, bn in enumerate(bns):
            if bn.momentum is None or not bn.track_running_stats or not bn.affine or bn.running_mean is None:
                raise NotImplementedError(f"bn{l + 1}: the train-mode HIP encoder implements BatchNorm with affine=True, "
                                          "track_running_stats=True and a numeric momentum (what the reference builds)")
        return bns

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def _pack(self, params, device):
        keep = []
        w = _lib.DaPointnetTrainWeights()

        def keep_(t):
            t = t.detach().to(device, torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        bns = self._bns()
        feat = int(params[3 * 4].shape[0])
        w.feat_dim = feat
        for l, bn in enumerate(bns):
            cw = params[3 * l].detach().reshape(params[3 * l].shape[0], -1)
            assert cw.shape[1] == WIDTHS_IN[l], (l, tuple(cw.shape))
            w.w[l] = keep_(cw)
            if l:
                w.wt[l] = keep_(cw.t())
            w.gamma[l], w.beta[l] = keep_(params[3 * l + 1]), keep_(params[3 * l + 2])
            w.running_mean[l], w.running_var[l] = keep_(bn.running_mean), keep_(bn.running_var)
            w.momentum[l], w.eps[l] = float(bn.momentum), float(bn.eps)
        return w, keep, bns, feat

    def run_forward(self, points, params):
        """-> (out, state, packed weights, kept tensors).  Updates every BatchNorm buffer of the module in place."""
        if points.device.type != "cuda":
            raise _lib.DaError("PointNetTrainEngine: the point clouds must live on the ROCm device")
        assert points.dim() == 3 and points.shape[2] == 3, tuple(points.shape)
        x = points.detach().to(torch.float32).contiguous()
        P, N = int(x.shape[0]), int(x.shape[1])
        if P * N == 1:          # what bn1 raises in the reference (pointnet.py:34)
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([1, 64, 1])}")
        dev = x.device
        w, keep, bns, feat = self._pack(params, dev)
        out = torch.empty(P, feat, dtype=torch.float32, device=dev)
        if P == 0:
            return out, None, w, keep
        state = torch.empty(self.lib.da_pointnet_train_state_bytes(P, N, feat), dtype=torch.uint8, device=dev)
        ws = self._workspace(self.lib.da_pointnet_train_workspace_bytes(P, N, feat), dev)
        run_out = torch.empty(LAYERS, 2, 128, dtype=torch.float32, device=dev)
        _lib.check(self.lib.da_pointnet_train_forward(w, P, N, _lib.ptr(x), _lib.ptr(out), out.stride(0), _lib.ptr(run_out),
                                                      _lib.ptr(state), state.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        with torch.no_grad():
            for l, bn in enumerate(bns):
                c = bn.running_mean.numel()
                bn.running_mean.copy_(run_out[l, 0, :c])
                bn.running_var.copy_(run_out[l, 1, :c])
                bn.num_batches_tracked.add_(1)
        keep.append(x)
        return out, state, w, keep

    def run_backward(self, points, params, grad_out, state, w):
        P, N = int(points.shape[0]), int(points.shape[1])
        dev = points.device
        grads = [torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in params]
        if P == 0:
            return [t.to(p.dtype) for t, p in zip(grads, params)]
        g = _lib.DaPointnetTrainGrads()
        for l in range(LAYERS):
            g.w[l], g.gamma[l], g.beta[l] = (grads[3 * l + k].data_ptr() for k in range(3))
        go = grad_out.detach().to(torch.float32).contiguous()
        ws = self._workspace(self.lib.da_pointnet_train_workspace_bytes(P, N, int(w.feat_dim)), dev)
        x = points.detach().to(torch.float32).contiguous()
        _lib.check(self.lib.da_pointnet_train_backward(w, P, N, _lib.ptr(x), _lib.ptr(go), go.stride(0), _lib.ptr(state), g,
                                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return [t.to(p.dtype) for t, p in zip(grads, params)]

    def forward(self, points):
        """train-mode forward; through the autograd Function when a gradient is wanted, else the forward alone."""
        if points.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("PointNet: the point clouds are data and get no gradient (as in the reference's training step); "
                                      "detach them")
        params = self.params()
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return PointNetTrainFunction.apply(self, points, *params)
        return self.run_forward(points, params)[0]


class PointNetTrainFunction(torch.autograd.Function):
    """PointNet.forward in train() mode as one autograd node: inputs (engine, points, *engine.params()), output [P, feat_dim].  The
    backward returns the gradients of every parameter; the saved state (pre-normalisation rows, batch statistics, arg-max
    points) is this context's own."""

    @staticmethod
    def forward(ctx, eng, points, *params):
        out, state, w, keep = eng.run_forward(points, params)
        ctx.eng, ctx.state, ctx.w, ctx.keep = eng, state, w, keep
        ctx.save_for_backward(points, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        points, *params = ctx.saved_tensors
        grads = ctx.eng.run_backward(points, params, grad_out, ctx.state, ctx.w)
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])]
        return (None, None, *grads)
