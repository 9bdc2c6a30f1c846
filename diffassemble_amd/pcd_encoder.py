"""Host side of the 3D piece encoder: packs the reference's ``VN_DGCNN`` state dict
(/root/reference/puzzle_diff/model/backbones/vnn/vn_dgcnn.py:7-31) into the fp32 blobs ``da_pcd_encoder_forward`` reads
(include/diffassemble_hip.h) and owns the workspace.  Also the two point-cloud primitives around it: ``knn`` (the
encoder's neighbour search, vn_dgcnn.py:114-120) and ``nearest_sq`` (the K = 1 search behind the part-accuracy metric,
chamfer_distance.py:148-149).  No torch arithmetic on the data path, no CPU fallback."""
import torch

from . import _lib

STAGES = (("conv1", "conv2", 1), ("conv3", "conv4", 21), ("conv5", None, 21))
BN_EPS = 1e-5


def _bn_affine(sd, name):
    """eval BatchNorm of the vector norm as  norm * scale + shift  (vn_layers.py:145-154)."""
    g, b = sd[f"{name}.batchnorm.bn.weight"].double(), sd[f"{name}.batchnorm.bn.bias"].double()
    mu, var = sd[f"{name}.batchnorm.bn.running_mean"].double(), sd[f"{name}.batchnorm.bn.running_var"].double()
    scale = g / torch.sqrt(var + BN_EPS)
    return torch.stack([scale, b - mu * scale]).float()


class PcdEncoderEngine:
    """Packed VN-DGCNN.  ``sd``: state dict with the reference's ``VN_DGCNN(feat_dim)`` keys (``pcd_backbone.*`` of an
    ``Eff_GAT_3d`` checkpoint with the prefix stripped).  ``inv`` selects the ``vn_dgcnn_inv`` output (linear0 path)."""

    def __init__(self, sd, *, inv=False, device=None, chunk=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.DaError("PcdEncoderEngine needs a ROCm device (no CPU path in diffassemble_amd)")
        self.lib = _lib.lib()
        self.inv, self.chunk = bool(inv), chunk
        sd = {k: v.detach().to(self.device, torch.float32) for k, v in sd.items() if v.is_floating_point()}
        self._keep = []
        w = _lib.DaPcdEncoderWeights()

        def keep(*ts):
            t = torch.cat([x.reshape(-1) for x in ts]).to(torch.float32).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        for s, (a, b, cin) in enumerate(STAGES):
            wf, wd = sd[f"{a}.map_to_feat.weight"], sd[f"{a}.map_to_dir.weight"]          # [21, 2 cin]
            assert wf.shape == (21, 2 * cin) and wd.shape == (21, 2 * cin), (a, tuple(wf.shape), tuple(wd.shape))
            w.premap[s] = keep(wf[:, :cin], wd[:, :cin], wf[:, cin:] - wf[:, :cin], wd[:, cin:] - wd[:, :cin])
            w.bn_a[s] = keep(_bn_affine(sd, a))
            if b is not None:
                # rows zero-padded to 22: a (c, c + 1) weight pair is one 64-bit scalar operand of a packed fp32 FMA
                pad = torch.nn.functional.pad
                w.conv_b[s] = keep(pad(sd[f"{b}.map_to_feat.weight"], (0, 1)), pad(sd[f"{b}.map_to_dir.weight"], (0, 1)),
                                   _bn_affine(sd, b))
        w6, d6 = sd["conv6.map_to_feat.weight"], sd["conv6.map_to_dir.weight"]
        self.feat_dim = int(w6.shape[0])
        assert w6.shape[1] == 63 and tuple(d6.shape) == (1, 63), (tuple(w6.shape), tuple(d6.shape))
        w.feat_dim = self.feat_dim
        w.conv6 = keep(w6, d6, _bn_affine(sd, "conv6"))
        if "linear0.weight" in sd:
            assert tuple(sd["linear0.weight"].shape) == (2 * self.feat_dim, 3)
            w.linear0 = keep(sd["linear0.weight"], sd["linear0.bias"])
        self.w = w
        self.out_dim = 2 * self.feat_dim if self.inv else 6 * self.feat_dim
        self._ws, self._ws_key = None, None

    def _chunk_for(self, n_parts, n_points):
        if self.chunk:
            return int(self.chunk)
        # ~1.9 KB of workspace per point: keep a chunk under ~2 GB
        return max(1, min(n_parts, (1 << 20) // max(n_points, 1)))

    def forward(self, points, out=None):
        """points [P, N, 3] fp32 (device), N >= 20 -> [P, 6 feat_dim] (or [P, 2 feat_dim] for inv) fp32."""
        if points.device.type != "cuda":
            raise _lib.DaError("PcdEncoderEngine.forward: the point clouds must live on the ROCm device")
        assert points.dim() == 3 and points.shape[2] == 3, tuple(points.shape)
        x = points.detach().to(torch.float32).contiguous()
        P, N = int(x.shape[0]), int(x.shape[1])
        if out is None:
            out = torch.empty(P, self.out_dim, dtype=torch.float32, device=self.device)
        if P == 0:
            return out
        chunk = self._chunk_for(P, N)
        key = (N, chunk)
        if self._ws_key != key:
            self._ws = torch.empty(self.lib.da_pcd_encoder_workspace_bytes(N, chunk, self.feat_dim), dtype=torch.uint8,
                                   device=self.device)
            self._ws_key = key
        assert out.dtype == torch.float32 and out.shape == (P, self.out_dim) and out.stride(1) == 1
        _lib.check(self.lib.da_pcd_encoder_forward(self.w, P, N, _lib.ptr(x), int(self.inv), _lib.ptr(out), out.stride(0),
                                                   _lib.ptr(self._ws), self._ws.numel(), chunk,
                                                   _lib.stream_ptr(self.device)))
        return out


def knn(x, k=_lib.PCD_K):
    """x [B, N, F] fp32 on the device, F == 3 or F <= 64 -> idx [B, N, k] int32: the k nearest points of the same cloud
    (self included), nearest first (vn_dgcnn.py:114-120; ties towards the lower index)."""
    if x.device.type != "cuda":
        raise _lib.DaError("knn: the clouds must live on the ROCm device")
    B, N, F = x.shape
    x = x.detach().to(torch.float32)
    if F == 3:
        x, ldx = x.contiguous(), 3
    else:
        assert F <= 64, F
        pad = torch.zeros(B, N, 64, dtype=torch.float32, device=x.device)
        pad[:, :, :F] = x
        x, ldx = pad, 64
    idx = torch.empty(B, N, k, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().da_knn(B, N, F, _lib.ptr(x), ldx, k, _lib.ptr(idx), _lib.stream_ptr(x.device)))
    return idx


def nearest_sq(a, b):
    """a [P, N, 3], b [P, M, 3] fp32 on the device -> (d_ab [P, N], d_ba [P, M]): squared distance from every point to the
    nearest point of the other cloud (pytorch3d ``knn_points(K=1)`` both ways, chamfer_distance.py:148-149)."""
    if a.device.type != "cuda" or b.device.type != "cuda":
        raise _lib.DaError("nearest_sq: the clouds must live on the ROCm device")
    a, b = a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
    P, N, _ = a.shape
    M = b.shape[1]
    assert b.shape[0] == P and a.shape[2] == 3 and b.shape[2] == 3
    d_ab = torch.empty(P, N, dtype=torch.float32, device=a.device)
    d_ba = torch.empty(P, M, dtype=torch.float32, device=a.device)
    if P:
        _lib.check(_lib.lib().da_nearest_sq(P, N, M, _lib.ptr(a), _lib.ptr(b), _lib.ptr(d_ab), _lib.ptr(d_ba),
                                            _lib.stream_ptr(a.device)))
    return d_ab, d_ba


# ---- train() mode (batch-statistics BatchNorm, backward) ---------------------------------------------------------------
CONVS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6")
BATCHNORMS = CONVS + ("VnInv.vn1", "VnInv.vn2")       # layer order of da_pcd_train_weights
_TRAIN_BYTES_PER_POINT = 31 * 1024                  # the backward's per-edge buffers of one chunk, per point


class PcdTrainEngine:
    """Train-mode VN-DGCNN of a live ``VN_DGCNN`` module (da_pcd_train_forward / _backward).  The parameters are packed
    from their CURRENT values on every call (they change every optimizer step); the saved state of a call belongs to
    that call's autograd context.  ``chunk``: fragments per pass of the backward's per-edge buffers (default: ~1 GB)."""

    def __init__(self, net, *, chunk=None):
        self.net, self.chunk = net, chunk
        self.lib = _lib.lib()
        self._ws = None

    def params(self):
        """The tensors the autograd Function differentiates, in its argument order: per conv1..conv6 map_to_feat,
        map_to_dir, BatchNorm weight, bias; then linear0 weight, bias."""
        out = []
        for n in CONVS:
            m = self.net.get_submodule(n)
            out += [m.map_to_feat.weight, m.map_to_dir.weight, m.batchnorm.bn.weight, m.batchnorm.bn.bias]
        return out + [self.net.linear0.weight, self.net.linear0.bias]

    def _bns(self):
        bns = [self.net.get_submodule(n).batchnorm.bn for n in BATCHNORMS]
        for n, bn in zip(BATCHNORMS, bns):
            if bn.momentum is None or not bn.track_running_stats or not bn.affine or bn.running_mean is None:
                raise NotImplementedError(f"{n}.batchnorm.bn: the train-mode HIP encoder implements BatchNorm with affine=True, "
                                          "track_running_stats=True and a numeric momentum (what the reference builds)")
        return bns

    def chunk_for(self, n_parts, n_points):
        if self.chunk:
            return max(1, min(n_parts, int(self.chunk)))
        return max(1, min(n_parts, (1 << 30) // (n_points * _TRAIN_BYTES_PER_POINT)))

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def _pack(self, params, device):
        """da_pcd_train_weights from the live parameters (detached fp32 copies kept in the returned list)."""
        keep = []
        w = _lib.DaPcdTrainWeights()

        def keep_(*ts):
            t = torch.cat([x.detach().reshape(-1).to(device, torch.float32) for x in ts]).contiguous()
            keep.append(t)
            return t.data_ptr()

        def scratch(n):
            t = torch.zeros(n, dtype=torch.float32, device=device)
            keep.append(t)
            return t.data_ptr()

        p = {n: params[4 * i: 4 * i + 4] for i, n in enumerate(CONVS)}
        pad = torch.nn.functional.pad
        for s, (a, b, cin) in enumerate(STAGES):
            wf, wd = p[a][0].detach(), p[a][1].detach()
            assert wf.shape == (21, 2 * cin) and wd.shape == (21, 2 * cin), (a, tuple(wf.shape))
            w.premap[s] = keep_(wf[:, :cin], wd[:, :cin], wf[:, cin:] - wf[:, :cin], wd[:, cin:] - wd[:, :cin])
            w.bn_a[s] = scratch(2 * 21)
            if b is not None:
                w.conv_b[s] = keep_(pad(p[b][0].detach(), (0, 1)), pad(p[b][1].detach(), (0, 1)), torch.zeros(2 * 21, device=device))
        w6, d6 = p["conv6"][0].detach(), p["conv6"][1].detach()
        feat = int(w6.shape[0])
        assert w6.shape[1] == 63 and tuple(d6.shape) == (1, 63), (tuple(w6.shape), tuple(d6.shape))
        w.feat_dim = feat
        w.conv6 = keep_(w6, d6, torch.zeros(2 * feat, device=device))
        w.linear0 = keep_(params[24], params[25])
        bns = self._bns()
        for l, bn in enumerate(bns):
            if l < 6:
                g, b_ = p[CONVS[l]][2], p[CONVS[l]][3]
            else:
                g, b_ = bn.weight, bn.bias
            w.gamma[l], w.beta[l] = keep_(g), keep_(b_)
            w.running_mean[l], w.running_var[l] = keep_(bn.running_mean), keep_(bn.running_var)
            w.momentum[l], w.eps[l] = float(bn.momentum), float(bn.eps)
        for v, n in enumerate(("VnInv.vn1", "VnInv.vn2")):
            m = self.net.get_submodule(n)
            w.inv_wf[v], w.inv_wd[v] = keep_(m.map_to_feat.weight), keep_(m.map_to_dir.weight)
        return w, keep, bns, feat

    def run_forward(self, points, params, inv):
        """-> (out, state, packed weights, kept tensors).  Updates every BatchNorm buffer of the module in place."""
        if points.device.type != "cuda":
            raise _lib.DaError("PcdTrainEngine: the point clouds must live on the ROCm device")
        assert points.dim() == 3 and points.shape[2] == 3, tuple(points.shape)
        x = points.detach().to(torch.float32).contiguous()
        P, N = int(x.shape[0]), int(x.shape[1])
        dev = x.device
        w, keep, bns, feat = self._pack(params, dev)
        out = torch.empty(P, 2 * feat if inv else 6 * feat, dtype=torch.float32, device=dev)
        state = torch.empty(self.lib.da_pcd_train_state_bytes(P, N, feat), dtype=torch.uint8, device=dev)
        ws = self._workspace(self.lib.da_pcd_train_workspace_bytes(P, N, self.chunk_for(P, N), feat), dev)
        run_out = torch.empty(len(BATCHNORMS), 2, 256, dtype=torch.float32, device=dev)
        _lib.check(self.lib.da_pcd_train_forward(w, P, N, _lib.ptr(x), int(inv), _lib.ptr(out), out.stride(0), _lib.ptr(run_out),
                                                 _lib.ptr(state), state.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        with torch.no_grad():
            for l, bn in enumerate(bns):
                c = bn.running_mean.numel()
                bn.running_mean.copy_(run_out[l, 0, :c])
                bn.running_var.copy_(run_out[l, 1, :c])
                bn.num_batches_tracked.add_(1)
        keep.append(x)
        return out, state, w, keep

    def run_backward(self, points, params, inv, grad_out, state, w, need_points):
        P, N = int(points.shape[0]), int(points.shape[1])
        dev = points.device
        feat = int(w.feat_dim)
        grads = [torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in params]
        gpts = torch.zeros(P, N, 3, dtype=torch.float32, device=dev) if need_points else None
        g = _lib.DaPcdTrainGrads()
        for l in range(6):
            g.wf[l], g.wd[l], g.gamma[l], g.beta[l] = (grads[4 * l + k].data_ptr() for k in range(4))
        if inv:
            g.linear0_w, g.linear0_b = grads[24].data_ptr(), grads[25].data_ptr()
        g.points = None if gpts is None else gpts.data_ptr()
        go = grad_out.detach().to(torch.float32).contiguous()
        chunk = self.chunk_for(P, N)
        ws = self._workspace(self.lib.da_pcd_train_workspace_bytes(P, N, chunk, feat), dev)
        x = points.detach().to(torch.float32).contiguous()
        _lib.check(self.lib.da_pcd_train_backward(w, P, N, _lib.ptr(x), int(inv), _lib.ptr(go), go.stride(0), _lib.ptr(state), g,
                                                  _lib.ptr(ws), ws.numel(), chunk, _lib.stream_ptr(dev)))
        if not inv:
            grads[24] = grads[25] = None
        grads = [None if t is None else t.to(p.dtype) for t, p in zip(grads, params)]
        return (None if gpts is None else gpts.to(points.dtype)), grads

    def forward(self, points, inv):
        """train-mode forward; through the autograd Function when a gradient is wanted, else the forward alone."""
        params = self.params()
        if torch.is_grad_enabled() and (points.requires_grad or any(p.requires_grad for p in params)):
            return PcdTrainFunction.apply(self, bool(inv), points, *params)
        return self.run_forward(points, params, inv)[0]


class PcdTrainFunction(torch.autograd.Function):
    """VN_DGCNN.forward in train() mode as one autograd node: inputs (engine, inv, points, *engine.params()), output
    [P, 6 feat] (or [P, 2 feat] for inv).  The backward returns the gradients of the points and of every parameter; the
    saved state (neighbour lists, pooled maps, batch statistics) is this context's own."""

    @staticmethod
    def forward(ctx, eng, inv, points, *params):
        out, state, w, keep = eng.run_forward(points, params, inv)
        ctx.eng, ctx.inv, ctx.state, ctx.w, ctx.keep = eng, inv, state, w, keep
        ctx.save_for_backward(points, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        points, *params = ctx.saved_tensors
        gpts, grads = ctx.eng.run_backward(points, params, ctx.inv, grad_out, ctx.state, ctx.w, ctx.needs_input_grad[2])
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])]
        return (None, None, gpts, *grads)
