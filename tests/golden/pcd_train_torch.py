"""Torch restatement (TEST INFRASTRUCTURE) of the reference's 3D piece encoder in train() mode, written from the maths of
vnn/vn_layers.py:50-91,133-154 and vn_dgcnn.py:34-74 (batch-statistics VNBatchNorm), point-major like oracle/vn_dgcnn.py:
a vector-neuron map is [..., C, 3].  Differentiable with torch autograd; any dtype / device.  Used as the torch baseline of
tests/tools/pcd_train_bench.py; pinned to tests/golden/pcd_train_v1.npz by tests/test_pcd_train_host.py.  The running
statistics are not tracked (only the forward / backward arithmetic is restated)."""
import torch


def torch_layer(x, wf, wd, g, b, dims, eps=1e-5):
    """VNLinearLeakyReLU with batch-statistics VNBatchNorm over `dims`; x [..., Cin, 3] -> [..., Cout, 3]."""
    p = torch.einsum("oc,...ck->...ok", wf, x)
    d = torch.einsum("oc,...ck->...ok", wd, x)
    n = p.norm(dim=-1) + 1e-6
    mu, var = n.mean(dims, keepdim=True), n.var(dims, unbiased=False, keepdim=True)
    y = (n - mu) / torch.sqrt(var + eps) * g + b
    p = p / n[..., None] * y[..., None]
    dot = (p * d).sum(-1, keepdim=True)
    mask = (dot >= 0).to(p.dtype)
    dsq = (d * d).sum(-1, keepdim=True)
    return 0.2 * p + 0.8 * (mask * p + (1 - mask) * (p - dot / (dsq + 1e-6) * d))


def torch_graph(x, k=20):
    """x [P, N, C, 3] -> cat(x_j - x_i, x_i) over the k nearest j: [P, N, k, 2C, 3]."""
    P, N, C, _ = x.shape
    f = x.reshape(P, N, C * 3)
    with torch.no_grad():
        sc = -(f * f).sum(-1)[:, :, None] + 2 * f @ f.transpose(1, 2) - (f * f).sum(-1)[:, None, :]
        idx = sc.topk(k, dim=-1)[1]
    nb = torch.gather(x[:, None].expand(P, N, N, C, 3), 2, idx[..., None, None].expand(P, N, k, C, 3))
    ctr = x[:, :, None].expand_as(nb)
    return torch.cat([nb - ctr, ctr], dim=3)


def torch_encoder(net, pts, inv=False):
    """train-mode VN_DGCNN.forward restated on torch ops: [P, N, 3] -> [P, 6 feat] (or [P, 2 feat] with ``inv``).
    ``net``: anything with ``named_parameters()`` in the reference's key layout (a VN_DGCNN module)."""
    sd = dict(net.named_parameters())

    def L(name, x, dims):
        return torch_layer(x, sd[f"{name}.map_to_feat.weight"], sd[f"{name}.map_to_dir.weight"],
                           sd[f"{name}.batchnorm.bn.weight"], sd[f"{name}.batchnorm.bn.bias"], dims)

    e = (0, 1, 2)
    x = pts[:, :, None, :]
    x1 = L("conv2", L("conv1", torch_graph(x), e), e).mean(2)
    x2 = L("conv4", L("conv3", torch_graph(x1), e), e).mean(2)
    x3 = L("conv5", torch_graph(x2), e).mean(2)
    y = L("conv6", torch.cat([x1, x2, x3], 2), (0, 1)).mean(1)
    y = torch.cat([y, y], 1)                                                     # [P, 2 feat, 3]
    if inv:
        return (y @ sd["linear0.weight"].T + sd["linear0.bias"]).mean(1)
    return y.reshape(pts.shape[0], -1)
