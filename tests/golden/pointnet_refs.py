"""fp64 contract of the PointNet fragment encoder (include/diffassemble_hip.h, "PointNet fragment encoder";
diffassemble_amd/csrc/da_pointnet.hip): the eval forward, the train() forward and its backward as EXPLICIT formulas on a state
dict with the reference's keys (conv{1..5}.weight [out, in, 1], bn{1..5}.{weight,bias,running_mean,running_var}).  Nothing here
calls autograd; tests/test_pointnet_host.py holds ``backward`` against torch autograd of ``train_forward`` and holds all three
against the reference's own module (tests/golden/pointnet_v1.npz, written by make_pointnet_golden.py), and
tests/test_gpu_pointnet.py holds the HIP kernels against them.

Every function runs in the dtype of its operands (the tests pass fp64).  With x_0 = the points [M, 3], M = P N, layer
l = 1..5:   y_l = x_{l-1} W_l^T,   z_l = gamma_l (y_l - m_l) r_l + beta_l,   x_l = relu(z_l) (l < 5),   out = max_n z_5,
where (m_l, r_l) = (running mean, 1 / sqrt(running var + eps)) in eval() and (mean over the M rows, 1 / sqrt(biased variance
over the M rows + eps)) in train()."""
from types import SimpleNamespace as NS

import torch

LAYERS, EPS, MOMENTUM = 5, 1e-5, 0.1


def _w(sd, l):
    return sd[f"conv{l}.weight"][:, :, 0]


def eval_forward(sd, pts):
    """pts [P, N, 3] -> [P, F]: BatchNorm on the running statistics."""
    P, N = pts.shape[:2]
    x = pts.reshape(P * N, 3)
    for l in range(1, LAYERS + 1):
        y = x @ _w(sd, l).t()
        r = 1.0 / torch.sqrt(sd[f"bn{l}.running_var"] + EPS)
        z = sd[f"bn{l}.weight"] * (y - sd[f"bn{l}.running_mean"]) * r + sd[f"bn{l}.bias"]
        x = torch.relu(z) if l < LAYERS else z
    return x.reshape(P, N, -1).max(dim=1).values


def first_argmax(z):
    """z [P, N, F] -> the LOWEST n attaining max_n z [P, F]."""
    hit = z == z.max(dim=1, keepdim=True).values
    n = torch.arange(z.shape[1], device=z.device).reshape(1, -1, 1).expand_as(z)
    return torch.where(hit, n, torch.full_like(n, z.shape[1])).min(dim=1).values


def top2_gap(z):
    """z [P, N, F] -> the difference between the largest and the second largest value over n [P, F] (inf for N == 1)."""
    if z.shape[1] < 2:
        return torch.full(z[:, 0].shape, float("inf"), dtype=z.dtype)
    t = torch.topk(z, 2, dim=1).values
    return t[:, 0] - t[:, 1]


def train_forward(sd, pts):
    """pts [P, N, 3] -> NS(out [P, F], x (inputs of the layers), y, xhat, r (lists over the layers), z5 [P, N, F], arg [P, F],
    run_mean, run_var (lists: the updated running statistics))."""
    P, N = pts.shape[:2]
    M = P * N
    x = pts.reshape(M, 3)
    f = NS(x=[], y=[], xhat=[], r=[], z=[], run_mean=[], run_var=[])
    for l in range(1, LAYERS + 1):
        y = x @ _w(sd, l).t()
        mean = y.sum(0) / M
        var = ((y - mean) ** 2).sum(0) / M
        r = 1.0 / torch.sqrt(var + EPS)
        xhat = (y - mean) * r
        z = sd[f"bn{l}.weight"] * xhat + sd[f"bn{l}.bias"]
        f.x.append(x); f.y.append(y); f.xhat.append(xhat); f.r.append(r); f.z.append(z)
        f.run_mean.append((1 - MOMENTUM) * sd[f"bn{l}.running_mean"] + MOMENTUM * mean.detach())
        f.run_var.append((1 - MOMENTUM) * sd[f"bn{l}.running_var"] + MOMENTUM * var.detach() * M / (M - 1))
        x = torch.relu(z) if l < LAYERS else z
    f.z5 = x.reshape(P, N, -1)
    f.arg = first_argmax(f.z5.detach())
    f.out = torch.gather(f.z5, 1, f.arg[:, None, :])[:, 0]
    return f


def backward(sd, pts, f, d_out):
    """The gradients of sum(out * d_out) with respect to conv{l}.weight, bn{l}.weight, bn{l}.bias, from the forward's record."""
    P, N = pts.shape[:2]
    M = P * N
    dz = torch.zeros_like(f.z5)
    dz.scatter_(1, f.arg[:, None, :], d_out[:, None, :])          # the max routes the gradient to the arg-max row
    dz = dz.reshape(M, -1)
    grads = {}
    for l in range(LAYERS, 0, -1):
        if l < LAYERS:
            dz = dz * (f.z[l - 1] > 0)                            # ReLU
        xhat, gamma = f.xhat[l - 1], sd[f"bn{l}.weight"]
        s1, s2 = dz.sum(0), (dz * xhat).sum(0)
        grads[f"bn{l}.bias"], grads[f"bn{l}.weight"] = s1, s2
        dy = gamma * f.r[l - 1] * (dz - s1 / M - xhat * (s2 / M))
        grads[f"conv{l}.weight"] = (dy.t() @ f.x[l - 1])[:, :, None]
        dz = dy @ _w(sd, l)
    return grads


def param_keys():
    return [k for l in range(1, LAYERS + 1) for k in (f"conv{l}.weight", f"bn{l}.weight", f"bn{l}.bias")]
