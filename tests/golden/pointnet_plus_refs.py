"""Contract of the PointNet++ fragment encoder (include/diffassemble_hip.h, "PointNet++ fragment encoder";
diffassemble_amd/csrc/da_pointnet_plus.hip): the eval forward of ``PointNetPlus(normal_channel=False)`` on a state dict with the
reference's keys, restated.  The discrete part -- farthest point sampling and the ball query -- follows the selection rule in
numpy float32, every operation rounded on its own; everything after it runs in the dtype of its operands (the tests pass fp64).
tests/test_pointnet_plus_host.py holds it against the reference's own module (tests/golden/pointnet_plus_v1.npz, written by
make_pointnet_plus_golden.py), tests/test_gpu_pointnet_plus.py holds the HIP kernels against it.

Also here: the generators of the fixture's weights and clouds (numpy ``default_rng`` seeds; the fixture stores SHA-256 digests, not
the 1.47 M weights)."""
import hashlib

import numpy as np
import torch

EPS = 1e-5
S1, K1, R1 = 512, 32, 0.2
S2, K2, R2 = 128, 64, 0.4
SA_WIDTHS = ((6, 64, 64, 128), (131, 128, 128, 256), (259, 256, 512, 1024))
CASES = [(1, 1), (1, 64), (2, 513), (3, 1000), (2, 2048), (20, 1000)]
WEIGHT_SEED = 20250
F32 = np.float32


# ------------------------------------------------------------------------------------------------------ generators
def _bn(rng, c, out, name, dims):
    sign = np.where(rng.random(c) < 0.25, -1.0, 1.0)
    out[f"{name}.weight"] = (sign * (0.5 + rng.random(c))).astype(F32)
    out[f"{name}.bias"] = (0.3 * rng.standard_normal(c)).astype(F32)
    out[f"{name}.running_mean"] = (0.3 * rng.standard_normal(c)).astype(F32)
    out[f"{name}.running_var"] = (0.25 + 1.5 * rng.random(c)).astype(F32)
    out[f"{name}.num_batches_tracked"] = np.array(0, dtype=np.int64)


def make_weights(seed=WEIGHT_SEED):
    """The state dict of PointNetPlus() as numpy arrays, in the module's key order: He-scaled Gaussian layers (the six coordinate
    columns of sa1's first layer three times that: the coordinates are small), 0.1 randn biases, BatchNorm statistics and affine
    parameters that leave nothing trivial (running mean 0.3 randn, running var in [0.25, 1.75], |gamma| in [0.5, 1.5] with about
    a quarter negative, beta 0.3 randn)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for s, widths in enumerate(SA_WIDTHS):
        for i in range(3):
            cin, cout = widths[i], widths[i + 1]
            gain = (3.0 if (s, i) == (0, 0) else 1.0) * np.sqrt(2.0 / cin)
            sd[f"sa{s + 1}.mlp_convs.{i}.weight"] = (gain * rng.standard_normal((cout, cin, 1, 1))).astype(F32)
            sd[f"sa{s + 1}.mlp_convs.{i}.bias"] = (0.1 * rng.standard_normal(cout)).astype(F32)
        for i in range(3):
            _bn(rng, widths[i + 1], sd, f"sa{s + 1}.mlp_bns.{i}", 2)
    for j, (cin, cout) in enumerate(((1024, 512), (512, 256))):
        sd[f"fc{j + 1}.weight"] = (np.sqrt(2.0 / cin) * rng.standard_normal((cout, cin))).astype(F32)
        sd[f"fc{j + 1}.bias"] = (0.1 * rng.standard_normal(cout)).astype(F32)
        _bn(rng, cout, sd, f"bn{j + 1}", 1)
    return sd


def state(dtype=torch.float32, seed=WEIGHT_SEED):
    return {k: torch.from_numpy(v).to(dtype if v.dtype.kind == "f" else torch.int64) for k, v in make_weights(seed).items()}


def make_cloud(P, N, seed, scale=0.3):
    """scale * randn rounded to fp16, as float32 [P, N, 3]."""
    return (scale * np.random.default_rng(seed).standard_normal((P, N, 3))).astype(np.float16).astype(F32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------ the selection rule
def d2(p, q):
    """fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), d* = fl(p* - q*): float32 arrays [..., 3], broadcast."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    assert dx.dtype == F32
    return (dx * dx + dy * dy) + dz * dz


def fps(points, npoint, start):
    """points [P, N, 3] float32, start [P] -> int64 [P, npoint]: the farthest point so far, ties to the LOWEST index."""
    points = np.asarray(points, F32)
    P, N = points.shape[:2]
    dist = np.full((P, N), 1e10, F32)
    far = np.asarray(start, np.int64).copy()
    idx = np.zeros((P, npoint), np.int64)
    rows = np.arange(P)
    for i in range(npoint):
        idx[:, i] = far
        dist = np.minimum(dist, d2(points, points[rows, far][:, None, :]))
        far = np.argmax(dist, axis=1)                  # numpy's argmax returns the first maximum
    return idx


def ball_query(points, centre, radius, nsample):
    """points [P, N, 3] float32, centre int [P, S] (indices among the N points) -> int64 [P, S, nsample]: the first nsample n in
    ascending order for which d2(centre, x_n) > float32(radius ** 2) is FALSE, the rest filled with the first of them."""
    points = np.asarray(points, F32)
    P, N = points.shape[:2]
    centre = np.asarray(centre, np.int64)
    out = np.zeros((P, centre.shape[1], nsample), np.int64)
    r2 = F32(radius ** 2)
    for p in range(P):
        member = ~(d2(points[p][centre[p]][:, None, :], points[p][None, :, :]) > r2)       # [S, N]
        rank = np.cumsum(member, axis=1) - 1
        out[p] = np.argmax(member, axis=1)[:, None]
        s, n = np.nonzero(member & (rank < nsample))
        out[p, s, rank[s, n]] = n
    return out


def select(points, start1, start2):
    """Both levels' selections of a float32 cloud [P, N, 3] -> dict(fps1 [P, 512], grp1 [P, 512, 32], fps2 [P, 128] (indices among
    the 512), grp2 [P, 128, 64] (likewise))."""
    points = np.asarray(points, F32)
    rows = np.arange(points.shape[0])[:, None]
    fps1 = fps(points, S1, start1)
    grp1 = ball_query(points, fps1, R1, K1)
    l1_xyz = points[rows, fps1]
    fps2 = fps(l1_xyz, S2, start2)
    grp2 = ball_query(l1_xyz, fps2, R2, K2)
    return dict(fps1=fps1, grp1=grp1, fps2=fps2, grp2=grp2)


# ------------------------------------------------------------------------------------------------------ the layers
def _bn_eval(sd, name, y):
    r = 1.0 / torch.sqrt(sd[f"{name}.running_var"] + EPS)
    return sd[f"{name}.weight"] * (y - sd[f"{name}.running_mean"]) * r + sd[f"{name}.bias"]


def _stack(sd, level, rows):
    """rows [..., cin] -> three times relu(bn(conv)) -> [..., cout]."""
    for i in range(3):
        w = sd[f"sa{level}.mlp_convs.{i}.weight"][:, :, 0, 0]
        rows = torch.relu(_bn_eval(sd, f"sa{level}.mlp_bns.{i}", rows @ w.t() + sd[f"sa{level}.mlp_convs.{i}.bias"]))
    return rows


def eval_forward(sd, pts, sel):
    """pts [P, N, 3] (torch, the dtype of sd), sel = select(...) -> [P, 256]; one fragment at a time."""
    out = []
    for p in range(pts.shape[0]):
        x = pts[p]
        f1, g1, f2, g2 = (torch.from_numpy(sel[k][p]) for k in ("fps1", "grp1", "fps2", "grp2"))
        l1_xyz = x[f1]                                                                           # [512, 3]
        l1 = _stack(sd, 1, torch.cat([x[g1] - l1_xyz[:, None, :], x[g1]], -1)).max(dim=1).values  # [512, 128]
        l2_xyz = l1_xyz[f2]                                                                      # [128, 3]
        l2 = _stack(sd, 2, torch.cat([l1_xyz[g2] - l2_xyz[:, None, :], l1[g2]], -1)).max(dim=1).values   # [128, 256]
        l3 = _stack(sd, 3, torch.cat([l2_xyz, l2], -1)).max(dim=0).values                        # [1024]
        h = torch.relu(_bn_eval(sd, "bn1", l3 @ sd["fc1.weight"].t() + sd["fc1.bias"]))
        out.append(torch.relu(_bn_eval(sd, "bn2", h @ sd["fc2.weight"].t() + sd["fc2.bias"])))
    return torch.stack(out) if out else pts.new_zeros(0, 256)
