"""Contract of the PointNet++ fragment encoder (include/diffassemble_hip.h, "PointNet++ fragment encoder";
diffassemble_amd/csrc/da_pointnet_plus.hip): the eval forward of ``PointNetPlus(normal_channel=False)`` on a state dict with the
reference's keys, restated.  The discrete part -- farthest point sampling and the ball query -- follows the selection rule in
numpy float32, every operation rounded on its own; everything after it runs in the dtype of its operands (the tests pass fp64).
tests/test_pointnet_plus_host.py holds it against the reference's own module (tests/golden/pointnet_plus_v1.npz, written by
make_pointnet_plus_golden.py), tests/test_gpu_pointnet_plus.py holds the HIP kernels against it.

Stage by stage (tests/test_pointnet_plus_stages_host.py, tests/test_gpu_pointnet_plus_stages.py): ``stage_sa`` / ``head`` are the
pieces of ``eval_forward``, ``stage_sa32`` / ``head32`` the same in plain fp32 on folded weights (the rounding scale the kernels are
held to, ``stage_bound``), ``stage_cases`` the inputs injected into one stage alone, ``decisive_positions`` the proof that a group's
every row decides some output cell.

Also here: the generators of the fixture's weights and clouds (numpy ``default_rng`` seeds; the fixture stores SHA-256 digests, not
the 1.47 M weights)."""
import hashlib
from types import SimpleNamespace

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


def stage_sa(sd, level, rows, dim=-2):
    """One level's stack and its maximum over the rows of a group: rows [..., K, cin] (``dim``: the axis of the K rows) ->
    (the stack's output BEFORE the maximum [..., K, cout], the maximum [..., cout]), in the dtype of sd."""
    pre = _stack(sd, level, rows)
    return pre, pre.max(dim=dim).values


def head(sd, part):
    """part [..., 4, 1024] (sa3's maxima per tile of 32 points) -> maximum over the tiles, fc1 / bn1 / relu, fc2 / bn2 / relu
    [..., 256]."""
    l3 = part.max(dim=-2).values
    h = torch.relu(_bn_eval(sd, "bn1", l3 @ sd["fc1.weight"].t() + sd["fc1.bias"]))
    return torch.relu(_bn_eval(sd, "bn2", h @ sd["fc2.weight"].t() + sd["fc2.bias"]))


def rows_sa1(x, f1, g1):
    """x [N, 3], f1 [512], g1 [512, 32] -> sa1's grouped rows [512, 32, 6] = [x_n - centre | x_n]."""
    return torch.cat([x[g1] - x[f1][:, None, :], x[g1]], -1)


def rows_sa2(x, f1, f2, g2, l1):
    """-> sa2's grouped rows [128, 64, 131] = [l1_xyz_n - centre | l1 feature]; f2 / g2 index the 512 points of level 1."""
    l1_xyz = x[f1]
    return torch.cat([l1_xyz[g2] - l1_xyz[f2][:, None, :], l1[g2]], -1)


def rows_sa3(x, f1, f2, l2):
    """-> sa3's rows [128, 259] = [l2_xyz | l2 feature]."""
    return torch.cat([x[f1][f2], l2], -1)


def eval_forward(sd, pts, sel):
    """pts [P, N, 3] (torch, the dtype of sd), sel = select(...) -> [P, 256]; one fragment at a time."""
    out = []
    for p in range(pts.shape[0]):
        x = pts[p]
        f1, g1, f2, g2 = (torch.from_numpy(sel[k][p]) for k in ("fps1", "grp1", "fps2", "grp2"))
        l1 = stage_sa(sd, 1, rows_sa1(x, f1, g1))[1]                                             # [512, 128]
        l2 = stage_sa(sd, 2, rows_sa2(x, f1, f2, g2, l1))[1]                                     # [128, 256]
        l3 = stage_sa(sd, 3, rows_sa3(x, f1, f2, l2), dim=0)[1]                                  # [1024]
        out.append(head(sd, l3[None, :]))
    return torch.stack(out) if out else pts.new_zeros(0, 256)


# ------------------------------------------------------------------------------------------------------ the same in plain fp32
def folded32(sd):
    """The engine's operands, restated: eval BatchNorm folded into every layer in fp64 (W' = diag(s) W, b' = (b - mean) s + beta,
    s = gamma / sqrt(var + eps)), rounded to fp32 once.  {"sa<level>": [(W, b)] * 3, "fc1": (W, b), "fc2": (W, b)}; the columns stay
    in the reference's order [xyz | features]."""
    def fold(w, b, bn):
        s = sd[f"{bn}.weight"].double() / torch.sqrt(sd[f"{bn}.running_var"].double() + EPS)
        return (w.double() * s[:, None]).float(), ((b.double() - sd[f"{bn}.running_mean"].double()) * s + sd[f"{bn}.bias"].double()).float()
    out = {f"sa{l}": [fold(sd[f"sa{l}.mlp_convs.{i}.weight"][:, :, 0, 0], sd[f"sa{l}.mlp_convs.{i}.bias"], f"sa{l}.mlp_bns.{i}") for i in range(3)]
           for l in (1, 2, 3)}
    for j in (1, 2):
        out[f"fc{j}"] = fold(sd[f"fc{j}.weight"], sd[f"fc{j}.bias"], f"bn{j}")
    return out


def stage_sa32(fw, level, rows, dim=-2):
    """stage_sa's maximum evaluated in plain fp32 on the folded weights (``fw = folded32(sd)``, rows fp32): an fp32 evaluation
    that is not the kernel's, whose distance from fp64 is the rounding scale the kernels are held to."""
    assert rows.dtype == torch.float32
    for w, b in fw[f"sa{level}"]:
        rows = torch.relu(rows @ w.t() + b)
    return rows.max(dim=dim).values


def head32(fw, part):
    assert part.dtype == torch.float32
    h = torch.relu(part.max(dim=-2).values @ fw["fc1"][0].t() + fw["fc1"][1])
    return torch.relu(h @ fw["fc2"][0].t() + fw["fc2"][1])


def decisive_positions(pre_max, dim, tol):
    """pre_max: a stage's values before its maximum over axis ``dim`` -> int64 [size of dim]: for each position along ``dim`` the
    number of cells (all other axes) in which that position holds the maximum by more than 2 tol, so that a maximum which leaves
    the position out, or reads another row in its place, is off by more than tol there."""
    x = pre_max.movedim(dim, -1)
    top = x.topk(2, dim=-1)
    clear = (top.values[..., 0] - top.values[..., 1]) > 2 * tol
    return torch.bincount(top.indices[..., 0][clear].reshape(-1), minlength=x.shape[-1])


# ------------------------------------------------------------------------------------------------------ injected stage inputs
STAGE_SEED = 31700
STAGE_TOL_FACTOR = 8          # kernel bound = 8 x (plain fp32 evaluation - fp64) of the same stage: another summation order of the same length
HEAD_MARGIN = 0.5             # by how much the winning tile of a head channel exceeds the other three (at least)


def _distinct(rng, groups, k, n):
    """[groups, k] int64: k distinct members of [0, n) per group, a random subset in random order."""
    return np.argsort(rng.random((groups, n)), axis=1)[:, :k]


def _edge_groups(grp, centre, n):
    """The groups kernels get wrong first, written over a few random ones of fragment 0 and the last fragment: all members one
    index (the ball query's padding), one holding index 0 and the last index, a centre at the last index."""
    k = grp.shape[-1]
    for p in (0, grp.shape[0] - 1):
        grp[p, 3] = 5 % n
        grp[p, 4, 0], grp[p, 4, k - 1] = 0, n - 1
        others = np.arange(1, n - 1)[:k - 2]
        if len(others) == k - 2:
            grp[p, 4, 1:k - 1] = others            # the group stays distinct
        centre[p, 5] = n - 1
        centre[p, grp.shape[1] - 1] = n - 1            # the last group of the fragment too
    return grp, centre


def _stage_case(stage, **kw):
    c = SimpleNamespace(stage=stage, coverage=True, pts=None, fps1=None, grp1=None, fps2=None, grp2=None, l1=None, l2=None, part=None)
    c.__dict__.update(kw)
    c.P, c.N = c.pts.shape[:2]
    return c


def _sa1_case(seed, P, N, last_member_in=None):
    rng = np.random.default_rng(seed)
    pts = make_cloud(P, N, seed + 1)
    fps1 = rng.integers(0, N, (P, S1))
    if N >= K1:
        grp1 = _distinct(rng, P * S1, K1, N).reshape(P, S1, K1)
        grp1, fps1 = _edge_groups(grp1, fps1, N)
    else:
        grp1 = rng.integers(0, N, (P, S1, K1))
    if last_member_in is not None:
        # every group of that fragment reads its last point, in row 7 (and all of group 6).  A group that drew N - 1 already now
        # holds it twice: with the edge groups, the few groups that are not 32 distinct members
        grp1[last_member_in, :, 7] = N - 1
        grp1[last_member_in, 6] = N - 1
    return _stage_case("sa1", pts=pts, fps1=fps1, grp1=grp1, coverage=N >= K1)


def stage_cases():
    """The injected inputs of the stage tests, {name: case}: every index in range (fps1 / grp1 in [0, N), fps2 / grp2 in [0, 512)),
    groups of DISTINCT members in random order so that every row position of a group decides some output cell, the edge groups of
    _edge_groups, features relu(randn) as fp32 and different per fragment.  int64 indices, float32 points and features (numpy)."""
    cases = {"sa1": _sa1_case(STAGE_SEED, 2, 64), "sa1_n2048": _sa1_case(STAGE_SEED + 10, 2, 2048, last_member_in=1),
             "sa1_n1": _sa1_case(STAGE_SEED + 20, 1, 1)}
    rng = np.random.default_rng(STAGE_SEED + 30)
    P, N = 2, 64
    fps2 = rng.integers(0, S1, (P, S2))
    fps2[:, 0], fps2[:, 1] = 0, S1 - 1
    grp2, fps2 = _edge_groups(_distinct(rng, P * S2, K2, S1).reshape(P, S2, K2), fps2, S1)
    cases["sa2"] = _stage_case("sa2", pts=make_cloud(P, N, STAGE_SEED + 31), fps1=rng.integers(0, N, (P, S1)), fps2=fps2, grp2=grp2,
                               l1=np.maximum(rng.standard_normal((P, S1, 128)), 0).astype(F32))
    rng = np.random.default_rng(STAGE_SEED + 40)
    P = 3
    cases["sa3"] = _stage_case("sa3", pts=make_cloud(P, N, STAGE_SEED + 41), fps1=rng.integers(0, N, (P, S1)), fps2=rng.integers(0, S1, (P, S2)),
                               l2=np.maximum(rng.standard_normal((P, S2, 256)), 0).astype(F32))
    rng = np.random.default_rng(STAGE_SEED + 50)
    P = 5                                              # the head takes four fragments per workgroup: the last one holds a single fragment
    part = (0.5 * np.maximum(rng.standard_normal((P, 4, 1024)), 0)).astype(F32)
    winner = rng.integers(0, 4, (P, 1024))
    lift = (part.max(axis=1) + HEAD_MARGIN + rng.random((P, 1024))).astype(F32)
    np.put_along_axis(part, winner[:, None, :], lift[:, None, :], axis=1)
    cases["head"] = _stage_case("head", pts=make_cloud(P, N, STAGE_SEED + 51), part=part)
    for c in cases.values():
        for k, hi in (("fps1", c.N), ("grp1", c.N), ("fps2", S1), ("grp2", S1)):
            v = getattr(c, k)
            assert v is None or (v.dtype == np.int64 and v.min() >= 0 and v.max() < hi), (c.stage, k)
    return cases


def stage_rows(c, dtype, pts=None, xyz=True):
    """The rows the case's stage reads, [P, groups, K, cin] (sa3: [P, 128, 259]) in ``dtype``.  ``pts``: other points than the
    case's (a mutation); ``xyz=False``: the coordinate columns of sa2 / sa3 left at zero (another)."""
    x = torch.from_numpy(c.pts if pts is None else pts).to(dtype)
    t = lambda a: torch.from_numpy(a)
    if c.stage == "sa1":
        return torch.stack([rows_sa1(x[p], t(c.fps1[p]), t(c.grp1[p])) for p in range(c.P)])
    if c.stage == "sa2":
        rows = torch.stack([rows_sa2(x[p], t(c.fps1[p]), t(c.fps2[p]), t(c.grp2[p]), t(c.l1[p]).to(dtype)) for p in range(c.P)])
    else:
        rows = torch.stack([rows_sa3(x[p], t(c.fps1[p]), t(c.fps2[p]), t(c.l2[p]).to(dtype)) for p in range(c.P)])
    if not xyz:
        rows[..., :3] = 0
    return rows


def stage_bound(ref64, ref32):
    """(E32, tol): E32 = max |ref32 - ref64| / max |ref64| over the whole stage tensor, tol = 8 E32 max |ref64| -- the bound, per
    element, of a kernel's output against ref64."""
    scale = float(ref64.abs().max())
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    return e32, STAGE_TOL_FACTOR * e32 * scale


def stage_reference(c, sd64, fw):
    """-> (pre, out64, out32, E32, tol) of a case: the stage's values before the maximum (fp64; the head: ``part``), its output in
    fp64 and in plain fp32, and stage_bound of the two."""
    if c.stage == "head":
        pre = torch.from_numpy(c.part).double()
        out64, out32 = head(sd64, pre), head32(fw, torch.from_numpy(c.part))
    else:
        level = int(c.stage[2])                        # the rows of a group (sa3: a fragment's 128 points) are axis -2 at every level
        pre, out64 = stage_sa(sd64, level, stage_rows(c, torch.float64))
        out32 = stage_sa32(fw, level, stage_rows(c, torch.float32))
    return (pre, out64, out32) + stage_bound(out64, out32)


def eval_chain(sd, pts, sel, fw=None):
    """eval_forward tensor by tensor: dict(l1 [P, 512, 128], l2 [P, 128, 256], l3 [P, 1024], out [P, 256]).  With ``fw``
    (folded32) the plain fp32 evaluation of the same chain, each stage on the fp32 output of the one before."""
    keep = dict(l1=[], l2=[], l3=[], out=[])
    sa = (lambda level, rows: stage_sa(sd, level, rows)[1]) if fw is None else (lambda level, rows: stage_sa32(fw, level, rows))
    for p in range(pts.shape[0]):
        x = pts[p]
        f1, g1, f2, g2 = (torch.from_numpy(sel[k][p]) for k in ("fps1", "grp1", "fps2", "grp2"))
        l1 = sa(1, rows_sa1(x, f1, g1))
        l2 = sa(2, rows_sa2(x, f1, f2, g2, l1))
        l3 = sa(3, rows_sa3(x, f1, f2, l2))
        out = head(sd, l3[None, :]) if fw is None else head32(fw, l3[None, :])
        for k, v in (("l1", l1), ("l2", l2), ("l3", l3), ("out", out)):
            keep[k].append(v)
    return {k: torch.stack(v) for k, v in keep.items()}
