"""Cases of the 3D training step (golden_v6.npz, make_golden_v6.py): the reference's own 3D ``p_losses`` + backward
(spatial_diffusion_3d_test_double_diffusion.py:410-572) at train_3d.py's configuration -- START_X, ``vn_dgcnn``,
``loss_type="all"`` -- with the transformer, exophormer and gcn backbones.  Weights and inputs are regenerated from the
seeds here (oracle/weights.py, gcn_cases.py); the fixture stores results only."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from oracle import weights as W  # noqa: E402

import gcn_cases as GC  # noqa: E402

GOLDEN6_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v6.npz")
STEPS, MAX_PARTS, N_POINTS, SIZES, D, FEAT, HIDDEN, VIRT = 300, 6, 1000, (5, 2, 6), 832, 768, 256, 8
# the reference's rot_points_cd_loss hard-codes 1000 points (utils_3d.py), so a smaller cloud cannot run there
TRAIN3D = [
    dict(name="train3d_transformer", arch="transformer", seed=601),
    dict(name="train3d_exophormer", arch="exophormer", seed=602),
    dict(name="train3d_gcn", arch="gcn", seed=603),
]
TRAP_T = (0, 1, 2, 5, 10, 25, 50, 100, 200, 299)      # timesteps whose IGSO(3) CDF rows the fixture stores
W_MIN = 1e-3                                          # |w| of every stored quaternion: below, the w >= 0 standardisation is rounding's


def make_state(arch, steps, seed, n_layers=4):
    """The reference's Eff_GAT_3d key layout (live denoiser parameters) for one of the three backbones."""
    if arch == "gcn":
        return GC.make_gcn_state(steps, 7, None, D, HIDDEN, "3d", seed)
    return W.make_denoiser_state(steps, 7, None, D=D, hidden=HIDDEN, variant="3d", arch=arch, virt_nodes=VIRT, n_layers=n_layers,
                                 seed=seed)


def unit_quaternions(rng, n, w_min=0.05):
    """[n, 4] fp32 unit quaternions with w >= w_min (rotation angles away from pi: |angle - pi| >= 2 asin(w_min))."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1
    q[:, 0] = np.maximum(q[:, 0], w_min)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return torch.from_numpy(q.astype(np.float32))


def poses(n, seed):
    """Ground-truth poses [n, 7]: unit quaternion wxyz | translation ~ 0.5 N(0, 1)."""
    rng = np.random.default_rng(seed + 31)
    return torch.cat([unit_quaternions(rng, n), torch.from_numpy((0.5 * rng.standard_normal((n, 3))).astype(np.float32))], 1)


def valids_of(sizes, n_parts):
    v = torch.zeros(len(sizes), n_parts, dtype=torch.bool)
    for i, n in enumerate(sizes):
        v[i, :n] = True
    return v


def build_case(spec, sizes=SIZES, n_points=N_POINTS, n_parts=MAX_PARTS, steps=STEPS):
    """-> dict(sd, x_start [P, 7], t [P], feats [P, 768], pts [P, N, 3], edge_index, batch, valids [G, n_parts]) from the seeds."""
    P = sum(sizes)
    rng = np.random.default_rng(spec["seed"] + 77)
    _, feats = W.make_inputs(P, 7, FEAT, spec["seed"])
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    tg = torch.from_numpy(rng.integers(0, steps, size=len(sizes)))
    return dict(sd=make_state(spec["arch"], steps, spec["seed"]), x_start=poses(P, spec["seed"]), t=tg[batch], feats=feats,
                pts=W.make_point_clouds(P, n_points, spec["seed"]), edge_index=edge_index, batch=batch,
                valids=valids_of(sizes, n_parts))


def load_golden6():
    return np.load(GOLDEN6_FILE)
