"""Cases of the 3D model with ``use_6dof=True`` (golden_v11.npz, make_golden_v11.py): the reference's own ``p_losses`` +
backward with the 13-channel model (spatial_diffusion_3d_test_double_diffusion.py:410-572, nine Gaussian channels, the
Gram-Schmidt rotation in the loss) for the transformer, exophormer and gcn backbones, and for the transformer a 10-step DDIM
``p_sample_loop`` with the evaluation's pose read-out and metrics.  The shapes are train3d_cases.py's; the state dicts are its
7-channel ones with the two tensors the mode widens -- ``pos_mlp.0.weight`` [16, 13] and ``mlp_t.2`` [9, 256] / [9] -- drawn
from the seeds here.  The fixture stores results only."""
import os

import numpy as np
import torch

import train3d_cases as T3

GOLDEN11_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v11.npz")
STEPS, MAX_PARTS, N_POINTS, SIZES, FEAT, VIRT, W_MIN = T3.STEPS, T3.MAX_PARTS, T3.N_POINTS, T3.SIZES, T3.FEAT, T3.VIRT, T3.W_MIN
C_IN, T_CH = 13, 9
A_MIN = 1e-6                     # |a1| and |a2 - (a2.b1) b1| of every stored row: the 1e-12 clamp of the normalisations is inactive
LOOP_RATIO, LOOP_ITERS = 30, 10  # the stored DDIM trajectory: inference_ratio = 30 over 300 steps, noise_weight = 0, START_X
TRAIN3D_6DOF = [
    dict(name="train3d_6dof_transformer", arch="transformer", seed=1101),
    dict(name="train3d_6dof_exophormer", arch="exophormer", seed=1102),
    dict(name="train3d_6dof_gcn", arch="gcn", seed=1103),
]
LOOP_CASE = "train3d_6dof_transformer"


def _uniform(rng, fan_in, *shape):
    k = 1.0 / np.sqrt(fan_in)
    return torch.from_numpy(rng.uniform(-k, k, size=shape).astype(np.float32))


def make_state(arch, steps, seed, n_layers=4):
    """The reference's Eff_GAT_3d(input_channels=13, t_channels=9) key layout (live denoiser parameters)."""
    sd = dict(T3.make_state(arch, steps, seed, n_layers))
    rng = np.random.default_rng(seed + 913)
    sd["pos_mlp.0.weight"] = _uniform(rng, C_IN, 16, C_IN)
    sd["mlp_t.2.weight"] = _uniform(rng, 256, T_CH, 256)
    sd["mlp_t.2.bias"] = _uniform(rng, 256, T_CH)
    return sd


def build_case(spec, steps=STEPS):
    """train3d_cases.build_case with the 13-channel state dict: x_start stays [P, 7]."""
    case = T3.build_case(spec, steps=steps)
    case["sd"] = make_state(spec["arch"], steps, spec["seed"])
    return case


def ptr_of(sizes=SIZES):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)


def load_golden11():
    return np.load(GOLDEN11_FILE)
