"""Cases and CPU restatements of the discrete position + rotation diffusion (TEST INFRASTRUCTURE; no product file imports this).

* ``make_rot_state``: ``discrete_cases.make_discrete_state`` plus the four ``final_mlp_rot`` tensors of ``Eff_GAT_Discrete_ROT``.
* ``feature_images``: the four feature images of a Batch, [4, N, 1088] (image r stands for the encoder's output on the crops rotated
  by -r quarter turns; seeded noise here, since the encoder is outside the path).
* ``forward_with_feats``: efficient_gat_discrete_rotation.py:87-115 with the ``(x, attentions)`` pair unpacked, both heads, in the
  dtype of the state; ``rot_step``: spatial_diffusion_discrete_rot.py:288-330 in the closed form of ``discrete_cases``, fp64.
* the configuration of golden_v9.npz (make_golden_v9.py) and its loader.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import discrete_cases as DC
from oracle import denoiser as OD
from oracle import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GAP, GAP_CAP = DC.GAP, DC.GAP_CAP

# golden_v9.npz: the V7 shapes (K = 36, steps = 100, LINEAR schedule, ratio 5, two complete 36-piece puzzles) with four feature images.
# Near ties measured by make_golden_v9.py at this seed, of 1440 per trajectory: position 3 - 5, rot_0 1 - 2, rot_prev 0 (stored in the
# fixture; GAP_CAP allows 14).  A piece's raw rotation logits move little along a trajectory, so a near tie of rot_0 tends to repeat.
V9 = dict(DC.V7, seed=949, feat_seed=910, modes=((False, False), (True, False), (True, True)))
ROT_GAIN = 16.0
MODE_NAME = {(False, False): "plain", (True, False): "cold", (True, True): "cold_onlyrot"}


def make_rot_state(K, steps, seed=0, rot_gain=ROT_GAIN):
    """``rot_gain`` multiplies ``final_mlp_rot.2.weight``: at torch's default scale the four rotation logits are decided by the
    bias, every piece's rot_0 is the same rotation at every step, and a loop without cold diffusion never leaves feature image 0."""
    sd = DC.make_discrete_state(K, steps, seed)
    rng = np.random.default_rng(seed + 177)
    W._linear(rng, sd, "final_mlp_rot.0", 1152, 32)
    W._linear(rng, sd, "final_mlp_rot.2", 32, 4)
    sd["final_mlp_rot.2.weight"] *= rot_gain
    return sd


def feature_images(n, seed):
    return torch.stack([W.randn((n, 1088), seed + 10 * r) for r in range(4)])


def v9_case():
    c = V9
    sd = make_rot_state(c["K"], c["steps"], c["seed"])
    ei, batch = W.collate([W.dense_edge_index(n, True) for n in c["sizes"]], c["sizes"])
    return dict(sd=sd, edge_index=ei, batch=batch, feats4=feature_images(sum(c["sizes"]), c["feat_seed"]))


def load_golden9():
    return dict(np.load(os.path.join(HERE, "golden_v9.npz")))


def select_feats(feats4, rot_acc):
    """Row rot_acc[piece] of the four images: [N, 1088]."""
    return feats4[rot_acc.long() % 4, torch.arange(feats4.shape[1])]


def forward_with_feats(sd, idx, t, edge_index, feats, dtype=torch.float64):
    """(logits [N, K], rot_logits [N, 4]) of Eff_GAT_Discrete_ROT.forward_with_feats over ``feats`` [N, 1088], computed in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    comb = torch.cat([feats.to(dtype), sd["pos_mlp.weight"][idx], sd["time_emb.weight"][t]], -1)
    h = F.gelu(F.linear(comb, sd["mlp.0.weight"], sd["mlp.0.bias"]))
    combined = F.linear(h, sd["mlp.2.weight"], sd["mlp.2.bias"])
    z, _ = OD.transformer_gnn(sd, combined, edge_index)
    res = z + combined
    out = []
    for head in ("final_mlp", "final_mlp_rot"):
        hh = F.gelu(F.linear(res, sd[head + ".0.weight"], sd[head + ".0.bias"]))
        out.append(F.linear(hh, sd[head + ".2.weight"], sd[head + ".2.bias"]))
    return tuple(out)


def rot_step(alphas_cumprod, x_t, rot_t, logits, rot_logits, t, ratio, u_x, u_rot):
    """p_sample_ddpm after the model call, fp64 -> dict(x_prev, rot_0, rot_prev, post_x, post_rot, gap_x, gap_rot0, gap_rot)."""
    x_prev, post_x, gap_x = DC.reverse_step(alphas_cumprod, x_t, logits, t, ratio, u_x)
    rot_prev, post_rot, gap_rot = DC.reverse_step(alphas_cumprod, rot_t, rot_logits, t, ratio, u_rot)
    top = torch.topk(rot_logits.double(), 2, dim=-1).values
    return dict(x_prev=x_prev, rot_0=torch.argmax(rot_logits.double(), -1), rot_prev=rot_prev, post_x=post_x, post_rot=post_rot,
                gap_x=gap_x, gap_rot0=top[:, 0] - top[:, 1], gap_rot=gap_rot)
