"""Cases and CPU restatements of the discrete position diffusion (TEST INFRASTRUCTURE; no product file imports this).

* ``make_discrete_state``: seeded weights with ``Eff_GAT_Discrete``'s key layout for any K: ``oracle.weights.make_denoiser_state``
  with ``pos_mlp.weight [K, 32]`` swapped in for the pose MLP and a K-wide ``final_mlp.2``.
* ``forward_with_feats``: efficient_gat_discrete.py:72-97 composed from ``oracle.denoiser``'s pieces, in the dtype of the state.
* ``posterior_logits`` / ``reverse_step``: spatial_diffusion_discrete.py:193-227, 282-320 in the CLOSED FORM of the uniform
  transition (overline_Q[t] = a_t I + (1 - a_t) / K 11^T, overline_Q[t] overline_Q[p]^-1 = r I + (1 - r) / K 11^T, r = a_t / a_p),
  evaluated in fp64 from the fp32 ``alphas_cumprod`` buffer.
* the configuration of golden_v7.npz (make_golden_v7.py) and its loader.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import denoiser as OD
from oracle import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))

# golden_v7.npz: K = 36 (6 x 6), steps = 100, LINEAR schedule, inference_ratio 5, two puzzles of 36 pieces, complete graphs with
# self loops, random patch_feats [72, 1088]
V7 = dict(K=36, steps=100, ratio=5, sizes=(36, 36), seed=707, feat_seed=708, cfg_w=0.5, fwd_t=(95, 50, 0), post_t=(95, 50, 5),
          guided_t=(95, 50, 5))
GAP = 1e-3            # argmax comparisons leave out nodes whose top-2 gap of post + g is below this ...
GAP_CAP = 0.01        # ... and those may be at most this share of a case's nodes


def make_discrete_state(K, steps, seed=0, qk_gain=1.0):
    sd = W.make_denoiser_state(steps, 2, K, seed=seed, qk_gain=qk_gain)
    for k in [k for k in sd if k.startswith("pos_mlp.")]:
        del sd[k]
    rng = np.random.default_rng(seed + 77)
    sd["pos_mlp.weight"] = torch.from_numpy(rng.standard_normal((K, 32)).astype(np.float32))
    return sd


def v7_case():
    c = V7
    sd = make_discrete_state(c["K"], c["steps"], c["seed"])
    ei, batch = W.collate([W.dense_edge_index(n, True) for n in c["sizes"]], c["sizes"])
    feats = W.randn((sum(c["sizes"]), 1088), c["feat_seed"])
    return dict(sd=sd, edge_index=ei, batch=batch, feats=feats)


def load_golden7():
    return dict(np.load(os.path.join(HERE, "golden_v7.npz")))


def forward_with_feats(sd, idx, t, edge_index, feats, dtype=torch.float64):
    """logits [N, K] of Eff_GAT_Discrete.forward_with_feats, computed in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    comb = torch.cat([feats.to(dtype), sd["pos_mlp.weight"][idx], sd["time_emb.weight"][t]], -1)
    h = F.gelu(F.linear(comb, sd["mlp.0.weight"], sd["mlp.0.bias"]))
    combined = F.linear(h, sd["mlp.2.weight"], sd["mlp.2.bias"])
    z, _ = OD.transformer_gnn(sd, combined, edge_index)
    hh = F.gelu(F.linear(z + combined, sd["final_mlp.0.weight"], sd["final_mlp.0.bias"]))
    return F.linear(hh, sd["final_mlp.2.weight"], sd["final_mlp.2.bias"])


def linear_alphas_cumprod(steps):
    """The module's fp32 buffer for the LINEAR schedule (spatial_diffusion.py:282-290)."""
    return torch.cumprod(1.0 - torch.linspace(0.0001, 0.02, steps), 0)


def posterior_logits(alphas_cumprod, x_t, logits, t, prev_t, eps=1e-8):
    """q_posterior_logits in closed form, fp64; rows with t == 0 return the logits."""
    K = logits.shape[1]
    ac = alphas_cumprod.double()
    a_t, a_p = ac[t], ac[prev_t.clamp(min=0)]
    r = (a_t / a_p)[:, None]
    f1 = F.one_hot(x_t, K).double() * r + (1.0 - r) / K
    f2 = a_p[:, None] * F.softmax(logits.double(), -1) + ((1.0 - a_p) / K)[:, None]
    out = torch.log(f1 + eps) + torch.log(f2 + eps)
    return torch.where(t[:, None] == 0, logits.double(), out)


def reverse_step(alphas_cumprod, x_t, logits, t, ratio, u):
    """p_sample_ddpm after the model call, fp64: -> (x_prev [N], post [N, K], top-2 gap of post + g [N])."""
    post = posterior_logits(alphas_cumprod, x_t, logits, t, t - ratio)
    u = torch.clip(u.double(), torch.finfo(torch.float32).tiny, 1.0)
    val = post + (t != 0)[:, None] * -torch.log(-torch.log(u))
    top = torch.topk(val, 2, dim=-1).values
    return torch.argmax(val, -1), post, top[:, 0] - top[:, 1]


def check_argmax(x_prev, ref_prev, gap, what=""):
    """x_prev equals ref_prev wherever the restatement's top-2 gap is >= GAP; at most GAP_CAP of the nodes lie below it."""
    x_prev, ref_prev, gap = torch.as_tensor(x_prev).cpu().long(), torch.as_tensor(ref_prev).cpu().long(), torch.as_tensor(gap).cpu()
    clear = gap >= GAP
    assert float((~clear).double().mean()) <= GAP_CAP, (what, int((~clear).sum()), clear.numel())
    bad = (x_prev != ref_prev) & clear
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
