"""Cases and CPU restatements of the discrete position + rotation model's TRAINING side (TEST INFRASTRUCTURE; no product file imports
this).

* ``q_sample2``: the two noisings of spatial_diffusion_discrete_rot.py:177-183 in the closed form of ``discrete_train_cases.q_sample``
  (K classes, then 4), fp64.
* ``loss_rows`` / ``losses``: p_losses :208-273 for both heads.  The formulas are ``discrete_train_cases.loss_rows``; what differs is
  the label smoothing -- "cross_entropy" smooths neither head, "hybrid" smooths the position head's cross entropy (1e-2) and not the
  rotation head's -- so the cross-entropy rows are restated here.  Plain torch in the dtype of the logits, differentiable.
* the configuration of golden_v10.npz (make_golden_v10.py), its loader, the row mixes of the kernel tests, the denoiser cases.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import discrete_cases as DC
import discrete_rot_cases as RC
import discrete_train_cases as DT

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS, LAMBDA = DT.KINDS, DT.LAMBDA

# golden_v10.npz: v9's weights and graph (K = 36, steps = 100, two complete 36-piece puzzles), feature image 0; x_start a permutation per
# puzzle, rot_start seeded in {0..3}; t per graph.  One hybrid case with classifier_free_prob = 0.5 and the recorded [G] draw (exactly
# one puzzle masked), one hybrid case under only_rotation.
V10 = dict(K=36, steps=100, sizes=RC.V9["sizes"], seed=1010, lambda_loss=LAMBDA)
V10_CASES = tuple(dict(name=f"{kind}_t{a}_{b}", kind=kind, t=(a, b), cfg_prob=0.0, only_rot=False) for kind in KINDS for a, b in ((0, 50), (1, 99))) + \
    (dict(name="hybrid_t95_5_cfg", kind="hybrid", t=(95, 5), cfg_prob=0.5, only_rot=False),
     dict(name="hybrid_t40_70_onlyrot", kind="hybrid", t=(40, 70), cfg_prob=0.0, only_rot=True))


def load_golden10():
    return dict(np.load(os.path.join(HERE, "golden_v10.npz")))


def v10_inputs(spec):
    """x_start (a permutation per puzzle), rot_start in {0..3} and the per-node timesteps of one fixture case, from seeds."""
    sizes = V10["sizes"]
    rng = np.random.default_rng(V10["seed"] + sum(spec["t"]) + 7 * KINDS.index(spec["kind"]) + (1000 if spec["only_rot"] else 0))
    x_start = torch.from_numpy(np.concatenate([rng.permutation(V10["K"])[:n] for n in sizes])).long()
    rot_start = torch.from_numpy(rng.integers(0, 4, sum(sizes))).long()
    t = torch.cat([torch.full((n,), ti, dtype=torch.long) for n, ti in zip(sizes, spec["t"])])
    return x_start, rot_start, t


# ------------------------------------------------------------------------------------------------ restatements
def q_sample2(alphas_cumprod, x_start, rot_start, t, u_x, u_rot, K):
    """fp64 -> (x_t [N], gap_x [N], rot_t [N], gap_rot [N]); ``u_x`` None skips the position half (only_rotation)."""
    x_t, gap_x = DT.q_sample(alphas_cumprod, x_start, t, u_x, K) if u_x is not None else (None, None)
    rot_t, gap_rot = DT.q_sample(alphas_cumprod, rot_start, t, u_rot, 4)
    return x_t, gap_x, rot_t, gap_rot


def loss_rows(alphas_cumprod, logits, x_start, x_t, t, smooth):
    """(vb_row [N], ce_row [N]) of one head with ``logits.shape[1]`` classes and label smoothing ``smooth`` of the cross entropy."""
    vb, _ = DT.loss_rows(alphas_cumprod, logits, x_start, x_t, t)
    K = logits.shape[1]
    y = (1.0 - smooth) * F.one_hot(x_start, K).to(logits.dtype) + smooth / K
    return vb, -(y * F.log_softmax(logits, -1)).sum(-1)


def smoothing(kind):
    """(position head, rotation head) label smoothing of the cross entropy for a loss kind (:209-210, :242-243)."""
    return (0.01, 0.0) if kind == "hybrid" else (0.0, 0.0)


def head_loss(vb, ce, kind, lambda_loss=LAMBDA):
    return {"vb": vb.mean(), "cross_entropy": ce.mean(), "hybrid": lambda_loss * ce.mean() + vb.mean()}[kind]


def losses(alphas_cumprod, logits, rot_logits, x_start, x_t, rot_start, rot_t, t, kind, lambda_loss=LAMBDA):
    """(x_loss, rot_loss); ``logits`` None -> x_loss None (only_rotation)."""
    sx, sr = smoothing(kind)
    x_loss = None if logits is None else head_loss(*loss_rows(alphas_cumprod, logits, x_start, x_t, t, sx), kind, lambda_loss)
    return x_loss, head_loss(*loss_rows(alphas_cumprod, rot_logits, rot_start, rot_t, t, sr), kind, lambda_loss)


# ------------------------------------------------------------------------------------------------ kernel-test rows
Q_KS, Q_NS = (2, 35, 65, 1024), (1, 63, 130)
Q_STEPS = DT.Q_STEPS
# seeds for which at most GAP_CAP of the rows have a top-2 gap below GAP in fp64, in BOTH noisings (asserted by
# tests/test_discrete_rot_train_host.py)
Q_SEEDS = {(K, n): 2000 + 19 * i + j for i, K in enumerate(Q_KS) for j, n in enumerate(Q_NS)}


def q_sample_case(n, K, steps, seed):
    """(x_start, rot_start, t, u_x, u_rot) of one noising case: ``discrete_train_cases.q_sample_case`` plus the rotation half."""
    x0, t, u = DT.q_sample_case(n, K, steps, seed)
    rng = np.random.default_rng(seed + 500)
    r0 = torch.from_numpy(rng.integers(0, 4, n)).long()
    ur = torch.from_numpy(rng.uniform(1e-6, 1.0, (n, 4)).astype(np.float32))
    return x0, r0, t, u, ur


def row_mix(n, K, steps, seed, scale=3.0):
    """``discrete_train_cases.row_mix`` for both heads, sharing t: (logits, x0, xt, rot_logits, r0, rt, t)."""
    logits, x0, xt, t = DT.row_mix(n, K, steps, seed, scale)
    rl, r0, rt, t4 = DT.row_mix(n, 4, steps, seed + 900, scale)
    assert torch.equal(t, t4)
    return logits, x0, xt, rl, r0, rt, t


# ------------------------------------------------------------------------------------------------ denoiser cases
DENOISER_CASES = ("dense36x2", "expander64_d6")
_DENOISER = {}


def denoiser_case(key):
    """Inputs + fp64 forward / autograd through discrete_rot_cases.forward_with_feats with a random functional over BOTH outputs:
    computed once, shared, never modified.  dense36x2: golden_v9's weights, two complete 36-piece puzzles (K = 36), feature image 0;
    expander64_d6: one 64-node Exphander graph of degree 6 (K = 64), which trains on the edge-list (CSR) kernels."""
    if key in _DENOISER:
        return _DENOISER[key]
    from oracle import weights as W
    if key == "dense36x2":
        c = RC.v9_case()
        sd, ei, batch, feats, K, steps, seed = c["sd"], c["edge_index"], c["batch"], c["feats4"][0], RC.V9["K"], RC.V9["steps"], 93
    elif key == "expander64_d6":
        K, steps, seed = 64, 50, 94
        sd = RC.make_rot_state(K, steps, seed)
        ei, batch = W.collate([W.random_regular_edge_index(64, 6, np.random.default_rng(seed))], [64])
        feats = W.randn((64, 1088), seed + 1)
    else:
        raise KeyError(key)
    N = feats.shape[0]
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(0, K, N)).long()
    t = torch.from_numpy(rng.integers(0, steps, size=int(batch.max()) + 1))[batch]
    fx = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    fr = torch.from_numpy(rng.standard_normal((N, 4)).astype(np.float32))
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    fg = feats.double().clone().requires_grad_(True)
    logits, rot_logits = RC.forward_with_feats(sdg, idx, t, ei, fg)
    ((logits * fx.double()).sum() + (rot_logits * fr.double()).sum()).backward()
    _DENOISER[key] = dict(sd=sd, K=K, steps=steps, edge_index=ei, batch=batch, feats=feats, idx=idx, t=t, fx=fx, fr=fr,
                          logits=logits.detach(), rot_logits=rot_logits.detach(), grads={k: v.grad for k, v in sdg.items()},
                          d_feats=fg.grad)
    return _DENOISER[key]
