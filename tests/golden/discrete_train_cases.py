"""Cases and CPU restatements of the discrete position model's TRAINING side (TEST INFRASTRUCTURE; no product file imports this).

* ``q_sample``: spatial_diffusion_discrete.py:181-191 in the closed form of the uniform transition (overline_Q[t] = a_t I +
  (1 - a_t) / K 11^T), fp64: -> (x_t, top-2 gap of the perturbed logits).
* ``loss_rows`` / ``loss``: p_losses :260-271 with vb_terms_bpd :416-472, q_posterior_logits :193-227 at previous_t = t - 1 and
  categorical_kl_logits :475-488 (its +1e-6 on both logit vectors cancels inside the softmaxes), plain K-wide torch in the dtype of
  the logits (fp64 for the reference values, fp32 as the precision yardstick of the GPU tests), differentiable.
* ``d_logits``: the analytic gradient of ``loss`` with respect to the logits, the formulas the kernel evaluates.
* the configuration of golden_v8.npz (make_golden_v8.py), its loader, and the row mixes of the kernel tests.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import discrete_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
LN2 = math.log(2.0)
KINDS = ("vb", "cross_entropy", "hybrid")
LAMBDA = 0.01
TINY = float(torch.finfo(torch.float32).tiny)

# golden_v8.npz: v7's weights, graph and features (K = 36, steps = 100, two complete 36-piece puzzles); x_start a permutation per puzzle;
# t per graph.  The last case has classifier_free_prob = 0.5 with the recorded [G] draw.
V8 = dict(K=36, steps=100, sizes=DC.V7["sizes"], seed=808, lambda_loss=LAMBDA)
V8_CASES = tuple(dict(name=f"{kind}_t{a}_{b}", kind=kind, t=(a, b), cfg_prob=0.0) for kind in KINDS for a, b in ((0, 50), (1, 99))) + \
    (dict(name="hybrid_t95_5_cfg", kind="hybrid", t=(95, 5), cfg_prob=0.5),)


def load_golden8():
    return dict(np.load(os.path.join(HERE, "golden_v8.npz")))


def v8_inputs(spec):
    """x_start (a permutation per puzzle) and the per-node timesteps of one fixture case, from seeds."""
    sizes = V8["sizes"]
    rng = np.random.default_rng(V8["seed"] + sum(spec["t"]) + 7 * KINDS.index(spec["kind"]))
    x_start = torch.from_numpy(np.concatenate([rng.permutation(V8["K"])[:n] for n in sizes])).long()
    t = torch.cat([torch.full((n,), ti, dtype=torch.long) for n, ti in zip(sizes, spec["t"])])
    return x_start, t


# ------------------------------------------------------------------------------------------------ restatements
def q_sample(alphas_cumprod, x_start, t, u, K):
    """fp64: x_t = argmax_k(log(a_t [k == x0] + (1 - a_t) / K + 1e-9) - log(-log(clip(u, tiny, 1)))) -> (x_t [N], top-2 gap [N])."""
    a = alphas_cumprod.double()[t][:, None]
    ql = torch.log(a * F.one_hot(x_start, K).double() + (1.0 - a) / K + 1e-9)
    val = ql - torch.log(-torch.log(torch.clip(u.double(), TINY, 1.0)))
    top = torch.topk(val, 2, dim=-1).values
    return torch.argmax(val, -1), top[:, 0] - top[:, 1]


def _scalars(alphas_cumprod, t, K, dtype):
    ac = alphas_cumprod.to(dtype)
    a_t, a_p = ac[t], ac[(t - 1).clamp(min=0)]
    return (a_t / a_p)[:, None], (((a_p - a_t) / a_p) / K)[:, None], a_p[:, None], ((1.0 - a_p) / K)[:, None]


def loss_rows(alphas_cumprod, logits, x_start, x_t, t, eps=1e-8):
    """(vb_row [N], ce_row [N]) in the dtype of ``logits``."""
    K, dt = logits.shape[1], logits.dtype
    r, c1, a_p, c2 = _scalars(alphas_cumprod, t, K, dt)
    pi, lp = F.softmax(logits, -1), F.log_softmax(logits, -1)
    e_t, e_0 = F.one_hot(x_t, K).to(dt), F.one_hot(x_start, K).to(dt)
    lf1 = torch.log(r * e_t + c1 + eps)
    m = lf1 + torch.log(a_p * pi + c2 + eps)
    qt = lf1 + torch.log(a_p * e_0 + c2 + eps)
    kl = (F.softmax(qt, -1) * (F.log_softmax(qt, -1) - F.log_softmax(m, -1))).sum(-1) / LN2
    nll = -(lp * e_0).sum(-1) / LN2
    y = 0.99 * e_0 + 0.01 / K
    return torch.where(t == 0, nll, kl), -(y * lp).sum(-1)


def loss(alphas_cumprod, logits, x_start, x_t, t, kind, lambda_loss=LAMBDA):
    vb, ce = loss_rows(alphas_cumprod, logits, x_start, x_t, t)
    return {"vb": vb.mean(), "cross_entropy": ce.mean(), "hybrid": lambda_loss * ce.mean() + vb.mean()}[kind]


def d_logits(alphas_cumprod, logits, x_start, x_t, t, kind, lambda_loss=LAMBDA, eps=1e-8):
    """d loss / d logits [N, K] by the closed formulas (no autograd), in the dtype of ``logits``."""
    N, K = logits.shape
    dt = logits.dtype
    r, c1, a_p, c2 = _scalars(alphas_cumprod, t, K, dt)
    pi = F.softmax(logits, -1)
    e_t, e_0 = F.one_hot(x_t, K).to(dt), F.one_hot(x_start, K).to(dt)
    lf1 = torch.log(r * e_t + c1 + eps)
    den = a_p * pi + c2 + eps
    g = (F.softmax(lf1 + torch.log(den), -1) - F.softmax(lf1 + torch.log(a_p * e_0 + c2 + eps), -1)) / LN2
    h = g * a_p / den
    d_vb = torch.where((t == 0)[:, None], (pi - e_0) / LN2, pi * (h - (pi * h).sum(-1, keepdim=True)))
    d_ce = pi - (0.99 * e_0 + 0.01 / K)
    w_vb, w_ce = {"vb": (1.0, 0.0), "cross_entropy": (0.0, 1.0), "hybrid": (1.0, lambda_loss)}[kind]
    return (w_vb * d_vb + w_ce * d_ce) / N


# ------------------------------------------------------------------------------------------------ kernel-test rows
def row_mix(n, K, steps, seed, scale=3.0):
    """n rows cycling through t in {0, 1, mid, steps - 1} with x_t == x0 and x_t != x0 alternating: (logits, x_start, x_t, t)."""
    rng = np.random.default_rng(seed)
    ts = (0, 1, steps // 2, steps - 1)
    t = torch.tensor([ts[i % 4] for i in range(n)], dtype=torch.long)
    x0 = torch.from_numpy(rng.integers(0, K, n))
    shift = torch.from_numpy(rng.integers(1, K, n))
    same = torch.tensor([(i // 4) % 2 == 0 for i in range(n)])
    xt = torch.where(same, x0, (x0 + shift) % K)
    logits = torch.from_numpy((scale * rng.standard_normal((n, K))).astype(np.float32))
    return logits, x0.long(), xt.long(), t


def q_sample_case(n, K, steps, seed):
    """(x_start, t, u) of one q_sample kernel case: t cycles through {0, 1, mid, steps - 1}, u uniform in (1e-6, 1)."""
    rng = np.random.default_rng(seed)
    ts = (0, 1, steps // 2, steps - 1)
    t = torch.tensor([ts[i % 4] for i in range(n)], dtype=torch.long)
    x0 = torch.from_numpy(rng.integers(0, K, n)).long()
    u = torch.from_numpy(rng.uniform(1e-6, 1.0, (n, K)).astype(np.float32))
    return x0, t, u


Q_KS, Q_NS = (2, 35, 64, 65, 144, 1024), (1, 63, 130)
Q_STEPS = 100
# seeds for which at most GAP_CAP of the rows have a top-2 gap below GAP in fp64 (asserted by tests/test_discrete_train_host.py)
Q_SEEDS = {(K, n): 1000 + 17 * i + j for i, K in enumerate(Q_KS) for j, n in enumerate(Q_NS)}


# ------------------------------------------------------------------------------------------------ denoiser cases
DENOISER_CASES = ("dense36x2", "expander64_d6")
_DENOISER = {}


def denoiser_case(key):
    """Inputs + fp64 forward / autograd through discrete_cases.forward_with_feats of one case: computed once, shared, never
    modified.  dense36x2: golden_v7's weights, two complete 36-piece puzzles (K = 36); expander64_d6: one 64-node Exphander graph
    of degree 6 (K = 64), which trains on the edge-list (CSR) kernels."""
    if key in _DENOISER:
        return _DENOISER[key]
    from oracle import weights as W
    if key == "dense36x2":
        c = DC.v7_case()
        sd, ei, batch, feats, K, steps, seed = c["sd"], c["edge_index"], c["batch"], c["feats"], DC.V7["K"], DC.V7["steps"], 91
    elif key == "expander64_d6":
        K, steps, seed = 64, 50, 92
        sd = DC.make_discrete_state(K, steps, seed)
        ei, batch = W.collate([W.random_regular_edge_index(64, 6, np.random.default_rng(seed))], [64])
        feats = W.randn((64, 1088), seed + 1)
    else:
        raise KeyError(key)
    N = feats.shape[0]
    rng = np.random.default_rng(seed)
    idx = torch.from_numpy(rng.integers(0, K, N)).long()                       # repeated indices: several pieces share a table row
    t = torch.from_numpy(rng.integers(0, steps, size=int(batch.max()) + 1))[batch]
    functional = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32))
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    fg = feats.double().clone().requires_grad_(True)
    logits = forward = DC.forward_with_feats(sdg, idx, t, ei, fg)
    (forward * functional.double()).sum().backward()
    _DENOISER[key] = dict(sd=sd, K=K, steps=steps, edge_index=ei, batch=batch, feats=feats, idx=idx, t=t, functional=functional,
                          logits=logits.detach(), grads={k: v.grad for k, v in sdg.items()}, d_feats=fg.grad)
    return _DENOISER[key]
