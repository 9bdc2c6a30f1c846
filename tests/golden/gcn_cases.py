"""GCN backbone (backbones/gcn.py:5-22) test support: a restatement of PyG's ``GCNConv`` with default settings, the GCN
cases of golden_v5.npz (make_golden_v5.py) and a restatement-based oracle of the whole denoiser forward.

``GCNConv`` is PyG's, unpinned and not installed (as TransformerConv); restated from PyG's published algorithm
for the 2.1 - 2.3 releases that pytorch==1.12.1 implies (gcn_norm + MessagePassing with aggr='add'):
  * add_remaining_self_loops: every existing self loop is dropped, exactly one self loop of weight 1 is added per node
    (appended behind the edges); duplicate non-loop edges are kept and each counts once;
  * deg[i] = number of incoming edges of i counted at the TARGET (edge_index[1]), self loop included;
  * norm_ji = deg[j]^-1/2 deg[i]^-1/2 (inf -> 0);
  * out_i = sum_{j -> i} norm_ji (x W^T)_j + b  (``lin`` has no bias; ``bias`` is added after the aggregation).
Weights and inputs are regenerated from seeds (oracle/weights.py), so the fixture stores outputs only.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
from oracle import weights as W  # noqa: E402

GOLDEN5_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v5.npz")


# ----------------------------------------------------------------------------- restatement
def gcn_norm(edge_index, n_nodes, dtype=torch.float32):
    """-> (src, dst, norm) of the edges GCNConv aggregates over: non-loop edges in the caller's order, then one self loop
    per node; norm in ``dtype`` (PyG: the features' dtype)."""
    src, dst = edge_index[0], edge_index[1]
    keep = src != dst
    loop = torch.arange(n_nodes, dtype=src.dtype, device=src.device)
    src = torch.cat([src[keep], loop])
    dst = torch.cat([dst[keep], loop])
    deg = torch.zeros(n_nodes, dtype=dtype, device=src.device).scatter_add_(0, dst, torch.ones_like(dst, dtype=dtype))
    dinv = deg.pow(-0.5)
    dinv.masked_fill_(dinv == float("inf"), 0.0)
    return src, dst, dinv[src] * dinv[dst]


def gcn_conv(x, edge_index, weight, bias):
    """PyG GCNConv(in, out)(x, edge_index) with default settings: x [n, in], weight [out, in], bias [out]."""
    h = x @ weight.t()
    src, dst, norm = gcn_norm(edge_index, x.shape[0], h.dtype)
    out = torch.zeros((x.shape[0], h.shape[1]), dtype=h.dtype, device=h.device)
    out.index_add_(0, dst, norm[:, None] * h[src])
    return out + bias


def dense_gcn_matrix(edge_index, n_nodes):
    """Independent check: D^-1/2 (A + I) D^-1/2 built from scratch as a dense float64 matrix, A[i, j] = number of edges
    j -> i with i != j (multi-edges counted), D = row sums of A + I (the target-side degrees)."""
    A = np.zeros((n_nodes, n_nodes), dtype=np.float64)
    for j, i in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        if i != j:
            A[i, j] += 1.0
    A += np.eye(n_nodes)
    d = A.sum(1)
    dinv = np.where(d > 0, d ** -0.5, 0.0)
    return torch.from_numpy(dinv[:, None] * A * dinv[None, :])


class GCNConv(nn.Module):
    """Stand-in for ``torch_geometric.nn.GCNConv`` (PyG's parameter names: ``lin.weight``, ``bias``) that the generator
    binds under the reference's import of torch_geometric."""

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        assert not kwargs, kwargs
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, x, edge_index):
        return gcn_conv(x, edge_index, self.lin.weight, self.bias)


# ----------------------------------------------------------------------------- cases
# graph: "dense" (self loops), "dense_noloop", "regular<d>" (Exphander, permutations kept), "dropout<pct>" (the dataset's
# random-dropout edge list, puzzle_dataset.py:615-628: directed, some self loops kept)
GCN_FWD2D = [
    dict(name="gcn_k36_noloop", sizes=[36], c=2, graph="dense_noloop", steps=50, seed=101),
    dict(name="gcn_rot144_g2", sizes=[144, 144], c=4, graph="dense", steps=100, seed=102),
    dict(name="gcn_expander_d6", sizes=[64, 64], c=4, graph="regular6", steps=300, seed=103),
    dict(name="gcn_expander_d7", sizes=[64, 64], c=4, graph="regular7", steps=300, seed=104),
    dict(name="gcn_dropout", sizes=[36, 64], c=4, graph="dropout30", steps=100, seed=105),
    dict(name="gcn_ragged", sizes=[36, 64, 100], c=4, graph="dense", steps=100, seed=106),
]
GCN_FWD3D = [
    dict(name="gcn3d_p20", sizes=[20, 7, 13], steps=300, seed=107),
]
GCN_LOOPS2D = [
    dict(name="gcn_ddim_t50_eps", base="gcn_k36_noloop", T=50, ratio=1, mean="EPSILON"),
    dict(name="gcn_ddim_t300_x0", base="gcn_expander_d6", T=300, ratio=10, mean="START_X"),
]
# p_losses + every live gradient (the reference's GNN_Diffusion.p_losses, spatial_diffusion.py:432-483, loss "huber"): a 12 x 12
# G = 2 Batch of complete graphs (closed-form aggregation) and the random-dropout Batch (CSR gather, transposed backward)
GCN_TRAIN2D = [
    dict(name="gcn_train_rot144_g2", base="gcn_rot144_g2", mean="EPSILON", seed=111),
    dict(name="gcn_train_dropout", base="gcn_dropout", mean="START_X", seed=112),
]
GCN_LOOPS3D = [
    dict(name="gcn_ddim3d_t300", base="gcn3d_p20", T=300, ratio=10, mean="START_X", max_iters=10),
]


def by_name(name):
    for s in GCN_FWD2D + GCN_FWD3D:
        if s["name"] == name:
            return s
    raise KeyError(name)


def make_gcn_state(steps, c_in, c_out, D, hidden, variant, seed):
    """The reference's Eff_GAT / Eff_GAT_3d key layout with the GCN backbone: the non-GNN parameters of
    oracle/weights.make_denoiser_state, GCNConv weights U(-1/sqrt(fan_in), 1/sqrt(fan_in)) and a non-zero bias (PyG's
    zero init would leave the bias path untested)."""
    sd = W.make_denoiser_state(steps, c_in, c_out, D=D, hidden=hidden, variant=variant, arch="transformer", n_layers=2, seed=seed)
    sd = {k: v for k, v in sd.items() if not k.startswith("gnn_backbone.")}
    rng = np.random.default_rng(seed + 5000)
    for l, (fi, fo) in enumerate(((D, 256), (256, D))):
        b = 1.0 / math.sqrt(fi)
        sd[f"gnn_backbone.module_list.{l}.lin.weight"] = torch.from_numpy(rng.uniform(-b, b, (fo, fi)).astype(np.float32))
        sd[f"gnn_backbone.module_list.{l}.bias"] = torch.from_numpy(rng.uniform(-b, b, (fo,)).astype(np.float32))
    return sd


def regular_from_perm(nodes, degree):
    """generate_random_regular_graph (puzzle_dataset.py:115-152) for a given permutation ``nodes`` (oracle/weights.py's
    restatement with the permutation drawn outside): int64 [2, n * degree]."""
    n = nodes.size
    reps = degree // 2
    ns = np.hstack([np.roll(nodes, i + 1) for i in range(reps)]) if reps else np.zeros(0, np.int64)
    ei = np.vstack((np.tile(nodes, reps), ns))
    if degree % 2 == 1:
        ei = np.hstack((ei, np.vstack((nodes[: n // 2], nodes[n // 2:]))))
    return torch.from_numpy(np.stack([np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])]).astype(np.int64))


def _graph(kind, n, rng):
    if kind == "dense":
        return W.dense_edge_index(n, True), None
    if kind == "dense_noloop":
        return W.dense_edge_index(n, False), None
    if kind.startswith("regular"):
        perm = rng.permutation(np.arange(n))
        return regular_from_perm(perm, int(kind[len("regular"):])), perm
    if kind.startswith("dropout"):
        ei = W.dense_edge_index(n, True)
        degree = round(int(kind[len("dropout"):]) * (n - 1) / 100)
        keep = torch.from_numpy(rng.permutation(ei.shape[1]))[: n * degree]
        return ei[:, keep], None
    raise ValueError(kind)


def build_case(spec, variant="2d"):
    """-> dict(sd, x, t, feats, edge_index, batch, perms) regenerated from the spec's seeds; perms [G, n] int64 for
    Exphander cases (else None)."""
    sizes = spec["sizes"]
    N = sum(sizes)
    rng = np.random.default_rng(spec["seed"] + 77)
    if variant == "2d":
        sd = make_gcn_state(spec["steps"], spec["c"], spec["c"], 1152, 128, "2d", spec["seed"])
        x, feats = W.make_inputs(N, spec["c"], 1088, spec["seed"])
        graphs = [_graph(spec["graph"], n, rng) for n in sizes]
    else:
        sd = make_gcn_state(spec["steps"], 7, None, 832, 256, "3d", spec["seed"])
        x, feats = W.make_inputs(N, 7, 768, spec["seed"])
        x[:, :4] = torch.nn.functional.normalize(x[:, :4], dim=-1)
        graphs = [(W.dense_edge_index(n, True), None) for n in sizes]
    edge_index, batch = W.collate([g[0] for g in graphs], sizes)
    perms = None
    if graphs[0][1] is not None:
        perms = torch.from_numpy(np.stack([g[1] for g in graphs]).astype(np.int64))
    tg = torch.from_numpy(rng.integers(0, spec["steps"], size=len(sizes)))
    return dict(sd=sd, x=x, t=tg[batch], feats=feats, edge_index=edge_index, batch=batch, perms=perms)


def load_golden5():
    return np.load(GOLDEN5_FILE)


# ----------------------------------------------------------------------------- oracle
def _gelu(x):
    return torch.nn.functional.gelu(x)


def forward_with_feats(sd, x, t, edge_index, feats, variant="2d", acts=None):
    """Eff_GAT(.._3d).forward_with_feats with the GCN backbone from the restatement alone (efficient_gat.py:121-146,
    efficient_gat_3d.py:173-220, gcn.py:16-22): 2D -> [N, c_out]; 3D -> [N, 7] (unit quaternion wxyz | translation).
    ``acts``: optional list that receives mlp's output and the two GCNConv outputs (before their GELU)."""
    L = torch.nn.functional.linear
    tf = sd["time_emb.weight"][t]
    pf = L(_gelu(L(x, sd["pos_mlp.0.weight"], sd["pos_mlp.0.bias"])), sd["pos_mlp.2.weight"], sd["pos_mlp.2.bias"])
    comb = torch.cat([feats, pf, tf], -1)
    if variant == "2d":
        comb = L(_gelu(L(comb, sd["mlp.0.weight"], sd["mlp.0.bias"])), sd["mlp.2.weight"], sd["mlp.2.bias"])
    else:
        lr = lambda v: torch.nn.functional.leaky_relu(v, 0.2)  # noqa: E731
        comb = lr(L(lr(L(comb, sd["mlp.0.weight"], sd["mlp.0.bias"])), sd["mlp.2.weight"], sd["mlp.2.bias"]))
    h = comb
    if acts is not None:
        acts.append(comb)
    for l in range(2):
        p = f"gnn_backbone.module_list.{l}."
        h = gcn_conv(h, edge_index, sd[p + "lin.weight"], sd[p + "bias"])
        if acts is not None:
            acts.append(h)
        h = _gelu(h)
    z = h + comb
    if variant == "2d":
        return L(_gelu(L(z, sd["final_mlp.0.weight"], sd["final_mlp.0.bias"])), sd["final_mlp.2.weight"], sd["final_mlp.2.bias"])
    tp = L(_gelu(L(z, sd["mlp_t.0.weight"], sd["mlp_t.0.bias"])), sd["mlp_t.2.weight"], sd["mlp_t.2.bias"])
    rp = L(_gelu(L(z, sd["mlp_r.0.weight"], sd["mlp_r.0.bias"])), sd["mlp_r.2.weight"], sd["mlp_r.2.bias"])
    from oracle import so3
    from oracle.pyg_restatement import matrix_to_quaternion
    return torch.hstack([torch.nn.functional.normalize(matrix_to_quaternion(so3.skew_to_rmat(rp)), p=2, dim=-1), tp])
