"""CPU tests of the GCN backbone (architecture="gcn", backbones/gcn.py:5-22): the GCNConv restatement against an
independent dense D^-1/2 (A + I) D^-1/2, the restatement-based oracle against golden_v5.npz (the reference's own code,
make_golden_v5.py), and the modules' state-dict surface."""
import numpy as np
import pytest
import torch

import gcn_cases as GC


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def golden5():
    return GC.load_golden5()


def _edge_case_graph():
    # node 0: multi-edge 1 -> 0 (twice) and an existing self loop (dropped, replaced by one of weight 1)
    # node 2: directed only (2 -> 3, no 3 -> 2); node 4: isolated; node 5: two self loops; node 6 stands alone as a
    # 1-node graph of the Batch
    src = [1, 1, 0, 2, 3, 0, 5, 5, 1]
    dst = [0, 0, 0, 3, 1, 3, 5, 5, 2]
    return torch.tensor([src, dst], dtype=torch.int64), 7


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_dense_formula(seed):
    ei, n = _edge_case_graph()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 12, generator=g, dtype=torch.float64)
    w = torch.randn(5, 12, generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    out = GC.gcn_conv(x, ei, w, b)
    ref = GC.dense_gcn_matrix(ei, n) @ (x @ w.t()) + b
    assert torch.allclose(out, ref, atol=1e-12), (out - ref).abs().max()
    # the edge-case rules, stated directly
    M = GC.dense_gcn_matrix(ei, n)
    assert M[0, 1] == pytest.approx(2.0 / np.sqrt(3 * 2))        # multi-edge counted twice; deg[0] = 2 + 1, deg[1] = 1 (3 -> 1) + 1
    assert M[4, 4] == 1.0 and M[6, 6] == 1.0                      # isolated node / 1-node graph: only its self loop
    assert M[5, 5] == 1.0                                         # existing self loops dropped, one added
    assert M[2, 3] == 0.0 and M[3, 2] != 0.0                       # directed: 2 -> 3 only, degrees at the target


def test_restatement_matches_dense_formula_on_batches():
    cases = [GC.build_case(GC.by_name(nm)) for nm in ("gcn_dropout", "gcn_expander_d7", "gcn_k36_noloop")]
    for case in cases:
        ei = case["edge_index"]
        n = case["batch"].numel()
        x = torch.randn(n, 8, dtype=torch.float64)
        w = torch.eye(8, dtype=torch.float64)
        ref = GC.dense_gcn_matrix(ei, n) @ x
        assert torch.allclose(GC.gcn_conv(x, ei, w, torch.zeros(8, dtype=torch.float64)), ref, atol=1e-12)


def test_closed_forms():
    """Complete graphs with or without self loops: A_hat = J / n; Exphander of degree d without duplicates: (A + I) / (d + 1)."""
    from oracle import weights as W
    for loops in (True, False):
        M = GC.dense_gcn_matrix(W.dense_edge_index(9, loops), 9)
        assert torch.allclose(M, torch.full((9, 9), 1.0 / 9, dtype=torch.float64))
    for d in (6, 7):
        ei = GC.regular_from_perm(np.random.default_rng(d).permutation(64), d)
        M = GC.dense_gcn_matrix(ei, 64)
        A = torch.zeros(64, 64, dtype=torch.float64)
        A[ei[1], ei[0]] = 1.0
        assert torch.allclose(M, (A + torch.eye(64, dtype=torch.float64)) / (d + 1))


@pytest.mark.parametrize("spec", GC.GCN_FWD2D, ids=lambda s: s["name"])
def test_oracle_reproduces_golden_2d(spec, golden5):
    case = GC.build_case(spec)
    acts = []
    out = GC.forward_with_feats(case["sd"], case["x"], case["t"], case["edge_index"], case["feats"], "2d", acts)
    assert rel(out, golden5[f"{spec['name']}/out"]) < 1e-5
    for i, a in enumerate(acts):
        assert rel(a[:: max(1, a.shape[0] // 8), :64], golden5[f"{spec['name']}/act{i}_rows"]) < 1e-5


def test_oracle_reproduces_golden_3d(golden5):
    spec = GC.GCN_FWD3D[0]
    case = GC.build_case(spec, "3d")
    acts = []
    out = GC.forward_with_feats(case["sd"], case["x"], case["t"], case["edge_index"], case["feats"], "3d", acts)
    assert rel(out, golden5[f"{spec['name']}/out"]) < 1e-5
    for i, a in enumerate(acts):
        assert rel(a[:: max(1, a.shape[0] // 8), :64], golden5[f"{spec['name']}/act{i}_rows"]) < 1e-5


def _keys_shapes(model, skip):
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith(skip)}
    keys = sorted(sd)
    return keys, [str(tuple(sd[k].shape)) for k in keys]


def test_gnn_diffusion_2d_gcn_state_dict(golden5):
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion
    m = GNN_Diffusion(steps=50, sampling="DDIM", visual_pretrained=False, architecture="gcn")
    assert m.model.gnn_backbone.arch == "gcn"
    keys, shapes = _keys_shapes(m.model, ("visual_backbone.", "pcd_backbone."))
    assert keys == list(golden5["statedict_gcn_2d/keys"])
    assert shapes == list(golden5["statedict_gcn_2d/shapes"])
    case = GC.build_case(GC.GCN_FWD2D[0])
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected
    assert all(k.startswith(("linear1.", "linear2.", "visual_backbone.", "mean", "std")) for k in missing), missing
    assert torch.equal(m.model.gnn_backbone.module_list[1].lin.weight, case["sd"]["gnn_backbone.module_list.1.lin.weight"])


def test_gnn_diffusion_3d_gcn_state_dict(golden5):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion
    m = GNN_Diffusion(steps=300, sampling="DDIM", backbone="vn_dgcnn", architecture="gcn")
    keys, shapes = _keys_shapes(m.model, ("visual_backbone.", "pcd_backbone."))
    assert keys == list(golden5["statedict_gcn_3d/keys"])
    assert shapes == list(golden5["statedict_gcn_3d/shapes"])
    case = GC.build_case(GC.GCN_FWD3D[0], "3d")
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected
    assert all(k.startswith("pcd_backbone.") for k in missing), missing


def test_gcn_module_surface():
    from diffassemble_amd.model.backbones import GCN, Eff_GAT
    g = GCN(1152, hidden_dim=256, output_size=1152)
    assert g.arch == "gcn" and g.virt_nodes == 0
    assert not hasattr(g.module_list[0].lin, "bias") or g.module_list[0].lin.bias is None
    from diffassemble_amd.train import _param_order
    m = Eff_GAT(10, architecture="gcn", visual_pretrained=False)
    names, n_layers = _param_order(m)
    assert n_layers == 2
    live = {k for k, p in m.named_parameters() if not k.startswith(("linear1.", "linear2.", "visual_backbone."))}
    assert set(names) == live and len(names) == len(live)             # every live parameter in the flat buffer, once
    assert names.index("gnn_backbone.module_list.1.lin.weight") < names.index("final_mlp.0.weight")
    assert names[names.index("gnn_backbone.module_list.0.lin.weight") + 1] == "gnn_backbone.module_list.0.bias"
    with pytest.raises(NotImplementedError):
        Eff_GAT(10, architecture="mlp", visual_pretrained=False)


def test_expander_plan_carries_band_degree():
    from diffassemble_amd.graph_plan import expander_plan
    perms = torch.stack([torch.randperm(64), torch.randperm(64)])
    for d in (6, 7):
        p = expander_plan(perms, d, "cpu", 0, banded=True)
        assert p.hybrid and p.band_degree == d and p.slot_node is not None
        assert p.c_struct(need_csr=False).band_degree == d
    assert expander_plan(perms, 6, "cpu", 4, banded=True).band_degree == 0       # virtual rows: not the GCN's closed form
