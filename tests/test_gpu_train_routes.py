"""The routes of ONE training step of the denoiser (csrc/da_train.hip: train_forward_impl / train_backward_impl), each selected at the
smallest shape that selects it: q16 and the pair matrices of complete graphs, the edge list, the exophormer's flash-style and
pair-matrix hybrid kernels, the 3D heads, the GCN, the discrete lookup and the two heads of the discrete rot model.

The parity suites compare values route by route; what they cannot see is the workspace a route is given.  Per route:
  * `da_train_workspace_bytes_ex` equals `EXPECTED` -- pure host arithmetic over the shapes (dims_of / carve_train: q16, flash versus
    pair matrix, dense versus hybrid), so it is the same number under every compiler;
  * two accumulated forward and backward passes are finite;
  * the backward as EARLY then LATE (`force_staged`) equals the backward as ALL: every array bit for bit, except the `time_emb` rows of
    the gradient, which k_time_scatter adds with atomics in either schedule -- they get the bound of
    test_gpu_train.py::test_side_stream_weight_gradients_are_bit_identical, <= 1e-6 * max|g| + 1e-12.

`EXPECTED` was recorded from the library of commit 5c80492 (the parent of the commit that split the training path into stages), in
the same GPU visit as this test's first run, by running `run_route` over `ROUTES` against that library (tools/train_route_dump.py);
it is a statement about that commit's workspace layout, not about the code under test.  Seeded weights and inputs are built as in
test_gpu_forward_routes.py."""
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_forward_routes as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def module(kind):
    """One trainable module per model kind, with the seeded weights of test_gpu_forward_routes.state, bound to its TrainEngine (shared by
    the routes over it: a run sets the engine's precision and schedule and clears its gradient buffer)."""
    from diffassemble_amd.model import backbones as B
    sd = FR.state(kind)
    steps = sd["time_emb.weight"].shape[0]
    if kind in ("tr", "gcn"):
        m = B.Eff_GAT(steps=steps, input_channels=4, output_channels=4, visual_pretrained=False, architecture="gcn" if kind == "gcn" else "transformer")
    elif kind == "exo":
        m = B.Eff_GAT(steps=steps, input_channels=4, output_channels=4, visual_pretrained=False, architecture="exophormer", virt_nodes=8)
    elif kind == "3d":
        m = B.Eff_GAT_3d(steps=steps, backbone="vn_dgcnn", n_layers=4)
    elif kind == "discrete":
        m = B.Eff_GAT_Discrete(steps=steps, input_channels=36, output_channels=36)
    elif kind == "discrete_rot":
        m = B.Eff_GAT_Discrete_ROT(steps=steps, input_channels=36, output_channels=36)
    else:
        raise KeyError(kind)
    _, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    m = m.to(torch.device("cuda:0")).train()
    m.train_engine(torch.device("cuda:0"))
    return m


def exo_graph():
    """The ragged Exphander Batch of test_gpu_train.py's side-stream worker: a hybrid plan."""
    from diffassemble_amd import expander
    ei, batch, _ = expander.ragged_regular_batch([12, 16, 6, 10], 60, np.random.default_rng(4))
    return ei, batch


# name -> (model kind, TrainEngine.precision, graph, da_config fields and environment held during the run, only_rotation)
def R(kind, prec, graph, cfg=None, env=None, only_rot=False):
    return dict(kind=kind, prec=prec, graph=graph, cfg=cfg or {}, env=env or {}, only_rot=only_rot)


C36_25 = lambda: FR.complete([36, 25])          # noqa: E731
C161_30 = lambda: FR.complete([161, 30])        # noqa: E731  (above the small-group limit of 160: pair matrices kept, no q16)
EDGES = dict(train_attn=0)
ROUTES = {
    **{f"tr36_25_{p}": R("tr", p, C36_25) for p in ("fp32", "bf16")},                              # bf16: q16
    **{f"tr161_30_{p}": R("tr", p, C161_30) for p in ("fp32", "bf16")},
    **{f"tr36_25_edges_{p}": R("tr", p, C36_25, cfg=EDGES) for p in ("fp32", "bf16")},
    "exo_flash_bf16": R("exo", "bf16", exo_graph),                                                 # flash-style kernels, HybSide
    "exo_pairs_fp32": R("exo", "fp32", exo_graph, env=dict(DA_HYBRID="force")),                    # pair-matrix hybrid
    **{f"exo_edges_{p}": R("exo", p, exo_graph, cfg=EDGES) for p in ("fp32", "bf16")},
    **{f"3d_p20_{p}": R("3d", p, lambda: FR.complete([20, 7, 13])) for p in ("fp32", "bf16")},
    "gcn36_bf16": R("gcn", "bf16", FR.TWO36),
    **{f"discrete36_{p}": R("discrete", p, FR.TWO36) for p in ("fp32", "bf16")},
    **{f"rot36_{p}": R("discrete_rot", p, FR.TWO36) for p in ("fp32", "bf16")},
    **{f"rot36_only_rotation_{p}": R("discrete_rot", p, FR.TWO36, only_rot=True) for p in ("fp32", "bf16")},      # d_logits == NULL
}


def run_route(name, dev, staged):
    """Two accumulated forward and backward passes (the second adds into the first's gradients) -> {array name: CPU tensor}: the
    forward outputs and d_feats of both passes, the flat gradient `grad`, `ws_bytes` and `time_emb` = (offset, length) of that table's
    rows in `grad`."""
    import ctypes as C
    from diffassemble_amd import _lib
    from diffassemble_amd.graph_plan import build_plan
    r = ROUTES[name]
    old_cfg = _lib.set_config(**r["cfg"])
    old_env = {k: os.environ.get(k) for k in r["env"]}
    os.environ.update(r["env"])
    try:
        m = module(r["kind"])
        te = m.train_engine(dev)
        te.precision, te.force_staged = r["prec"], staged
        te.flat_grad.zero_()
        ei, batch = r["graph"]()
        plan = build_plan(ei.to(dev), batch.to(dev), te.virt_nodes, hybrid="off" if te.arch == "gcn" else None).with_source_csr()
        n = plan.n_real
        res = {"ws_bytes": torch.tensor(int(te.lib.da_train_workspace_bytes_ex(C.byref(te.w), C.byref(te._cg(plan)), te._mma())))}
        for k in range(2):
            t = FR.timesteps(batch, te.steps, 7 + 10 * k).to(dev)
            feats = FR.randn((n, te.F), 8 + 10 * k).to(dev)
            if te.disc:
                x = torch.randint(0, 36, (n,), generator=torch.Generator().manual_seed(9 + 10 * k)).to(dev)
            else:
                x = FR.randn((n, te.c_in), 9 + 10 * k)
                if r["kind"] == "3d":
                    x[:, :4] = torch.nn.functional.normalize(x[:, :4], dim=-1)
                x = x.to(dev)
            outs = te.forward(plan, x, t, feats)
            outs = list(outs) if isinstance(outs, tuple) else [outs]
            d_outs = [FR.randn(tuple(o.shape), 11 + 10 * k + j).to(dev) for j, o in enumerate(outs)]
            if r["only_rot"]:
                d_outs[0] = None
            d_feats = te.backward(plan, x, t, d_outs[0], want_dfeats=True, **(dict(d_out_rot=d_outs[1]) if len(outs) == 2 else {}))
            for j, o in enumerate(outs):
                res[f"out{j}_pass{k}"] = o.cpu()
            res[f"d_feats_pass{k}"] = d_feats.cpu()
        torch.cuda.synchronize()
        res["grad"] = te.flat_grad.cpu()
        base = te.flat.data_ptr()
        res["time_emb"] = torch.tensor([((v.data_ptr() - base) // 4, v.numel()) for n_, v in zip(te.names, te.views) if n_ == "time_emb.weight"][0])
        return res
    finally:
        _lib.set_config(**{k: getattr(old_cfg, k) for k in r["cfg"]})
        for k, v in old_env.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def differing(a, b):
    """Names of the arrays of two `run_route` results that differ: torch.equal on every array, with the one exception of the `time_emb`
    rows of `grad` (atomics in k_time_scatter), which get <= 1e-6 * max|g| + 1e-12."""
    bad = [k for k in sorted(set(a) | set(b)) if k != "grad" and not (k in a and k in b and torch.equal(a[k], b[k]))]
    if "grad" in a and "grad" in b and a["grad"].shape == b["grad"].shape and torch.equal(a["time_emb"], b["time_emb"]):
        ga, gb = a["grad"].clone(), b["grad"].clone()
        o, k = (int(v) for v in b["time_emb"])
        if float((ga[o:o + k].double() - gb[o:o + k].double()).abs().max()) > 1e-6 * float(gb[o:o + k].abs().max()) + 1e-12:
            bad.append("grad[time_emb]")
        ga[o:o + k] = 0
        gb[o:o + k] = 0
        if not torch.equal(ga, gb):
            bad.append("grad")
    else:
        bad.append("grad")
    return bad


EXPECTED = {
    "tr36_25_fp32": 166383872,
    "tr36_25_bf16": 166863872,               # (+ the bf16 images of the q16 mode: weights and layer inputs)
    "tr161_30_fp32": 189125376,
    "tr161_30_bf16": 189125376,              # (no q16 beyond 160 nodes: the fp32 layout with its pair matrices)
    "tr36_25_edges_fp32": 165967104,
    "tr36_25_edges_bf16": 165967104,
    "exo_flash_bf16": 221024768,             # (the edge list's size + the pair offsets and the node -> graph table; no pair matrix)
    "exo_pairs_fp32": 262969088,
    "exo_edges_fp32": 221021952,
    "exo_edges_bf16": 221021952,
    "3d_p20_fp32": 160032000,
    "3d_p20_bf16": 160364800,
    "gcn36_bf16": 164049152,
    "discrete36_fp32": 167629312,
    "discrete36_bf16": 168151552,
    "rot36_fp32": 167829504,
    "rot36_bf16": 168351744,
    "rot36_only_rotation_fp32": 167829504,
    "rot36_only_rotation_bf16": 168351744,
}


def test_every_route_is_pinned():
    assert sorted(EXPECTED) == sorted(ROUTES)


@pytest.mark.parametrize("name", list(ROUTES))
def test_train_route_workspace_finite_and_staged_equals_all(dev, name):
    whole, staged = run_route(name, dev, staged=False), run_route(name, dev, staged=True)
    print(name, int(whole["ws_bytes"]))
    assert int(whole["ws_bytes"]) == EXPECTED[name], (name, int(whole["ws_bytes"]), EXPECTED[name])
    assert all(torch.isfinite(v).all() for v in whole.values()), name
    assert float(whole["grad"].abs().max()) > 0
    assert differing(staged, whole) == [], name
