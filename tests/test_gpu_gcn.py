"""GPU tests of the GCN backbone (architecture="gcn", backbones/gcn.py:5-22) against golden_v5.npz -- the reference's own
efficient_gat.py / efficient_gat_3d.py / gcn.py / spatial_diffusion.py with PyG's GCNConv restated (make_golden_v5.py).
Project bounds: fp32 within 1e-4, bf16 within 8e-3 of the fixtures; trajectories within 5e-4."""
import numpy as np
import pytest
import torch

import gcn_cases as GC

pytestmark = pytest.mark.gpu

RTOL32, RTOLBF, TRAJ32 = 1e-4, 8e-3, 5e-4
DENSE = {"dense": 1, "dense_noloop": 2}


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def golden5():
    return GC.load_golden5()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    return torch.device("cuda:0")


def _engine(case, prec, dev, variant="2d"):
    from diffassemble_amd import DenoiserEngine
    return DenoiserEngine(case["sd"], variant=variant, arch="gcn", precision=prec, device=dev)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("spec", GC.GCN_FWD2D, ids=lambda s: s["name"])
def test_forward_2d(spec, prec, golden5, dev):
    case = GC.build_case(spec)
    eng = _engine(case, prec, dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    assert plan.dense == DENSE.get(spec["graph"], 0) and not plan.hybrid
    out = eng.forward(plan, case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev))
    assert rel(out, golden5[f"{spec['name']}/out"]) < (RTOL32 if prec == "fp32" else RTOLBF)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["gcn_expander_d6", "gcn_expander_d7"])
def test_expander_closed_form_plan(name, prec, golden5, dev):
    spec = GC.by_name(name)
    case = GC.build_case(spec)
    d = int(spec["graph"][len("regular"):])
    eng = _engine(case, prec, dev)
    band = eng.plan_expander(case["perms"], d)
    assert band.hybrid and band.band_degree == d and band.row_ptr is None
    x, t, f = case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev)
    out_band = eng.forward(band, x, t, f).clone()
    out_csr = eng.forward(eng.plan(case["edge_index"], case["batch"]), x, t, f)
    assert rel(out_band, golden5[f"{name}/out"]) < (RTOL32 if prec == "fp32" else RTOLBF)
    assert rel(out_band, out_csr) < (1e-5 if prec == "fp32" else RTOLBF)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_band_aggregation_n900_d539(prec, dev):
    """The closed-form Exphander aggregation at the benched degree (60 %, d = 539, n = 900) against the CSR gather of the
    same edge list and a dense (A + I) / (d + 1) in fp64."""
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    from diffassemble_amd.graph_plan import build_plan, expander_plan
    n, d, G = 900, 539, 2
    rng = np.random.default_rng(539)
    perms = torch.from_numpy(np.stack([rng.permutation(n) for _ in range(G)]).astype(np.int64))
    band = expander_plan(perms.to(dev), d, dev, 0, banded=True)
    assert band.band_degree == d
    ei = torch.cat([GC.regular_from_perm(perms[g].numpy(), d) + g * n for g in range(G)], 1)
    csr = build_plan(ei.to(dev), torch.arange(G, device=dev).repeat_interleave(n), 0, hybrid="off")
    g = torch.Generator().manual_seed(7)
    x = torch.randn(G * n, 256, generator=g)
    b = torch.randn(256, generator=g) * 0.1
    ref = []
    for k in range(G):
        e = GC.regular_from_perm(perms[k].numpy(), d)
        A = torch.eye(n, dtype=torch.float64)
        A[e[1], e[0]] += 1.0
        ref.append((A / (d + 1)) @ x[k * n:(k + 1) * n].double())
    ref = torch.nn.functional.gelu(torch.cat(ref) + b.double())
    xd, bd = x.to(dev), b.to(dev)
    out_b = E.gcn_aggregate(band, xd, bd, _lib.ACT_GELU, prec)
    out_c = E.gcn_aggregate(csr, xd, bd, _lib.ACT_GELU, prec)
    tol = RTOL32 if prec == "fp32" else RTOLBF
    assert rel(out_b.float(), ref) < tol
    assert rel(out_c.float(), ref) < tol


def _per_step_loop(eng, plan, sch, x0, feats, T, ratio, mean_type):
    eng.set_features(plan, feats)
    x, traj = x0, []
    for i in reversed(range(0, T, ratio)):
        mo = eng.forward(plan, x, i, None)
        x = eng.ddim_step(sch, x, mo, i, ratio, mean_type)
        traj.append(x)
    return torch.stack(traj)


@pytest.mark.parametrize("lp", GC.GCN_LOOPS2D, ids=lambda s: s["name"])
def test_loop_2d(lp, golden5, dev):
    from diffassemble_amd import Schedule, _lib
    from oracle import diffusion as ODF
    spec = GC.by_name(lp["base"])
    case = GC.build_case(spec)
    eng = _engine(case, "fp32", dev)
    plan = eng.plan_expander(case["perms"], int(spec["graph"][7:])) if case["perms"] is not None else eng.plan(case["edge_index"], case["batch"])
    sch = Schedule(ODF.make_schedule(lp["T"]), dev)
    mt = getattr(_lib, f"MEAN_{lp['mean']}")
    x0 = torch.from_numpy(golden5[f"{lp['name']}/x_init"]).to(dev)
    feats = case["feats"].to(dev)
    traj, _ = eng.sample_loop(plan, sch, x0, feats, ratio=lp["ratio"], mean_type=mt, use_graph=True)
    traj = traj.clone()
    assert rel(traj, golden5[f"{lp['name']}/imgs"]) < TRAJ32
    eager, _ = eng.sample_loop(plan, sch, x0, feats, ratio=lp["ratio"], mean_type=mt, use_graph=False)
    assert torch.equal(eager, traj)
    assert rel(_per_step_loop(eng, plan, sch, x0, feats, lp["T"], lp["ratio"], mt), traj) < 1e-6


def test_loop_samplers_captured_vs_eager(golden5, dev):
    """DDPM and classifier-free guidance inside the captured loop give the eager loop's poses."""
    from diffassemble_amd import Schedule, _lib
    from oracle import diffusion as ODF
    spec = GC.by_name("gcn_k36_noloop")
    case = GC.build_case(spec)
    eng = _engine(case, "fp32", dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch = Schedule(ODF.make_schedule(50), dev)
    x0, feats = case["x"].to(dev), case["feats"].to(dev)
    noise = torch.randn((50, 36, 2), generator=torch.Generator().manual_seed(3)).to(dev)
    for kw in (dict(sampler="DDPM", noise=noise), dict(cfg_w=0.5)):
        a = eng.sample_loop(plan, sch, x0, feats, mean_type=_lib.MEAN_EPSILON, use_graph=True, **kw)[0].clone()
        b = eng.sample_loop(plan, sch, x0, feats, mean_type=_lib.MEAN_EPSILON, use_graph=False, **kw)[0]
        assert torch.isfinite(a).all() and torch.equal(a, b), kw


def test_module_forward_returns_no_attentions(golden5, dev):
    from diffassemble_amd.model.backbones import Eff_GAT
    spec = GC.by_name("gcn_dropout")
    case = GC.build_case(spec)
    m = Eff_GAT(spec["steps"], input_channels=4, output_channels=4, architecture="gcn", visual_pretrained=False)
    m.load_state_dict(case["sd"], strict=False)
    m = m.to(dev).eval()
    m.precision = "fp32"
    out, att = m.forward_with_feats(case["x"].to(dev), case["t"].to(dev), None, case["edge_index"].to(dev),
                                    case["feats"].to(dev), case["batch"].to(dev))
    assert att is None
    assert rel(out, golden5["gcn_dropout/out"]) < RTOL32
    # the standalone backbone through the kernel-level ABI: gcn.py:16-22 on the same graph
    h = torch.randn(100, 1152, generator=torch.Generator().manual_seed(1))
    y, none = m.gnn_backbone(h.to(dev), case["edge_index"].to(dev), case["batch"].to(dev))
    ref = h
    for l in range(2):
        p = f"gnn_backbone.module_list.{l}."
        ref = torch.nn.functional.gelu(GC.gcn_conv(ref, case["edge_index"], case["sd"][p + "lin.weight"], case["sd"][p + "bias"]))
    assert none is None and rel(y, ref) < RTOL32


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_3d(prec, golden5, dev):
    spec = GC.GCN_FWD3D[0]
    case = GC.build_case(spec, "3d")
    eng = _engine(case, prec, dev, "3d")
    plan = eng.plan(case["edge_index"], case["batch"])
    out = eng.forward(plan, case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev))
    assert rel(out, golden5[f"{spec['name']}/out"]) < (RTOL32 if prec == "fp32" else RTOLBF)


def test_loop_3d(golden5, dev):
    from diffassemble_amd import Schedule, _lib
    from oracle import diffusion as ODF
    lp = GC.GCN_LOOPS3D[0]
    spec = GC.by_name(lp["base"])
    case = GC.build_case(spec, "3d")
    eng = _engine(case, "fp32", dev, "3d")
    plan = eng.plan(case["edge_index"], case["batch"])
    sch = Schedule(ODF.make_schedule(lp["T"]), dev)
    x0 = torch.from_numpy(golden5[f"{lp['name']}/x_init"]).to(dev)
    traj, _ = eng.sample_loop(plan, sch, x0, case["feats"].to(dev), ratio=lp["ratio"], mean_type=_lib.MEAN_START_X,
                              max_iters=lp["max_iters"], use_graph=True)
    assert rel(traj, golden5[f"{lp['name']}/imgs"]) < TRAJ32


def test_csr_gather_edge_cases(dev):
    """The CSR kernels (k_gcn_dinv, k_gcn_agg_csr) on multi-edges, existing self loops, directed edges, an isolated node and a
    1-node graph, against the restatement."""
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    from diffassemble_amd.graph_plan import build_plan
    src = [1, 1, 0, 2, 3, 0, 5, 5, 1]
    dst = [0, 0, 0, 3, 1, 3, 5, 5, 2]
    ei = torch.tensor([src, dst], dtype=torch.int64)
    batch = torch.tensor([0, 0, 0, 0, 0, 0, 1])
    plan = build_plan(ei.to(dev), batch.to(dev), 0, hybrid="off")
    assert not plan.dense and not plan.hybrid and plan.row_ptr is not None
    g = torch.Generator().manual_seed(5)
    x, b = torch.randn(7, 256, generator=g), torch.randn(256, generator=g)
    ref = GC.gcn_conv(x, ei, torch.eye(256), b)
    for prec, tol in (("fp32", 1e-6), ("bf16", RTOLBF)):
        out = E.gcn_aggregate(plan, x.to(dev), b.to(dev), _lib.ACT_NONE, prec)
        assert rel(out.float(), ref) < tol, prec
        out = E.gcn_aggregate(plan, x.to(dev), b.to(dev), _lib.ACT_GELU, prec)
        assert rel(out.float(), torch.nn.functional.gelu(ref)) < tol, prec


def test_alpha_is_refused(dev):
    from diffassemble_amd import _lib
    case = GC.build_case(GC.by_name("gcn_k36_noloop"))
    eng = _engine(case, "fp32", dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    with pytest.raises(_lib.DaError):
        eng.forward(plan, case["x"].to(dev), case["t"].to(dev), case["feats"].to(dev), return_alpha=True)


def _gnn_diffusion(spec, case, mean, dev):
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=spec["steps"], sampling="DDIM", rotation=spec["c"] == 4, visual_pretrained=False,
                      model_mean_type=getattr(ModelMeanType, mean), architecture="gcn")
    m.model.load_state_dict(case["sd"], strict=False)
    return m.to(dev).train()


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("tr", GC.GCN_TRAIN2D, ids=lambda s: s["name"])
def test_p_losses_gradients_match_reference_fixture(tr, staged, golden5, dev):
    """The reference's own p_losses + backward with the GCN backbone (golden_v5.npz): the loss and every live gradient, through
    da_train_forward / da_train_backward (complete graphs: closed-form aggregation; the random-dropout Batch: CSR gather and
    the transposed backward over the by-source CSR), in one call and as the EARLY / LATE halves of the bucketed exchange."""
    GTOL = 1e-3
    spec = GC.by_name(tr["base"])
    case = GC.build_case(spec)
    m = _gnn_diffusion(spec, case, tr["mean"], dev)
    te = m.model.train_engine(dev)
    te.force_staged = staged
    t = torch.from_numpy(golden5[f"{tr['name']}/t"]).to(dev)
    noise = torch.from_numpy(golden5[f"{tr['name']}/noise"]).to(dev)
    loss = m.p_losses(case["x"].to(dev), t, noise=noise, loss_type="huber", cond=None, edge_index=case["edge_index"].to(dev),
                      batch=case["batch"].to(dev), patch_feats=case["feats"].to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert rel(loss.detach(), golden5[f"{tr['name']}/loss"]) < 1e-5
    live = {k: p for k, p in m.model.named_parameters() if f"{tr['name']}/grad_head/{k}" in golden5.files}
    assert len(live) == 17 and "gnn_backbone.module_list.0.bias" in live
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in live.values())
    for k, p in live.items():
        ref = torch.from_numpy(golden5[f"{tr['name']}/grad_head/{k}"]).double()
        got = p.grad.flatten()[: ref.numel()].double().cpu()
        assert float((got - ref).abs().max()) / max(float(ref.abs().max()), floor) < GTOL, k
        g = p.grad.double().cpu()
        st, st_ref = torch.stack([g.sum(), g.abs().sum(), (g * g).sum()]), golden5[f"{tr['name']}/grad_stats/{k}"]
        if float(st_ref[1]) > floor * p.numel() * 1e-2:
            assert abs(float(st[1]) - float(st_ref[1])) / float(st_ref[1]) < GTOL, k
            assert abs(float(st[2]) - float(st_ref[2])) / float(st_ref[2]) < 2 * GTOL, k


def test_configure_optimizers_step_matches_transformers_adafactor(golden5, dev):
    """One training step of the GCN model: p_losses backward, then configure_optimizers()'s step over the flat buffers,
    against transformers' Adafactor (the reference's optimizer, spatial_diffusion.py:701-705) given the same gradients."""
    from transformers.optimization import Adafactor
    tr = GC.GCN_TRAIN2D[1]
    spec = GC.by_name(tr["base"])
    case = GC.build_case(spec)
    m = _gnn_diffusion(spec, case, tr["mean"], dev)
    opt = m.configure_optimizers()
    te = m.model.train_engine(dev)
    loss = m.p_losses(case["x"].to(dev), torch.from_numpy(golden5[f"{tr['name']}/t"]).to(dev),
                      noise=torch.from_numpy(golden5[f"{tr['name']}/noise"]).to(dev), loss_type="huber", cond=None,
                      edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev), patch_feats=case["feats"].to(dev))
    loss.backward()
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in te.params]
    for rp, gv in zip(ref_params, te.grad_views):
        rp.grad = gv.detach().clone()
    assert all(float(rp.grad.abs().max()) > 0 for rp in ref_params)
    ref = Adafactor(ref_params)
    before = te.flat.clone()
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, te.flat)
    for n, p, rp in zip(te.names, te.params, ref_params):
        assert rel(p.detach(), rp.detach()) < 2e-6, n
