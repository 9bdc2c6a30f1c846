"""GPU tests of the PointNet++ fragment encoder (backbone="pointnet_plus"; da_pointnet_plus.hip through
diffassemble_amd.pointnet_plus_encoder and model/backbones/pointnet.py) against the contract of tests/golden/pointnet_plus_refs.py
on the generated weights and clouds of tests/golden/pointnet_plus_v1.npz (the contract itself is held against the reference's
module by tests/test_pointnet_plus_host.py).

Selections (farthest point sampling, ball query): index for index.  Eval parity: max |out - contract| <= 1e-4 max |contract|
(RTOL32, the project's fp32 parity bound).  Every parity test prints the figure it measures (pytest -s)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointnet_plus_refs as R
import train3d_cases as T3
from oracle import denoiser as OD
from oracle import weights as W

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_plus_v1.npz"))
CASES = [(1, 1), (1, 64), (2, 513), (3, 1000), (2, 2048), (20, 1000)]
RTOL32 = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def case(P, N):
    """One case, computed once and left unchanged: cloud, starts, the contract's selections and its fp64 output."""
    pre = f"case/{P}x{N}/"
    pts = R.make_cloud(P, N, int(GOLD[pre + "cloud_seed"]))
    start = (torch.from_numpy(GOLD[pre + "start1"].astype(np.int64)), torch.from_numpy(GOLD[pre + "start2"].astype(np.int64)))
    sel = R.select(pts, start[0].numpy(), start[1].numpy())
    out = R.eval_forward(R.state(torch.float64), torch.from_numpy(pts).double(), sel)
    return SimpleNamespace(pts=torch.from_numpy(pts), start=start, sel=sel, out=out, seed=int(GOLD[pre + "seed"]))


@functools.lru_cache(maxsize=None)
def make_net(dev):
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    net = PointNetPlus()
    net.load_state_dict(R.state(), strict=True)
    return net.to(dev).eval()


# ------------------------------------------------------------------------------------------------------------ selections
@pytest.mark.parametrize("P,N", CASES)
def test_fps_and_ball_query_are_index_exact(dev, P, N):
    from diffassemble_amd import pointnet_plus_encoder as E
    c = case(P, N)
    pts = c.pts.to(dev)
    fps1 = E.fps(pts, R.S1, c.start[0])
    assert fps1.dtype == torch.int32 and np.array_equal(fps1.cpu().numpy(), c.sel["fps1"])
    grp1 = E.ball_query(pts, fps1, R.R1, R.K1)
    assert np.array_equal(grp1.cpu().numpy(), c.sel["grp1"])
    l1_xyz = torch.gather(pts, 1, fps1.long()[:, :, None].expand(-1, -1, 3))
    fps2 = E.fps(l1_xyz, R.S2, c.start[1])
    assert np.array_equal(fps2.cpu().numpy(), c.sel["fps2"])
    assert np.array_equal(E.ball_query(l1_xyz, fps2, R.R2, R.K2).cpu().numpy(), c.sel["grp2"])


def test_selections_on_made_up_clouds(dev):
    from diffassemble_amd import pointnet_plus_encoder as E
    # every point twice: ties go to the lowest index, and once every distance is 0 the pick is index 0
    half = case(2, 513).pts[:, :300]
    twice = torch.cat([half, half], 1)
    start = torch.tensor([450, 7])
    want = R.fps(twice.numpy(), 512, start.numpy())
    assert (want[:, 1:300] < 300).all() and not want[:, 300:].any()
    got = E.fps(twice.to(dev), 512, start)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(E.ball_query(twice.to(dev), got, 0.2, 32).cpu().numpy(), R.ball_query(twice.numpy(), want, 0.2, 32))
    # N = 1
    one = torch.tensor([[[0.25, -0.5, 0.125]]])
    assert not E.fps(one.to(dev), 512, torch.zeros(1)).any() and not E.ball_query(one.to(dev), torch.zeros(1, 512), 0.2, 32).any()
    # a centre with two neighbours on one axis at the two fp16 values next to 0.2: one inside the ball, one outside
    lo, hi = float(np.float16(0.2)), float(np.nextafter(np.float16(0.2), np.float16(1)))
    assert lo < 0.2 < hi
    line = torch.tensor([[[0.0, 0, 0], [-hi, 0, 0], [lo, 0, 0], [0, hi, 0], [0, 0, -lo]]])
    got = E.ball_query(line.to(dev), torch.tensor([[0]]), 0.2, 4).cpu().numpy()
    assert got.tolist() == [[[0, 2, 4, 0]]] and np.array_equal(got, R.ball_query(line.numpy(), [[0]], 0.2, 4))


# ------------------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("P,N", CASES)
def test_eval_parity(dev, P, N):
    c = case(P, N)
    out = make_net(dev)(c.pts.to(dev), fps_start=c.start)
    assert out.shape == (P, 256) and out.dtype == torch.float32
    e = rel(out, c.out)
    print(f"pointnet_plus eval {P}x{N}: rel err {e:.3e}")
    assert e <= RTOL32
    torch.manual_seed(c.seed)                          # the module's own draw: the reference's starts
    assert torch.equal(make_net(dev)(c.pts.to(dev)), out)


def test_batch_invariance_and_reproducibility(dev):
    net, c = make_net(dev), case(3, 1000)
    pts = c.pts.to(dev)
    out = net(pts, fps_start=c.start)
    assert torch.equal(net(pts, fps_start=c.start), out)
    k = 7
    big = net(torch.cat([pts] * k), fps_start=tuple(torch.cat([s] * k) for s in c.start))
    assert torch.equal(big, torch.cat([out] * k))
    assert torch.equal(net(pts[1:2], fps_start=tuple(s[1:2] for s in c.start)), out[1:2])


def test_empty_and_strided_out(dev):
    net, c = make_net(dev), case(2, 513)
    assert net(torch.zeros(0, 20, 3, device=dev)).shape == (0, 256)
    pts = c.pts.to(dev)
    buf = torch.full((2, 400), 7.0, device=dev)
    view = buf[:, 64:320]
    got = net.engine().forward(pts, c.start, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, net(pts, fps_start=c.start))
    assert bool((buf[:, :64] == 7.0).all()) and bool((buf[:, 320:] == 7.0).all())


def test_refusals(dev):
    from diffassemble_amd import _lib
    from diffassemble_amd import pointnet_plus_encoder as E
    from diffassemble_amd.model.backbones.pointnet import PointNetPlus
    net = make_net(dev)
    with pytest.raises(_lib.DaError, match="n_points 2049"):
        net(torch.zeros(1, 2049, 3, device=dev))
    with pytest.raises(_lib.DaError, match="n_points 2049"):
        E.fps(torch.zeros(1, 2049, 3, device=dev), 4, torch.zeros(1))
    with pytest.raises(NotImplementedError, match="normal_channel"):
        PointNetPlus(normal_channel=True)
    other = PointNetPlus().to(dev).train()
    with pytest.raises(NotImplementedError, match=r"follow-up.*inference needs \.eval\(\)"):
        other(case(1, 64).pts.to(dev))


# ------------------------------------------------------------------------------------------------------------ through the model
def test_model_features_are_the_engines(dev):
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.pointnet_plus_encoder import PointNetPlusEngine
    m = Eff_GAT_3d(steps=10, backbone="pointnet_plus").to(dev).eval()
    m.pcd_encoder.load_state_dict(R.state(), strict=True)
    c = case(2, 513)
    torch.manual_seed(c.seed)
    feats = m.pcd_features(c.pts.to(dev))
    assert feats.shape == (2, 256)
    assert torch.equal(feats, PointNetPlusEngine(R.state(), device=dev).forward(c.pts.to(dev), c.start))


def test_forward_with_feats_d320_matches_the_oracle(dev):
    """The denoiser at D = 256 + 64 = 320 (8 heads of 40) on a 5-part complete graph against oracle.denoiser's 3D forward, under the
    bound of the existing 3D parity test (RTOL32 = 1e-4 in fp32 parity mode)."""
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    sd = W.make_denoiser_state(50, 7, None, D=320, hidden=256, variant="3d", seed=72, qk_gain=2.0)
    m = Eff_GAT_3d(steps=50, backbone="pointnet_plus")
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    m = m.to(dev).eval()
    m.precision = "fp32"
    ei, batch = W.collate([W.dense_edge_index(5, True)], [5])
    x = T3.poses(5, 9)
    t = torch.from_numpy(np.random.default_rng(2).integers(0, 50, 5))
    feats = torch.from_numpy(np.random.default_rng(3).standard_normal((5, 256)).astype(np.float32)).clamp_min(0)
    out, _ = m.forward_with_feats(x.to(dev), t.to(dev), ei.to(dev), feats.to(dev), batch.to(dev))
    ref, _ = OD.eff_gat_3d_forward_with_feats(sd, x, t, ei, feats, batch)
    e = rel(out, ref)
    print(f"forward_with_feats D=320 vs oracle: {e:.3e}")
    assert e < RTOL32


def test_denoiser_backward_d320_matches_oracle_autograd(dev):
    """Training the denoiser on this backbone's (precomputed) features runs the edge-list attention backward at heads of 40: the
    parameter gradients and d_feats against the oracle's autograd on two complete graphs (5 + 3 parts), under the bound of the
    existing 3D backward test (test_gpu_train3d: 1e-3 of each tensor's largest gradient, floored at 1e-4 of the largest of all)."""
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    GTOL = 1e-3
    sd = W.make_denoiser_state(50, 7, None, D=320, hidden=256, variant="3d", seed=73)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in (5, 3)], [5, 3])
    rng = np.random.default_rng(73)
    x, t = T3.poses(8, 73), torch.from_numpy(rng.integers(0, 50, size=2))[batch]
    feats = torch.from_numpy(rng.standard_normal((8, 256)).astype(np.float32)).clamp_min(0)
    functional = torch.from_numpy(rng.standard_normal((8, 7)).astype(np.float32))
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fg = feats.clone().requires_grad_(True)
    pred, _ = OD.eff_gat_3d_forward_with_feats(sdg, x, t, edge_index, fg, batch)
    (pred * functional).sum().backward()
    m = Eff_GAT_3d(steps=50, backbone="pointnet_plus", freeze_backbone=True)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    m = m.to(dev).train()
    f = feats.to(dev).requires_grad_(True)
    out, _ = m.forward_with_feats(x.to(dev), t.to(dev), edge_index.to(dev), f, batch.to(dev))
    assert rel(out, pred) < RTOL32
    (out * functional.to(dev)).sum().backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    floor = 1e-4 * max(float(v.grad.abs().max()) for v in sdg.values())
    errs = {k: float((params[k].grad.double().cpu() - v.grad.double()).abs().max()) / max(float(v.grad.abs().max()), floor) for k, v in sdg.items()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"denoiser backward D=320: worst gradient {worst[0]} {worst[1]:.3e}; d_feats {rel(f.grad, fg.grad):.3e}")
    assert all(e < GTOL for e in errs.values()), {k: e for k, e in errs.items() if e >= GTOL}
    assert rel(f.grad, fg.grad) < GTOL


def diffusion_module(dev, seed=82, steps=20):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=steps, sampling="DDIM", inference_ratio=2, noise_weight=0.0, model_mean_type=ModelMeanType.START_X,
                      backbone="pointnet_plus", max_num_part=6, loss_type="all", freeze_backbone=True)
    sd = W.make_denoiser_state(steps, 7, None, D=320, hidden=256, variant="3d", seed=seed)
    missing, unexpected = m.model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    m.model.pcd_encoder.load_state_dict(R.state(), strict=True)
    return m.to(dev).eval()


def test_sampling_loop_and_steps_from_raw_fragments(dev):
    m = diffusion_module(dev)
    sizes = (5, 3)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    pcds = torch.cat([case(3, 1000).pts[:, :200], case(20, 1000).pts[:5, :200]]).to(dev)
    b = SimpleNamespace(x=T3.poses(8, 45).to(dev), pcds=pcds, edge_index=edge_index.to(dev), batch=batch.to(dev),
                        category=["everyday", "everyday"])
    torch.manual_seed(5)
    a, _ = m.p_sample_loop(b.x.shape, b.pcds, b.edge_index, b.batch)
    torch.manual_seed(5)
    feats = m.pcd_features(b.pcds)                     # the same first draws of the host generator as inside the loop
    torch.manual_seed(5)
    c, _ = m.p_sample_loop(b.x.shape, None, b.edge_index, b.batch, pcd_feats=feats)
    assert len(a) == 10 and all(torch.equal(x, y) for x, y in zip(a, c)) and bool(torch.isfinite(a[-1]).all())
    m.initialize_torchmetrics(["everyday"])
    for step in (m.validation_step, m.test_step):
        poses = step(b, 0)
        assert poses.shape == (8, 7) and bool(torch.isfinite(poses).all())
    assert 0.0 <= float(m.metrics["part_acc_everyday"].compute()) <= 1.0
