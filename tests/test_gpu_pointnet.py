"""GPU tests of the PointNet fragment encoder (backbone="pointnet"; da_pointnet.hip through diffassemble_amd.pointnet_encoder and
model/backbones/pointnet.py) against the fp64 contract of tests/golden/pointnet_refs.py on the weights and clouds of
tests/golden/pointnet_v1.npz (the contract itself is held against the reference's module by tests/test_pointnet_host.py).

Eval parity: max |out - ref| <= 1e-4 max |ref| (the project's fp32 parity bound).
Train parity, per tensor: max |x - ref| / max |ref| <= max(16 x the reference's own recorded fp32-versus-fp64 deviation, 1e-5).
The max routes a gradient to ONE point, discontinuously at ties: the loss weight of every (fragment, channel) whose two largest
values lie closer than 1e-4 in the contract is set to zero; at most 1 % of a case's pairs may be masked (asserted).
Every test prints the figures it measures (pytest -s)."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointnet_refs as R
import train3d_cases as T3
from oracle import denoiser as OD
from oracle import weights as W

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet_v1.npz"))
CASES = [(1, 1), (1, 20), (2, 63), (3, 65), (5, 257), (20, 1000)]
TRAIN_CASES = [c for c in CASES if c[0] * c[1] >= 20]
RTOL32, FACTOR, FLOOR, GAP, GAP_CAP = 1e-4, 16, 1e-5, 1e-4, 0.01


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def state(dtype=torch.float32):
    return {k: torch.from_numpy(GOLD[f"sd/{k}"]).to(dtype if GOLD[f"sd/{k}"].dtype.kind == "f" else torch.int64) for k in GOLD["keys"]}


def points(P, N, dtype=torch.float32):
    return torch.from_numpy(GOLD[f"case/{P}x{N}/points"].astype(np.float32)).to(dtype)


def make_net(dev, train=False):
    from diffassemble_amd.model.backbones.pointnet import PointNet
    net = PointNet(128)
    net.load_state_dict(state(), strict=True)
    return net.to(dev).train(train)


def rel(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def contract(P, N):
    """The fp64 contract of one case, computed once: eval output, train record, masked loss weights, gradients."""
    sd, pts = state(torch.float64), points(P, N, torch.float64)
    c = SimpleNamespace(eval_out=R.eval_forward(sd, pts))
    if P * N >= 2:
        c.f = R.train_forward(sd, pts)
        open_ = R.top2_gap(c.f.z5) < GAP
        c.masked = float(open_.double().mean())
        c.w = torch.from_numpy(GOLD[f"case/{P}x{N}/w"]).double() * (~open_)
        c.grads = R.backward(sd, pts, c.f, c.w)
    return c


def tol(P, N, name):
    return max(FACTOR * float(GOLD[f"case/{P}x{N}/dev/{name}"]), FLOOR)


# ------------------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("P,N", CASES)
def test_eval_parity(dev, P, N):
    out = make_net(dev)(points(P, N).to(dev))
    assert out.shape == (P, 128) and out.dtype == torch.float32
    e = rel(out, contract(P, N).eval_out)
    print(f"pointnet eval {P}x{N}: rel err {e:.3e} (reference fp32 itself {float(GOLD[f'case/{P}x{N}/dev/eval_out']):.3e})")
    assert e <= RTOL32


def test_eval_empty_and_strided_out(dev):
    net = make_net(dev)
    out = net(torch.zeros(0, 20, 3, device=dev))
    assert out.shape == (0, 128)
    pts = points(3, 65).to(dev)
    buf = torch.full((3, 200), 7.0, device=dev)
    view = buf[:, 40:168]
    got = net.engine().forward(pts, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, net(pts))
    assert bool((buf[:, :40] == 7.0).all()) and bool((buf[:, 168:] == 7.0).all())


def test_eval_negative_maxima_and_chunk_invariance(dev):
    """Pooled values are often negative (the maxima start from -inf, not 0), and a fragment cut over several workgroups (P = 20:
    16 workgroups per fragment and the second pass) gives the bits of the same fragment walked by ONE workgroup (P = 2400 > 2048:
    no second pass): the max is exact."""
    net = make_net(dev)
    pts = points(20, 1000).to(dev)
    out = net(pts)
    assert float(out.min()) < 0
    big = net(torch.cat([pts] * 120))
    assert torch.equal(big[:20], out) and torch.equal(big[2380:], out)


def test_eval_other_feat_dims(dev):
    """feat_dim is a parameter of the eval kernel: a multiple of 32 up to 128 (here 64 against the contract); others are refused."""
    from diffassemble_amd import _lib
    from diffassemble_amd.model.backbones.pointnet import PointNet
    torch.manual_seed(11)
    for feat, ok in ((64, True), (48, False), (160, False)):
        net = PointNet(feat)
        with torch.no_grad():
            for l in range(1, 6):
                bn = getattr(net, f"bn{l}")
                bn.running_mean.normal_(0, 0.3), bn.running_var.uniform_(0.25, 1.75), bn.weight.uniform_(-1.5, 1.5), bn.bias.normal_(0, 0.3)
        sd = {k: v.double() for k, v in net.state_dict().items() if v.is_floating_point()}
        net = net.to(dev).eval()
        if ok:
            out = net(points(3, 65).to(dev))
            assert out.shape == (3, feat) and rel(out, R.eval_forward(sd, points(3, 65, torch.float64))) <= RTOL32
        else:
            with pytest.raises(_lib.DaError, match="multiple of 32 up to 128"):
                net(points(3, 65).to(dev))


# ------------------------------------------------------------------------------------------------------------ train
def run_train(dev, P, N, w):
    net = make_net(dev, train=True)
    out = net(points(P, N).to(dev))
    (out * w.to(dev, torch.float32)).sum().backward()
    torch.cuda.synchronize()
    return net, out.detach()


@pytest.mark.parametrize("P,N", TRAIN_CASES)
def test_train_parity(dev, P, N):
    c = contract(P, N)
    assert c.masked <= GAP_CAP, c.masked
    net, out = run_train(dev, P, N, c.w)
    worst = {}

    def hold(name, got, ref):
        e = rel(got, ref)
        worst[name] = e
        assert e <= tol(P, N, name), (name, e, tol(P, N, name))

    try:
        hold("train_out", out, c.f.out)
        for l in range(1, 6):
            bn = getattr(net, f"bn{l}")
            hold(f"run_mean/{l}", bn.running_mean, c.f.run_mean[l - 1])
            hold(f"run_var/{l}", bn.running_var, c.f.run_var[l - 1])
            assert int(bn.num_batches_tracked) == 1
        params = dict(net.named_parameters())
        for k in R.param_keys():
            assert params[k].grad is not None and params[k].grad.shape == params[k].shape, k
            hold(f"grad/{k}", params[k].grad, c.grads[k])
    finally:
        top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
        print(f"pointnet train {P}x{N}: masked pairs {c.masked:.4%}; worst rel errs " + ", ".join(f"{k} {v:.2e}" for k, v in top))


def test_train_is_bitwise_reproducible(dev):
    c = contract(20, 1000)
    a_net, a_out = run_train(dev, 20, 1000, c.w)
    b_net, b_out = run_train(dev, 20, 1000, c.w)
    assert torch.equal(a_out, b_out)
    for (k, p), q in zip(a_net.named_parameters(), b_net.parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, p), q in zip(a_net.named_buffers(), b_net.buffers()):
        assert torch.equal(p, q), k


def test_train_ties_go_to_the_lowest_index(dev):
    """Every point of a cloud twice: each maximum is attained at n and n + N / 2; the gradient must be the one of routing to n."""
    half = points(3, 65)[:, :32]
    pts = torch.cat([half, half], 1).double()
    sd = state(torch.float64)
    f = R.train_forward(sd, pts)
    assert int(f.arg.max()) < 32
    w = torch.from_numpy(GOLD["case/3x65/w"]).double()
    grads = R.backward(sd, pts, f, w)
    net = make_net(dev, train=True)
    (net(pts.float().to(dev)) * w.float().to(dev)).sum().backward()
    for k, p in net.named_parameters():
        assert rel(p.grad, grads[k]) <= tol(3, 65, f"grad/{k}"), (k, rel(p.grad, grads[k]))


def test_train_refusals(dev):
    net = make_net(dev, train=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        net(points(1, 1).to(dev))
    with pytest.raises(NotImplementedError):
        net(points(1, 20).to(dev).requires_grad_(True))
    with torch.no_grad():                                          # no gradient wanted: the forward alone, buffers still updated
        out = net(points(1, 20).to(dev))
    assert not out.requires_grad and int(net.bn3.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------------------ through the model
def test_model_features_are_the_engines(dev):
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    from diffassemble_amd.pointnet_encoder import PointNetEngine
    m = Eff_GAT_3d(steps=10, backbone="pointnet").to(dev).eval()
    m.pcd_backbone.load_state_dict(state(), strict=True)
    pts = points(5, 257).to(dev)
    feats = m.pcd_features(pts)
    assert feats.shape == (5, 128)
    assert torch.equal(feats, PointNetEngine(state(), device=dev).forward(pts))


def test_forward_with_feats_d192_matches_the_oracle(dev):
    """The denoiser at D = 128 + 64 = 192 (8 heads of 24) on a 5-part complete graph against oracle.denoiser's 3D forward, under the
    bound of the existing 3D parity test (test_gpu_parity.test_forward_3d: RTOL32 = 1e-4 in fp32 parity mode)."""
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    sd = W.make_denoiser_state(50, 7, None, D=192, hidden=256, variant="3d", seed=71, qk_gain=2.0)
    m = Eff_GAT_3d(steps=50, backbone="pointnet")
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    m.pcd_backbone.load_state_dict(state(), strict=True)
    m = m.to(dev).eval()
    m.precision = "fp32"
    pts = points(5, 257).to(dev)
    ei, batch = W.collate([W.dense_edge_index(5, True)], [5])
    x = T3.poses(5, 9)
    t = torch.from_numpy(np.random.default_rng(2).integers(0, 50, 5))
    feats = m.pcd_features(pts)
    out, _ = m.forward_with_feats(x.to(dev), t.to(dev), ei.to(dev), feats, batch.to(dev))
    ref, _ = OD.eff_gat_3d_forward_with_feats(sd, x, t, ei, feats.cpu(), batch)
    e = rel(out, ref)
    print(f"forward_with_feats D=192 vs oracle: {e:.3e}")
    assert e < RTOL32


def diffusion_module(dev, freeze, seed=81, steps=20):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=steps, sampling="DDIM", inference_ratio=2, noise_weight=0.0, model_mean_type=ModelMeanType.START_X,
                      backbone="pointnet", max_num_part=6, loss_type="all", freeze_backbone=freeze)
    sd = W.make_denoiser_state(steps, 7, None, D=192, hidden=256, variant="3d", seed=seed)
    missing, unexpected = m.model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    m.model.pcd_backbone.load_state_dict(state(), strict=True)
    return m.to(dev)


def small_batch(dev, sizes=(5, 3), n_points=65, n_parts=6, seed=45, steps=20):
    P = sum(sizes)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.integers(0, steps, size=len(sizes)))[batch]
    noise = tuple(torch.from_numpy(a.astype(np.float32)).to(dev) for a in
                  (rng.standard_normal((P, 3)), rng.standard_normal((P, 3)), rng.uniform(0.05, 0.95, P)))
    pcds = torch.cat([points(5, 257)[:, :n_points], points(3, 65)[:, :n_points]])
    return SimpleNamespace(x=T3.poses(P, seed).to(dev), pcds=pcds.to(dev), edge_index=edge_index.to(dev), batch=batch.to(dev),
                           valids=T3.valids_of(sizes, n_parts).to(dev), data_id=list(range(len(sizes))), t=t.to(dev), noise=noise)


def test_sampling_loop_from_raw_fragments(dev):
    m = diffusion_module(dev, freeze=True).eval()
    b = small_batch(dev)
    torch.manual_seed(5)
    a, _ = m.p_sample_loop(b.x.shape, b.pcds, b.edge_index, b.batch)
    torch.manual_seed(5)
    c, _ = m.p_sample_loop(b.x.shape, None, b.edge_index, b.batch, pcd_feats=m.pcd_features(b.pcds))
    assert len(a) == 10 and all(torch.equal(x, y) for x, y in zip(a, c)) and bool(torch.isfinite(a[-1]).all())
    bt = SimpleNamespace(x=b.x, pcds=b.pcds, edge_index=b.edge_index, batch=b.batch, category=["everyday", "everyday"])
    m.initialize_torchmetrics(["everyday"])
    assert m.validation_step(bt, 0).shape == (8, 7) and m.test_step(bt, 0).shape == (8, 7)
    assert 0.0 <= float(m.metrics["part_acc_everyday"].compute()) <= 1.0


def test_p_losses_trains_the_encoder(dev):
    """One p_losses with a trainable encoder on two objects (5 + 3 parts of 65 points): the gradient that reaches pcd_feats, fed to
    the contract's backward, gives the encoder's parameter gradients (train-parity tolerance of the 65-point case)."""
    m = diffusion_module(dev, freeze=False).train()
    b = small_batch(dev)
    seen = {}
    inner = m.model.pcd_features_train

    def spy(pcd):
        feats = inner(pcd)
        feats.retain_grad()
        seen["feats"] = feats
        return feats

    m.model.pcd_features_train = spy
    losses = m.p_losses(b.x, b.t, noise=b.noise, loss_type="all", cond=b.pcds, edge_index=b.edge_index, batch=b.batch, n_batch=2,
                        valids=b.valids)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    d_feats = seen["feats"].grad
    assert d_feats is not None and float(d_feats.abs().max()) > 0
    sd, pts = state(torch.float64), b.pcds.double().cpu()
    f = R.train_forward(sd, pts)
    assert rel(seen["feats"], f.out) <= tol(3, 65, "train_out")
    grads = R.backward(sd, pts, f, d_feats.double().cpu())
    worst = 0.0
    for k, p in m.model.pcd_backbone.named_parameters():
        e = rel(p.grad, grads[k])
        worst = max(worst, e)
        assert e <= tol(3, 65, f"grad/{k}"), (k, e)
    print(f"p_losses encoder gradients vs contract: worst rel err {worst:.2e}")


def test_optimizer_step_moves_the_encoder_and_frozen_gets_none(dev):
    from diffassemble_amd.train import FusedAdafactor, HybridAdafactor
    b = small_batch(dev)
    m = diffusion_module(dev, freeze=False).train()
    enc = m.model.pcd_backbone
    m.log = lambda *a, **k: None
    opt = m.configure_optimizers()
    assert isinstance(opt, HybridAdafactor)
    key0 = enc.engine_key()
    before = {k: p.detach().clone() for k, p in enc.named_parameters()}
    torch.manual_seed(3)
    m.training_step(b, 1).backward()
    opt.step()
    torch.cuda.synchronize()
    for k, p in enc.named_parameters():
        assert bool(torch.isfinite(p).all()) and not torch.equal(before[k], p.detach()), k
    assert enc.engine_key() != key0
    m.eval()
    assert bool(torch.isfinite(m.pcd_features(b.pcds)).all())        # the eval engine, rebuilt from the stepped parameters
    frozen = diffusion_module(dev, freeze=True).train()
    frozen.log = lambda *a, **k: None
    assert isinstance(frozen.configure_optimizers(), FusedAdafactor)
    frozen.training_step(b, 1).backward()
    assert all(p.grad is None for p in frozen.model.pcd_backbone.parameters())
    assert frozen.model.time_emb.weight.grad is not None
