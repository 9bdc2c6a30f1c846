"""GPU tests of the discrete position diffusion (DA_VARIANT_DISCRETE, da_d3pm.hip): the reverse-step kernel alone, its
generator, the forward against the reference's logits (golden_v7.npz), teacher-forced parity with the reference's own loop,
the captured loop against the eager per-step path, and the module.  Project bounds: fp32 within 1e-4, bf16 within 8e-3
(max-abs relative to the tensor's max-abs); argmax comparisons leave out near ties (discrete_cases.GAP / GAP_CAP)."""
import types

import numpy as np
import pytest
import torch

import discrete_cases as DC
from oracle import weights as W

pytestmark = pytest.mark.gpu

RTOL32, RTOLBF = 1e-4, 8e-3
V = DC.V7
N = sum(V["sizes"])


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g7():
    return DC.load_golden7()


@pytest.fixture(scope="module")
def case():
    return DC.v7_case()


def _sched(steps, dev):
    from diffassemble_amd import Schedule
    from oracle import diffusion as ODF
    cpu = ODF.make_schedule(steps)
    return Schedule(cpu, dev), cpu["alphas_cumprod"]


def _engine(sd, prec, dev):
    from diffassemble_amd import DenoiserEngine
    return DenoiserEngine(sd, variant="discrete", arch="transformer", precision=prec, device=dev)


def _seed(dev, seed, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


# ---------------------------------------------------------------------------------------- 1. the step kernel alone
@pytest.mark.parametrize("K", [2, 35, 36, 144, 900, 1024])
def test_step_kernel(K, dev):
    from diffassemble_amd import engine as E
    n, steps, ratio = 130, 600, 10
    sch, ac = _sched(steps, dev)
    gen = torch.Generator().manual_seed(1000 + K)
    logits = 3.0 * torch.randn(n, K, generator=gen)
    x_t = torch.randint(0, K, (n,), generator=gen)
    u = torch.rand(n, K, generator=gen)
    t = torch.tensor([0, ratio, 590, 337, 20, 599, 0, 100, ratio, 250] * (n // 10))
    x_prev, post = E.d3pm_step(sch, x_t.to(dev), logits.to(dev), t.to(dev), ratio, noise=u.to(dev), return_post=True)
    ref_prev, ref_post, gap = DC.reverse_step(ac, x_t, logits, t, ratio, u)
    err = float((post.double().cpu() - ref_post).abs().max())
    print(f"K={K}: post max abs err {err:.3e}, max |post| {float(ref_post.abs().max()):.3f}")
    assert err <= RTOL32 * float(ref_post.abs().max())
    DC.check_argmax(x_prev, ref_prev, gap, f"K={K}")
    assert torch.equal(x_prev.cpu()[t == 0], logits.argmax(-1)[t == 0])
    # a scalar t (the loop's form) gives the rows the per-node form gives
    tt = torch.full((n,), 590)
    a = E.d3pm_step(sch, x_t.to(dev), logits.to(dev), 590, ratio, noise=u.to(dev))
    assert torch.equal(a, E.d3pm_step(sch, x_t.to(dev), logits.to(dev), tt.to(dev), ratio, noise=u.to(dev)))


def test_step_rejects_a_scalar_t_inside_the_first_stride(dev):
    from diffassemble_amd import _lib
    from diffassemble_amd import engine as E
    sch, _ = _sched(100, dev)
    z = torch.zeros(4, 8, device=dev)
    with pytest.raises(_lib.DaError, match="ratio"):
        E.d3pm_step(sch, torch.zeros(4, dtype=torch.long, device=dev), z, 3, 5, noise=z + 0.5)


# ---------------------------------------------------------------------------------------- 2. the generator
def test_generator(dev):
    from diffassemble_amd import engine as E
    s = _seed(dev, 0x1234567890ABCDE, 7)
    u = E.d3pm_noise(s, 3, 64, 144)
    assert u.shape == (64, 144) and float(u.min()) > 0.0 and float(u.max()) <= 1.0
    assert torch.equal(u, E.d3pm_noise(s, 3, 64, 144))
    for other in (E.d3pm_noise(s, 4, 64, 144), E.d3pm_noise(_seed(dev, 0x1234567890ABCDF, 7), 3, 64, 144),
                  E.d3pm_noise(_seed(dev, 0x1234567890ABCDE, 8), 3, 64, 144)):
        assert float((other != u).float().mean()) > 0.99
    # offset shifts the flat element index: element e at offset 8 is element e + 1 at offset 7
    assert torch.equal(E.d3pm_noise(_seed(dev, 0x1234567890ABCDE, 8), 3, 64, 144).flatten()[:-1], u.flatten()[1:])
    big = E.d3pm_noise(s, 0, 8192, 128).flatten().double().cpu()          # 2^20 draws
    assert float(big.min()) > 0.0 and float(big.max()) <= 1.0
    assert abs(float(big.mean()) - 0.5) < 0.002                             # sigma of the mean = 0.2887 / 1024: about 7 sigma
    hist = torch.histc(big, bins=64, min=0.0, max=1.0)
    p = 1.0 / 64
    sigma = (big.numel() * p * (1 - p)) ** 0.5
    assert float((hist - big.numel() * p).abs().max()) < 6 * sigma
    # the step draws exactly these numbers when no noise buffer is given
    sch, _ = _sched(600, dev)
    gen = torch.Generator().manual_seed(5)
    n, K = 130, 144
    logits, x_t = (3.0 * torch.randn(n, K, generator=gen)).to(dev), torch.randint(0, K, (n,), generator=gen).to(dev)
    t = torch.tensor([0, 10, 590, 337, 20] * (n // 5), device=dev)
    own = E.d3pm_step(sch, x_t, logits, t, 10, seed=s, iteration=11)
    assert torch.equal(own, E.d3pm_step(sch, x_t, logits, t, 10, noise=E.d3pm_noise(s, 11, n, K)))
    assert not torch.equal(own, E.d3pm_step(sch, x_t, logits, t, 10, seed=s, iteration=12))


# ---------------------------------------------------------------------------------------- 3. forward
@pytest.mark.parametrize("folds_off", [0, 2, 3], ids=["both_folds", "mlp2_fold", "generic"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_against_reference(prec, folds_off, g7, case, dev):
    from diffassemble_amd import _lib
    old = _lib.set_config(disable_folds=folds_off)          # a denoiser keeps the folds it was created with
    try:
        eng = _engine(case["sd"], prec, dev)
    finally:
        _lib.set_config(disable_folds=old.disable_folds)
    assert (eng.flags & 3) == 3 - folds_off                 # bit 0: mlp.2 composed into its consumers, bit 1: folded last layer
    plan = eng.plan(case["edge_index"], case["batch"])
    assert plan.dense == 1
    feats = case["feats"].to(dev)
    for t in V["fwd_t"]:
        idx = torch.from_numpy(g7[f"fwd/t{t}/idx"]).to(dev)
        out = eng.forward_idx(plan, idx, torch.full((N,), t, dtype=torch.long, device=dev), feats)
        e = rel(out, g7[f"fwd/t{t}/logits"])
        print(f"forward_idx {prec} t={t}: rel err {e:.3e}")
        assert e < (RTOL32 if prec == "fp32" else RTOLBF)
        assert torch.equal(out, eng.forward_idx(plan, idx, t, None))          # scalar t, staged features


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_k35_incomplete_graphs(prec, dev):
    K, steps, sizes = 35, 50, (20, 35)
    sd = DC.make_discrete_state(K, steps, seed=35)
    rng = np.random.default_rng(35)
    ei, batch = W.collate([W.random_regular_edge_index(n, 6, rng) for n in sizes], sizes)
    n = sum(sizes)
    feats = W.randn((n, 1088), 36)
    gen = torch.Generator().manual_seed(37)
    idx = torch.randint(0, K, (n,), generator=gen)
    idx[:3] = torch.tensor([-4, K, K + 100])                               # clamped by the kernel, as t is
    t = torch.randint(0, steps, (n,), generator=gen)
    eng = _engine(sd, prec, dev)
    plan = eng.plan(ei, batch)
    assert plan.dense == 0
    out = eng.forward_idx(plan, idx.to(dev), t.to(dev), feats.to(dev))
    ref = DC.forward_with_feats(sd, idx.clamp(0, K - 1), t, ei, feats)
    e = rel(out, ref)
    print(f"forward_idx {prec} K=35 CSR: rel err {e:.3e}")
    assert out.shape == (n, K) and e < (RTOL32 if prec == "fp32" else RTOLBF)


# ---------------------------------------------------------------------------------------- 4. teacher-forced reference parity
def _module(case, dev, **kw):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=V["steps"], inference_ratio=V["ratio"], sampling="DDPM",
                      scheduler=SD.ModelScheduler.LINEAR, **kw)
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected and all(k.startswith(("visual_backbone", "mean", "std")) for k in missing)
    m.model.precision = "fp32"
    return m.to(dev).eval()


def test_teacher_forced_against_the_reference_loop(g7, case, dev):
    m = _module(case, dev)
    ac = m.alphas_cumprod.cpu()
    ei, batch, feats = case["edge_index"].to(dev), case["batch"].to(dev), case["feats"].to(dev)
    traj, uni = torch.from_numpy(g7["loop/traj"]), torch.from_numpy(g7["loop/uniforms"])
    x_t = torch.from_numpy(g7["loop/x_init"])
    got, ref, gaps = [], [], []
    for it, i in enumerate(reversed(range(0, V["steps"], V["ratio"]))):
        t = torch.full((N,), i, dtype=torch.long)
        got.append(m.p_sample_ddpm(x_t.to(dev), t.to(dev), i, None, ei, feats, batch, noise=uni[it].to(dev)).cpu())
        logits = DC.forward_with_feats(case["sd"], x_t, t, case["edge_index"], case["feats"])
        gaps.append(DC.reverse_step(ac, x_t, logits, t, V["ratio"], uni[it])[2])
        ref.append(traj[it])
        x_t = traj[it]                                                      # teacher forcing: the reference's own x_t
    assert got[0].dtype == torch.int64
    DC.check_argmax(torch.cat(got), torch.cat(ref), torch.cat(gaps), "loop")


def test_teacher_forced_guided_steps(g7, case, dev):
    m = _module(case, dev, classifier_free_prob=0.1, classifier_free_w=V["cfg_w"])
    ac, w = m.alphas_cumprod.cpu(), V["cfg_w"]
    ei, batch, feats = case["edge_index"].to(dev), case["batch"].to(dev), case["feats"].to(dev)
    got, ref, gaps = [], [], []
    for i in V["guided_t"]:
        x_t, u = torch.from_numpy(g7[f"guided/t{i}/x_t"]), torch.from_numpy(g7[f"guided/t{i}/uniforms"])
        t = torch.full((N,), i, dtype=torch.long)
        got.append(m.p_sample_ddpm(x_t.to(dev), t.to(dev), i, None, ei, feats, batch, noise=u.to(dev)).cpu())
        lc = DC.forward_with_feats(case["sd"], x_t, t, case["edge_index"], case["feats"])
        lu = DC.forward_with_feats(case["sd"], x_t, t, case["edge_index"], torch.zeros_like(case["feats"]))
        gaps.append(DC.reverse_step(ac, x_t, (1 + w) * lc - w * lu, t, V["ratio"], u)[2])
        ref.append(torch.from_numpy(g7[f"guided/t{i}/x_prev"]))
    DC.check_argmax(torch.cat(got), torch.cat(ref), torch.cat(gaps), "guided")


# ---------------------------------------------------------------------------------------- 5. the captured loop
def _eager_loop(eng, plan, sch, x0, feats, steps, ratio, noise, cfg_w, n_iters):
    x, traj = x0, []
    zeros = torch.zeros_like(feats)
    for it, i in enumerate(reversed(range(0, steps, ratio))):
        if it == n_iters:
            break
        logits = eng.forward_idx(plan, x, i, feats)
        if cfg_w is not None:
            unc = eng.forward_idx(plan, x, i, zeros)
            logits = (1 + cfg_w) * logits - cfg_w * unc
        x = eng.d3pm_step(sch, x, logits, i, ratio, noise=noise[it])
        traj.append(x)
    return torch.stack(traj)


@pytest.mark.parametrize("cfg_w", [None, 0.5], ids=["plain", "guided"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_loop_equals_the_eager_steps(prec, cfg_w, g7, case, dev):
    eng = _engine(case["sd"], prec, dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    feats = case["feats"].to(dev)
    x0 = torch.from_numpy(g7["loop/x_init"]).to(dev)
    noise = torch.from_numpy(g7["loop/uniforms"]).to(dev)
    n_iters = V["steps"] // V["ratio"]
    traj, xf = eng.sample_loop_idx(plan, sch, x0, feats, ratio=V["ratio"], use_graph=True, cfg_w=cfg_w, noise=noise)
    traj, xf = traj.clone(), xf.clone()
    assert traj.shape == (n_iters, N) and traj.dtype == torch.int32 and torch.equal(traj[-1], xf)
    assert int(traj.min()) >= 0 and int(traj.max()) < V["K"]
    eager = _eager_loop(eng, plan, sch, x0, feats, V["steps"], V["ratio"], noise, cfg_w, n_iters)
    assert torch.equal(traj.long(), eager)
    # a replay of the cached graph, and the same loop without a graph
    again, _ = eng.sample_loop_idx(plan, sch, x0, feats, ratio=V["ratio"], use_graph=True, cfg_w=cfg_w, noise=noise)
    assert torch.equal(again, traj)
    plain, _ = eng.sample_loop_idx(plan, sch, x0, feats, ratio=V["ratio"], use_graph=False, cfg_w=cfg_w, noise=noise)
    assert torch.equal(plain, traj)


def test_loop_seed_and_truncation(g7, case, dev):
    eng = _engine(case["sd"], "bf16", dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    feats = case["feats"].to(dev)
    x0 = torch.from_numpy(g7["loop/x_init"]).to(dev)
    kw = dict(ratio=V["ratio"], use_graph=True)
    a = eng.sample_loop_idx(plan, sch, x0, feats, generator=torch.Generator().manual_seed(11), **kw)[0].clone()
    b = eng.sample_loop_idx(plan, sch, x0, feats, generator=torch.Generator().manual_seed(11), **kw)[0].clone()
    c = eng.sample_loop_idx(plan, sch, x0, feats, generator=torch.Generator().manual_seed(12), **kw)[0].clone()
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the kernels read the seed on the device: the same draws through the stand-alone step reproduce the first iteration
    eng.seed_tensor(generator=torch.Generator().manual_seed(11))
    first = eng.d3pm_step(sch, x0, eng.forward_idx(plan, x0, 95, feats), 95, V["ratio"], seed=eng._seed, iteration=0)
    assert torch.equal(first, a[0].long())
    # max_iters truncates as in da_sample_loop
    short, xf = eng.sample_loop_idx(plan, sch, x0, feats, max_iters=3, generator=torch.Generator().manual_seed(11), **kw)
    assert short.shape == (3, N) and torch.equal(short, a[:3]) and torch.equal(xf, a[2])
    _, xf2 = eng.sample_loop_idx(plan, sch, x0, feats, max_iters=3, keep_traj=False, generator=torch.Generator().manual_seed(11), **kw)
    assert torch.equal(xf2, a[2])


# ---------------------------------------------------------------------------------------- 6. the module
def _batch(case, dev, indexes):
    return types.SimpleNamespace(indexes=indexes.to(dev), patches=None, edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                                 patches_dim=torch.tensor([[6, 6], [6, 6]], device=dev), patch_feats=case["feats"].to(dev))


def test_module_sampling_and_validation(case, dev):
    from diffassemble_amd import _lib
    m = _module(case, dev)
    imgs = m.p_sample_loop((N,), None, case["edge_index"].to(dev), case["batch"].to(dev), patch_feats=case["feats"].to(dev))
    assert len(imgs) == 20 and all(x.dtype == torch.int64 and x.shape == (N,) for x in imgs)
    assert all(int(x.min()) >= 0 and int(x.max()) < 36 for x in imgs)
    assert len(m.predict_step(_batch(case, dev, torch.zeros(N, dtype=torch.long)), 0)) == 20
    # rigged head: logits = 50 one_hot(c) for every piece, so a Batch whose every ground-truth index is c (mod K) is solved
    c = 17
    with torch.no_grad():
        m.model.final_mlp[2].weight.zero_()
        m.model.final_mlp[2].bias.copy_(50.0 * torch.nn.functional.one_hot(torch.tensor(c), 36).float())
    m.initialize_torchmetrics([(6, 6)])
    pred = m.validation_step(_batch(case, dev, c + 36 * torch.arange(N)), 0)
    assert torch.equal(pred.cpu(), torch.full((N,), c))
    assert float(m.metrics["overall_acc"].compute()) == 1.0 and float(m.metrics["overall__piece_acc"].compute()) == 1.0
    assert float(m.metrics["(6, 6)_acc"].compute()) == 1.0
    assert float(m.metrics["overall_nImages"].compute()) == 2.0 and float(m.metrics["(6, 6)_nImages"].compute()) == 2.0
    m.initialize_torchmetrics([(6, 6)])
    m.test_step(_batch(case, dev, torch.arange(N)[torch.randperm(N, generator=torch.Generator().manual_seed(1))]), 0)
    assert float(m.metrics["overall_acc"].compute()) == 0.0
    assert float(m.metrics["overall__piece_acc"].compute()) == pytest.approx(2 / N)
    # entries that take float poses reject the discrete engine (nothing is launched)
    eng = m.model.engine(dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    with pytest.raises(_lib.DaError, match="position indices"):
        eng.forward(plan, torch.zeros(N, 1, device=dev), 0, case["feats"].to(dev))
    with pytest.raises(_lib.DaError, match="position indices"):
        eng.sample_loop(plan, sch, torch.zeros(N, 1, device=dev), case["feats"].to(dev), ratio=5)
    with pytest.raises(_lib.DaError):
        eng.ddim_step(sch, torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev), 5, 5, _lib.MEAN_EPSILON)
    with pytest.raises(_lib.DaError):
        eng.ddpm_step(sch, torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev), 5)
