"""GPU tests of the discrete position + rotation diffusion (DA_VARIANT_DISCRETE_ROT, da_d3pm_rot.hip): the two-process reverse-step
kernel alone, the rotation draw domain, the two-headed forward with the addend-row select against the reference's logits
(golden_v9.npz), teacher-forced parity with the reference's own loops, the captured loop against the eager per-step path, the module,
and the position model's loop (the code this variant shares a library with).  Project bounds: fp32 within 1e-4, bf16 within 8e-3
(max-abs relative to the tensor's max-abs); argmax comparisons leave out near ties (discrete_cases.GAP / GAP_CAP)."""
import types

import numpy as np
import pytest
import torch

import discrete_cases as DC
import discrete_rot_cases as RC
from oracle import weights as W

pytestmark = pytest.mark.gpu

RTOL32, RTOLBF = 1e-4, 8e-3
V = RC.V9
N = sum(V["sizes"])
N_IT = V["steps"] // V["ratio"]
T_OF = list(reversed(range(0, V["steps"], V["ratio"])))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g9():
    return RC.load_golden9()


@pytest.fixture(scope="module")
def case():
    return RC.v9_case()


def _sched(steps, dev):
    from diffassemble_amd import Schedule
    from oracle import diffusion as ODF
    cpu = ODF.make_schedule(steps)
    return Schedule(cpu, dev), cpu["alphas_cumprod"]


def _engine(sd, prec, dev, variant="discrete_rot"):
    from diffassemble_amd import DenoiserEngine
    return DenoiserEngine(sd, variant=variant, arch="transformer", precision=prec, device=dev)


def _seed(dev, seed, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


# ---------------------------------------------------------------------------------------- 1. the step kernel alone
@pytest.mark.parametrize("K", [2, 35, 36, 1024])
def test_step_kernel(K, dev):
    from diffassemble_amd import engine as E
    n, steps, ratio = 130, 600, 10
    sch, ac = _sched(steps, dev)
    gen = torch.Generator().manual_seed(2000 + K)
    logits, rl = 3.0 * torch.randn(n, K, generator=gen), 3.0 * torch.randn(n, 4, generator=gen)
    x_t, r_t = torch.randint(0, K, (n,), generator=gen), torch.randint(0, 4, (n,), generator=gen)
    u, ur = torch.rand(n, K, generator=gen), torch.rand(n, 4, generator=gen)
    t = torch.tensor([0, ratio, 590, 337, 20, 599, 0, 100, ratio, 250] * (n // 10))
    to = lambda *xs: [x.to(dev) for x in xs]      # noqa: E731
    xp, r0, rp, post, rpost = E.d3pm_rot_step(sch, *to(x_t, r_t, logits, rl, t), ratio, noise_x=u.to(dev), noise_rot=ur.to(dev),
                                              return_post=True)
    s = RC.rot_step(ac, x_t, r_t, logits, rl, t, ratio, u, ur)
    for got, ref, what in ((post, s["post_x"], "post_x"), (rpost, s["post_rot"], "post_rot")):
        err = float((got.double().cpu() - ref).abs().max())
        print(f"K={K}: {what} max abs err {err:.3e}, max |post| {float(ref.abs().max()):.3f}")
        assert err <= RTOL32 * float(ref.abs().max())
    DC.check_argmax(xp, s["x_prev"], s["gap_x"], f"K={K} x")
    DC.check_argmax(rp, s["rot_prev"], s["gap_rot"], f"K={K} rot")
    DC.check_argmax(r0, s["rot_0"], s["gap_rot0"], f"K={K} rot_0")
    assert torch.equal(xp.cpu()[t == 0], logits.argmax(-1)[t == 0]) and torch.equal(rp.cpu()[t == 0], rl.argmax(-1)[t == 0])
    # the position half is da_d3pm_step, bit for bit
    x_only, post_only = E.d3pm_step(sch, x_t.to(dev), logits.to(dev), t.to(dev), ratio, noise=u.to(dev), return_post=True)
    assert torch.equal(x_only, xp) and torch.equal(post_only, post)
    # a scalar t (the loop's form) gives the rows the per-node form gives
    a = E.d3pm_rot_step(sch, *to(x_t, r_t, logits, rl), 590, ratio, noise_x=u.to(dev), noise_rot=ur.to(dev))
    b = E.d3pm_rot_step(sch, *to(x_t, r_t, logits, rl, torch.full((n,), 590)), ratio, noise_x=u.to(dev), noise_rot=ur.to(dev))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_rotation_half_is_the_position_step_at_four_classes(dev):
    """Both posteriors of da_d3pm_rot_step are one device routine (d3pm_categorical): da_d3pm_step at K = 4 on the rotation half's
    rows and injected uniforms gives its rot_prev and post_rot bit for bit.  n = 9: a full workgroup and a one-row one; t mixes 0, the
    ratio and large values."""
    from diffassemble_amd import engine as E
    n, K, steps, ratio = 9, 7, 600, 10
    sch, _ = _sched(steps, dev)
    gen = torch.Generator().manual_seed(4004)
    logits, rl = (3.0 * torch.randn(n, K, generator=gen)).to(dev), (3.0 * torch.randn(n, 4, generator=gen)).to(dev)
    x_t, r_t = torch.randint(0, K, (n,), generator=gen).to(dev), torch.randint(0, 4, (n,), generator=gen).to(dev)
    u, ur = torch.rand(n, K, generator=gen).to(dev), torch.rand(n, 4, generator=gen).to(dev)
    t = torch.tensor([0, ratio, 590, 337, 0, 599, ratio, 20, 0], device=dev)
    _, _, rp, _, rpost = E.d3pm_rot_step(sch, x_t, r_t, logits, rl, t, ratio, noise_x=u, noise_rot=ur, return_post=True)
    r4, post4 = E.d3pm_step(sch, r_t, rl, t, ratio, noise=ur, return_post=True)
    assert torch.equal(r4, rp) and torch.equal(post4, rpost)
    assert 0 <= int(rp.min()) and int(rp.max()) < 4 and bool(torch.isfinite(rpost).all())


# ---------------------------------------------------------------------------------------- 2. the generator
def test_rotation_draw_domain(dev):
    from diffassemble_amd import engine as E
    s = _seed(dev, 0x1234567890ABCDE, 7)
    n = 4096
    ur = E.d3pm_noise(s, 3, n, 4, domain="sampling_rot")
    assert ur.shape == (n, 4) and float(ur.min()) > 0.0 and float(ur.max()) <= 1.0
    assert torch.equal(ur, E.d3pm_noise(s, 3, n, 4, domain="sampling_rot"))
    assert abs(float(ur.double().mean()) - 0.5) < 6 * 0.2887 / (4 * n) ** 0.5
    # another stream than the position domain's (and the training domain's) at the same seed, iteration and flat element
    for other in ("sampling", "training"):
        assert float((E.d3pm_noise(s, 3, n, 4, domain=other) != ur).float().mean()) > 0.99
    assert float((E.d3pm_noise(s, 4, n, 4, domain="sampling_rot") != ur).float().mean()) > 0.99
    # the position domain is da_d3pm_noise, bit for bit
    assert torch.equal(E.d3pm_noise(s, 3, 64, 144, domain="sampling"), E.d3pm_noise(s, 3, 64, 144))
    # the step draws exactly these numbers when no noise buffer is given: position uniforms [n, K], rotation uniforms [n, 4]
    sch, _ = _sched(600, dev)
    gen = torch.Generator().manual_seed(5)
    n, K = 130, 36
    logits, rl = (3.0 * torch.randn(n, K, generator=gen)).to(dev), (3.0 * torch.randn(n, 4, generator=gen)).to(dev)
    x_t, r_t = torch.randint(0, K, (n,), generator=gen).to(dev), torch.randint(0, 4, (n,), generator=gen).to(dev)
    t = torch.tensor([0, 10, 590, 337, 20] * (n // 5), device=dev)
    own = E.d3pm_rot_step(sch, x_t, r_t, logits, rl, t, 10, seed=s, iteration=11)
    inj = E.d3pm_rot_step(sch, x_t, r_t, logits, rl, t, 10, noise_x=E.d3pm_noise(s, 11, n, K),
                          noise_rot=E.d3pm_noise(s, 11, n, 4, domain="sampling_rot"))
    assert all(torch.equal(p, q) for p, q in zip(own, inj))
    other = E.d3pm_rot_step(sch, x_t, r_t, logits, rl, t, 10, seed=s, iteration=12)
    assert not torch.equal(own[0], other[0]) and not torch.equal(own[2], other[2])


# ---------------------------------------------------------------------------------------- 3. forward
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_against_reference(prec, g9, case, dev):
    eng = _engine(case["sd"], prec, dev)
    assert (eng.flags & 3) == 1 and eng.flags & 8          # mlp.2 composed into its consumers; NO folded last layer; hoisted mlp.0
    plan = eng.plan(case["edge_index"], case["batch"])
    assert plan.dense == 1
    feats4 = case["feats4"].to(dev)
    tol = RTOL32 if prec == "fp32" else RTOLBF
    for t in V["fwd_t"]:
        idx, acc = torch.from_numpy(g9[f"fwd/t{t}/idx"]).to(dev), torch.from_numpy(g9[f"fwd/t{t}/rot_acc"]).to(dev)
        lo, rl = eng.forward_rot(plan, idx, torch.full((N,), t, dtype=torch.long, device=dev), feats4, rot_acc=acc)
        e, er = rel(lo, g9[f"fwd/t{t}/logits"]), rel(rl, g9[f"fwd/t{t}/rot_logits"])
        print(f"forward_rot {prec} t={t}: rel err logits {e:.3e}, rot_logits {er:.3e}")
        assert lo.shape == (N, V["K"]) and rl.shape == (N, 4) and e < tol and er < tol
        lo2, rl2 = eng.forward_rot(plan, idx, t, None, rot_acc=acc)                      # scalar t, staged images
        assert torch.equal(lo, lo2) and torch.equal(rl, rl2)
    # a wrong addend row shows: image 0 for every piece is another result, and it is what rot_acc = None selects
    z0, r0 = eng.forward_rot(plan, idx, t, None, rot_acc=None)
    z1, r1 = eng.forward_rot(plan, idx, t, None, rot_acc=torch.zeros_like(acc))
    assert torch.equal(z0, z1) and torch.equal(r0, r1) and rel(z0, lo) > 10 * tol
    # [N, F] features stage image 0 four times: every rot_acc selects the same row
    za, _ = eng.forward_rot(plan, idx, t, case["feats4"][0].to(dev), rot_acc=acc)
    assert torch.equal(za, z0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_k35_incomplete_graphs(prec, dev):
    K, steps, sizes = 35, 50, (20, 35)
    sd = RC.make_rot_state(K, steps, seed=35)
    rng = np.random.default_rng(35)
    ei, batch = W.collate([W.random_regular_edge_index(n, 6, rng) for n in sizes], sizes)
    n = sum(sizes)
    assert n % 8 != 0
    feats4 = RC.feature_images(n, 36)
    gen = torch.Generator().manual_seed(37)
    idx, acc, t = torch.randint(0, K, (n,), generator=gen), torch.randint(0, 4, (n,), generator=gen), torch.randint(0, steps, (n,), generator=gen)
    eng = _engine(sd, prec, dev)
    plan = eng.plan(ei, batch)
    assert plan.dense == 0
    lo, rl = eng.forward_rot(plan, idx.to(dev), t.to(dev), feats4.to(dev), rot_acc=acc.to(dev))
    ref_lo, ref_rl = RC.forward_with_feats(sd, idx, t, ei, RC.select_feats(feats4, acc))
    e, er = rel(lo, ref_lo), rel(rl, ref_rl)
    print(f"forward_rot {prec} K=35 CSR: rel err logits {e:.3e}, rot_logits {er:.3e}")
    tol = RTOL32 if prec == "fp32" else RTOLBF
    assert lo.shape == (n, K) and rl.shape == (n, 4) and e < tol and er < tol


# ---------------------------------------------------------------------------------------- 4. teacher-forced reference parity
def _module(case, dev, **kw):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete_rot import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=V["steps"], inference_ratio=V["ratio"], sampling="DDPM",
                      scheduler=SD.ModelScheduler.LINEAR, **kw)
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected and all(k.startswith(("visual_backbone", "mean", "std")) for k in missing)
    m.model.precision = "fp32"
    return m.to(dev).eval()


@pytest.mark.parametrize("cold,only_rot", V["modes"], ids=[RC.MODE_NAME[m] for m in V["modes"]])
def test_teacher_forced_against_the_reference_loop(cold, only_rot, g9, case, dev):
    p = f"loop/{RC.MODE_NAME[(cold, only_rot)]}/"
    m = _module(case, dev, cold_diffusion=cold, only_rotation=only_rot)
    ac = m.alphas_cumprod.cpu()
    ei, batch, feats4 = case["edge_index"].to(dev), case["batch"].to(dev), case["feats4"].to(dev)
    ld = lambda k: torch.from_numpy(g9[p + k])      # noqa: E731
    ins, u_x, u_rot = [ld("in_" + k) for k in ("index", "rot", "rot_acc")], ld("u_x"), ld("u_rot")
    got = {k: [] for k in ("x_prev", "rot_0", "rot_prev", "rot_acc")}
    gap = {k: [] for k in got}
    for it, i in enumerate(T_OF):
        idx, rot, acc = (x[it] for x in ins)                                  # teacher forcing: the reference's own input state
        t = torch.full((N,), i, dtype=torch.long)
        xp, r0, rp = m.p_sample_ddpm(idx.to(dev), rot.to(dev), t.to(dev), i, None, ei, feats4, batch, rot_acc=acc.to(dev),
                                     noise=u_x[it].to(dev), noise_rot=u_rot[it].to(dev))
        lo, rl = RC.forward_with_feats(case["sd"], idx, t, case["edge_index"], RC.select_feats(case["feats4"], acc))
        s = RC.rot_step(ac, idx, rot, lo, rl, t, V["ratio"], u_x[it], u_rot[it])
        for k, v, g in (("x_prev", xp, "gap_x"), ("rot_0", r0, "gap_rot0"), ("rot_prev", rp, "gap_rot")):
            got[k].append(v.cpu())
            gap[k].append(s[g])
        got["rot_acc"].append((acc + (rp if cold else r0).cpu()) % 4)         # the loop's state update on the kernel's outputs
        gap["rot_acc"].append(s["gap_rot" if cold else "gap_rot0"])
    assert got["x_prev"][0].dtype == torch.int64
    for k, ref in (("x_prev", "x_prev"), ("rot_0", "rot_0"), ("rot_prev", "rot_prev"), ("rot_acc", "traj_rot_acc")):
        DC.check_argmax(torch.cat(got[k]), ld(ref).flatten(), torch.cat(gap[k]), p + k)      # near ties counted over the whole trajectory
    assert torch.equal(ld("traj_index"), ld("x_prev"))


# ---------------------------------------------------------------------------------------- 5. the captured loop
def _eager_loop(eng, plan, sch, x0, r0, feats4, noise_x, noise_rot, cold, x_fixed, n_iters):
    x, rot, acc = x0.long(), r0.long(), torch.zeros_like(r0).long()
    tx, ta = [], []
    for it, i in enumerate(T_OF[:n_iters]):
        xin = x_fixed.long() if x_fixed is not None else x
        lo, rl = eng.forward_rot(plan, xin, i, feats4 if it == 0 else None, rot_acc=acc)
        x, rot_0, rot_prev = eng.d3pm_rot_step(sch, xin, rot, lo, rl, i, V["ratio"], noise_x=noise_x[it], noise_rot=noise_rot[it])
        rot = rot_prev if cold else rot_0
        acc = (acc + rot) % 4
        tx.append(x)
        ta.append(acc)
    return torch.stack(tx), torch.stack(ta)


@pytest.mark.parametrize("fixed", [False, True], ids=["free", "x_fixed"])
@pytest.mark.parametrize("cold", [False, True], ids=["rot0", "cold"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_loop_equals_the_eager_steps(prec, cold, fixed, g9, case, dev):
    eng = _engine(case["sd"], prec, dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    feats4 = case["feats4"].to(dev)
    p = "loop/cold/"
    x0, r0 = torch.from_numpy(g9[p + "x_init"]).to(dev), torch.from_numpy(g9[p + "rot_init"]).to(dev)
    nx, nr = torch.from_numpy(g9[p + "u_x"]).to(dev), torch.from_numpy(g9[p + "u_rot"]).to(dev)
    xf = torch.from_numpy(g9["loop/x_start"]).to(dev) if fixed else None
    kw = dict(ratio=V["ratio"], cold=cold, x_fixed=xf, noise_x=nx, noise_rot=nr)
    tx, ta, fx, fa = (x.clone() for x in eng.sample_loop_rot(plan, sch, x0, r0, feats4, use_graph=True, **kw))
    assert tx.shape == ta.shape == (N_IT, N) and tx.dtype == ta.dtype == torch.int32
    assert torch.equal(tx[-1], fx) and torch.equal(ta[-1], fa)
    assert int(tx.min()) >= 0 and int(tx.max()) < V["K"] and int(ta.min()) >= 0 and int(ta.max()) < 4
    ex, ea = _eager_loop(eng, plan, sch, x0, r0, feats4, nx, nr, cold, xf, N_IT)
    assert torch.equal(tx.long(), ex) and torch.equal(ta.long(), ea)
    assert len(set(ta.flatten().tolist())) == 4            # the trajectory visits every feature image
    # a replay of the cached graph, and the same loop without a graph
    again = eng.sample_loop_rot(plan, sch, x0, r0, feats4, use_graph=True, **kw)
    assert torch.equal(again[0], tx) and torch.equal(again[1], ta)
    plain = eng.sample_loop_rot(plan, sch, x0, r0, feats4, use_graph=False, **kw)
    assert torch.equal(plain[0], tx) and torch.equal(plain[1], ta)
    # without trajectories the state lives in the workspace: the same final state
    last = eng.sample_loop_rot(plan, sch, x0, r0, feats4, use_graph=True, keep_traj=False, **kw)
    assert last[0] is None and torch.equal(last[2], fx) and torch.equal(last[3], fa)


def test_loop_seed_and_truncation(g9, case, dev):
    eng = _engine(case["sd"], "bf16", dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    feats4 = case["feats4"].to(dev)
    x0, r0 = torch.from_numpy(g9["loop/cold/x_init"]).to(dev), torch.from_numpy(g9["loop/cold/rot_init"]).to(dev)
    kw = dict(ratio=V["ratio"], use_graph=True, cold=True)
    run = lambda s, **k: [x if x is None else x.clone() for x in eng.sample_loop_rot(plan, sch, x0, r0, feats4,      # noqa: E731
                                                                                      generator=torch.Generator().manual_seed(s), **kw, **k)]
    a, b, c = run(11), run(11), run(12)          # b, c replay the graph a recorded: the kernels read the rewritten seed
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # the same draws through the stand-alone step reproduce the first iteration
    eng.seed_tensor(generator=torch.Generator().manual_seed(11))
    lo, rl = eng.forward_rot(plan, x0, 95, None, rot_acc=None)
    xp, _, rp = eng.d3pm_rot_step(sch, x0, r0, lo, rl, 95, V["ratio"], seed=eng._seed, iteration=0)
    assert torch.equal(xp, a[0][0].long()) and torch.equal(rp % 4, a[1][0].long())
    # max_iters truncates as in da_sample_loop_idx
    short = run(11, max_iters=3)
    assert short[0].shape == (3, N) and torch.equal(short[0], a[0][:3]) and torch.equal(short[1], a[1][:3])
    assert torch.equal(short[2], a[0][2]) and torch.equal(short[3], a[1][2])


# ---------------------------------------------------------------------------------------- 6. the module
def _batch(case, dev, indexes, rot_index):
    return types.SimpleNamespace(indexes=indexes.to(dev), rot_index=rot_index.to(dev), patches=None, edge_index=case["edge_index"].to(dev),
                                 batch=case["batch"].to(dev), patches_dim=torch.tensor([[6, 6], [6, 6]], device=dev),
                                 patch_feats=case["feats4"].to(dev))


def _rig(m, c, rc):
    """logits = 50 one_hot(c), rot logits = 50 one_hot(rc) for every piece: positions end at c; rot_0 = rc at each of the 20 steps, so
    rot_acc walks rc, 2 rc, ... and ends at 20 rc % 4 = 0."""
    with torch.no_grad():
        m.model.final_mlp[2].weight.zero_()
        m.model.final_mlp[2].bias.copy_(50.0 * torch.nn.functional.one_hot(torch.tensor(c), 36).float())
        m.model.final_mlp_rot[2].weight.zero_()
        m.model.final_mlp_rot[2].bias.copy_(50.0 * torch.nn.functional.one_hot(torch.tensor(rc), 4).float())


def test_module_sampling_and_validation(case, dev):
    from diffassemble_amd import _lib
    m = _module(case, dev)
    imgs = m.p_sample_loop((N,), None, case["edge_index"].to(dev), case["batch"].to(dev), patch_feats=case["feats4"].to(dev))
    assert len(imgs) == 20 and all(len(pr) == 2 and all(x.dtype == torch.int64 and x.shape == (N,) for x in pr) for pr in imgs)
    assert all(0 <= int(x.min()) and int(x.max()) < 36 and 0 <= int(r.min()) and int(r.max()) < 4 for x, r in imgs)
    z = torch.zeros(N, dtype=torch.long)
    assert len(m.predict_step(_batch(case, dev, z, z), 0)) == 20
    c, rc = 17, 1
    _rig(m, c, rc)
    traj = m.p_sample_loop((N,), None, case["edge_index"].to(dev), case["batch"].to(dev), patch_feats=case["feats4"].to(dev))
    assert [int(r[0]) for _, r in traj[:5]] == [1, 2, 3, 0, 1] and all(bool((r == r[0]).all()) for _, r in traj)
    # every position right; puzzle 0 has every rotation right (mod 4), puzzle 1 one piece wrong: only puzzle 0 counts
    gt_rot = 4 * torch.arange(N)
    gt_rot[40] += 1
    m.initialize_torchmetrics([(6, 6)])
    pred, pred_rot = m.validation_step(_batch(case, dev, c + 36 * torch.arange(N), gt_rot), 0)
    assert torch.equal(pred.cpu(), torch.full((N,), c)) and torch.equal(pred_rot.cpu(), torch.zeros(N, dtype=torch.long))
    assert float(m.metrics["overall_acc"].compute()) == 0.5 and float(m.metrics["overall__piece_acc"].compute()) == pytest.approx(1 - 1 / N)
    assert float(m.metrics["overall_nImages"].compute()) == 2.0 and float(m.metrics["(6, 6)_nImages"].compute()) == 2.0
    # every rotation right, one position wrong in puzzle 0: that puzzle does not count ...
    gt_idx = c + 36 * torch.arange(N)
    gt_idx[3] += 1
    m.initialize_torchmetrics([(6, 6)])
    m.test_step(_batch(case, dev, gt_idx, 4 * torch.arange(N)), 0)
    assert float(m.metrics["overall_acc"].compute()) == 0.5
    # ... unless only the rotations are asked for (the loop then starts every step from the given indices)
    mo = _module(case, dev, only_rotation=True)
    _rig(mo, c, rc)
    mo.initialize_torchmetrics([(6, 6)])
    mo.validation_step(_batch(case, dev, torch.arange(N)[torch.randperm(N, generator=torch.Generator().manual_seed(1))], 4 * torch.arange(N)), 0)
    assert float(mo.metrics["overall_acc"].compute()) == 1.0 and float(mo.metrics["overall__piece_acc"].compute()) == 1.0
    # the entries of the other variants reject this engine (nothing is launched), and the rot entries reject the position engine
    eng = m.model.engine(dev)
    plan = eng.plan(case["edge_index"], case["batch"])
    sch, _ = _sched(V["steps"], dev)
    f0 = case["feats4"][0].to(dev)
    with pytest.raises(_lib.DaError, match="da_denoiser_forward_rot"):
        eng.forward(plan, torch.zeros(N, 1, device=dev), 0, None)
    with pytest.raises(_lib.DaError, match="da_denoiser_forward_rot"):
        eng.forward_idx(plan, z.to(dev), 0, None)
    with pytest.raises(_lib.DaError, match="da_sample_loop_rot"):
        eng.sample_loop_idx(plan, sch, z.to(dev), f0, ratio=5, restage=False)
    with pytest.raises(_lib.DaError, match="da_sample_loop_rot"):
        eng.sample_loop(plan, sch, torch.zeros(N, 1, device=dev), f0, ratio=5, restage=False)
    pos = _engine(DC.v7_case()["sd"], "bf16", dev, variant="discrete")
    with pytest.raises(_lib.DaError, match="not a discrete rot denoiser"):
        pos.forward_rot(pos.plan(case["edge_index"], case["batch"]), z.to(dev), 0, case["feats4"].to(dev))


# ---------------------------------------------------------------------------------------- 7. the position model is what it was
def test_position_loop_still_equals_its_eager_steps(dev):
    c7, g7 = DC.v7_case(), DC.load_golden7()
    eng = _engine(c7["sd"], "bf16", dev, variant="discrete")
    assert (eng.flags & 3) == 3
    plan = eng.plan(c7["edge_index"], c7["batch"])
    sch, _ = _sched(DC.V7["steps"], dev)
    feats = c7["feats"].to(dev)
    x0, noise = torch.from_numpy(g7["loop/x_init"]).to(dev), torch.from_numpy(g7["loop/uniforms"]).to(dev)
    traj = eng.sample_loop_idx(plan, sch, x0, feats, ratio=DC.V7["ratio"], use_graph=True, noise=noise)[0].clone()
    x, eager = x0, []
    for it, i in enumerate(reversed(range(0, DC.V7["steps"], DC.V7["ratio"]))):
        x = eng.d3pm_step(sch, x, eng.forward_idx(plan, x, i, feats), i, DC.V7["ratio"], noise=noise[it])
        eager.append(x)
    assert torch.equal(traj.long(), torch.stack(eager))
