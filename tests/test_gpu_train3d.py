"""GPU tests of the 3D training step: the pose head's backward and the SE(3) noising on their own, the 3D denoiser's
forward + backward against the oracle's autograd, p_losses against the reference's own step (golden_v6.npz,
make_golden_v6.py), the encoder chain and one full optimizer step.

Bounds.  The per-piece fp32 kernels (da_head3d_backward, da_q_sample_se3) follow the rule of test_gpu_loss3d.py: at most 4x
the error of the same expression evaluated by torch in fp32 against fp64, in max-abs terms scaled by the largest element,
floored at 16 fp32 ulps of unit scale.  The denoiser backward keeps test_gpu_train.py's bounds (output 1e-4, gradients
GTOL = 1e-3 with the 1e-4 x max floor), the fixture comparison test_gpu_gcn.py's (fp32) and test_gpu_train.py's documented
bf16-mode bound."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_cases as GC
import train3d_cases as T3
from oracle import denoiser as OD
from oracle import so3
from oracle import weights as W
from oracle.pyg_restatement import matrix_to_quaternion, quaternion_to_matrix

pytestmark = pytest.mark.gpu
GTOL = 1e-3
ULP16 = 16 * 2.0 ** -23


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden6():
    return T3.load_golden6()


def within_4x(name, hip, f32, f64):
    scale = float(f64.abs().max())
    e32 = float((f32.double() - f64).abs().max()) / scale
    ehip = float((hip.double().cpu() - f64).abs().max()) / scale
    print(f"{name}: scale {scale:.3e}  torch-fp32 err {e32:.3e}  HIP err {ehip:.3e}")
    assert math.isfinite(ehip) and ehip <= max(4 * e32, ULP16), (name, e32, ehip)
    return e32, ehip


# ------------------------------------------------------------------------------------------------ da_head3d_backward
SPECIAL_NORMS = (0.0, 1e-6, 9e-5, 1.1e-4, 3.0, 3.3, 4.0, 6.0)      # r = 0, both sides of the series switch, across the sign change of w


def head_rows(n, seed=5):
    """pre [n, 6] = [r | t]: the special norms first, then |r| <= 2 at random; |w| = |cos(|r| / 2)| >= 1e-3 by construction."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    norms = rng.uniform(0.05, 2.0, n)
    norms[: min(n, len(SPECIAL_NORMS))] = SPECIAL_NORMS[: min(n, len(SPECIAL_NORMS))]
    assert np.abs(np.cos(norms / 2)).min() >= 1e-3
    r = torch.from_numpy((d * norms[:, None]).astype(np.float32))
    t = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((n, 7)).astype(np.float32))
    return torch.cat([r, t], 1), g


def head_autograd(pre, g, dtype):
    p = pre.to(dtype).requires_grad_(True)
    q = F.normalize(matrix_to_quaternion(so3.skew_to_rmat(p[:, :3])), p=2, dim=-1)
    out = torch.hstack((q, p[:, 3:]))
    (out * g.to(dtype)).sum().backward()
    return p.grad.detach(), out.detach()


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_head3d_backward_against_fp64_autograd(dev, n):
    from diffassemble_amd import _lib
    pre, g = head_rows(n)
    g64, out64 = head_autograd(pre, g, torch.float64)
    g32, _ = head_autograd(pre, g, torch.float32)
    assert float(out64[:, 0].abs().min()) >= 1e-3
    d_pre = torch.full((n, 6), float("nan"), device=dev)
    pre_d, g_d = pre.to(dev), g.to(dev)
    _lib.check(_lib.lib().da_head3d_backward(n, _lib.ptr(pre_d), _lib.ptr(g_d), _lib.ptr(d_pre), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert torch.equal(d_pre[:, 3:].cpu(), g[:, 4:])                  # the translation passes straight through
    within_4x(f"head3d backward n={n}", d_pre, g32, g64)
    k = min(n, len(SPECIAL_NORMS))
    within_4x(f"head3d backward n={n}, special rows", d_pre[:k], g32[:k], g64[:k])


# ------------------------------------------------------------------------------------------------ da_q_sample_se3
def schedule_3d(steps=T3.STEPS):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    return GNN_Diffusion(steps=steps, sampling="DDIM", backbone="vn_dgcnn", max_num_part=T3.MAX_PARTS, model_mean_type=ModelMeanType.START_X)


_TRAP = {}


def trap_table(m):
    from diffassemble_amd.engine import igso3_trap_table
    if m.steps not in _TRAP:
        _TRAP[m.steps] = igso3_trap_table(m.sqrt_one_minus_alphas_cumprod)
    return _TRAP[m.steps]


def noising_restatement(m, x_start, t, noise_tr, axes, unif, dtype):
    """p_losses :421-441 + IsotropicGaussianSO3.sample (distributions.py:507-526) on the fp32 CDF table, arithmetic in ``dtype``.
    The reference gathers trap_start / trap_end from the FIRST piece's column (index [P, 1] along dim 0 of a [999, P] table)."""
    trap = trap_table(m)
    sac, somac = m.sqrt_alphas_cumprod.to(dtype), m.sqrt_one_minus_alphas_cumprod.to(dtype)
    x = x_start.to(dtype)
    tr = sac[t, None] * x[:, 4:] + somac[t, None] * noise_tr.to(dtype)
    idx1 = (trap[t] <= unif[:, None]).sum(1).clamp(max=998)
    idx0 = (idx1 - 1).clamp(min=0)
    row0 = trap[t[0]].to(dtype)
    ts, te = row0[idx0], row0[idx1]
    wgt = ((unif.to(dtype) - ts) / (te - ts).clamp(min=1e-6)).clamp(0, 1)
    loc = (math.pi * torch.linspace(0, 1.0, 1000) ** 3.0)[1:].to(dtype)
    ang = torch.lerp(loc[idx0], loc[idx1], wgt)
    a = axes.to(dtype)
    a = a / a.norm(dim=-1, keepdim=True)
    noise = torch.matrix_exp(so3.vec2skew(a * ang[:, None]))
    rot = so3.so3_scale(quaternion_to_matrix(x[:, :4]), sac[t]) @ noise
    return torch.cat([matrix_to_quaternion(rot), tr], 1)


def run_noising(m, dev, x_start, t, noise_tr, axes, unif):
    m = m.to(dev)
    out = m.q_sample_se3(x_start.to(dev), t.to(dev), (noise_tr.to(dev), axes.to(dev), unif.to(dev)))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("spec", T3.TRAIN3D, ids=lambda s: s["name"])
def test_q_sample_se3_reproduces_the_reference_noising(dev, golden6, spec):
    case = T3.build_case(spec)
    name = spec["name"]
    t = torch.from_numpy(golden6[f"{name}/t"])
    assert torch.equal(t, case["t"])
    draws = [torch.from_numpy(golden6[f"{name}/{k}"]) for k in ("noise_tr", "axes", "unif")]
    want = torch.from_numpy(golden6[f"{name}/x_noisy"])
    assert float(want[:, 0].abs().min()) >= T3.W_MIN
    m = schedule_3d()
    f64 = noising_restatement(m, case["x_start"], t, *draws, torch.float64)
    f32 = noising_restatement(m, case["x_start"], t, *draws, torch.float32)
    got = run_noising(m, dev, case["x_start"], t, *draws)
    e32, _ = within_4x(f"{name} x_noisy", got, f32, f64)
    # the reference's own fp32 result is one more fp32 evaluation of the expression: it validates the restatement
    eref = float((want.double() - f64).abs().max()) / float(f64.abs().max())
    print(f"{name}: reference fixture vs fp64 restatement {eref:.3e}")
    assert eref <= max(4 * e32, ULP16)


@pytest.mark.parametrize("n", [1, 65])
def test_q_sample_se3_edge_rows(dev, n):
    """unif in {0, just below the first positive CDF entry, 1 - 2^-24, exactly 1.0 (clamps, must not fault)}, t in {0, steps - 1},
    identity and random x_start rotations."""
    m = schedule_3d()
    trap = trap_table(m)
    rng = np.random.default_rng(9)
    rows = []
    for t in (0, m.steps - 1):
        first = trap[t][trap[t] > 0][0]
        for u in (0.0, float(torch.nextafter(first, torch.tensor(0.0))), 1.0 - 2.0 ** -24, 1.0):
            for ident in (True, False):
                rows.append((t, u, ident))
    rows = [rows[i % len(rows)] for i in range(n)] if n > 1 else [rows[7]]           # n = 1: (t = 0, u = 1.0, random rotation)
    t = torch.tensor([r[0] for r in rows])
    unif = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    assert float(unif.max()) == 1.0
    q = T3.unit_quaternions(rng, n)
    for i, r in enumerate(rows):
        if r[2]:
            q[i] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    x_start = torch.cat([q, torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))], 1)
    noise_tr = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    axes = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    f64 = noising_restatement(m, x_start, t, noise_tr, axes, unif, torch.float64)
    f32 = noising_restatement(m, x_start, t, noise_tr, axes, unif, torch.float32)
    keep = f64[:, 0].abs() >= T3.W_MIN                                 # (a row whose w is rounding's to sign is compared up to that sign)
    got = run_noising(m, dev, x_start, t, noise_tr, axes, unif)
    assert bool(torch.isfinite(got).all())
    assert float((got[:, :4].norm(dim=1) - 1).abs().max()) < 1e-5
    flip = torch.where(keep, torch.ones(n), torch.sign((got[:, :4].double() * f64[:, :4]).sum(1)).float())
    got = torch.cat([got[:, :4] * flip[:, None], got[:, 4:]], 1)
    f32f = torch.cat([f32[:, :4] * torch.where(keep, torch.ones(n), torch.sign((f32[:, :4].double() * f64[:, :4]).sum(1)).float())[:, None], f32[:, 4:]], 1)
    within_4x(f"edge rows n={n}", got, f32f, f64)


# ------------------------------------------------------------------------------------------------ denoiser backward
BATCHES = {"p2_5_20": (2, 5, 20), "p20x5_7": (20, 20, 20, 20, 20, 7)}
_ORACLE = {}


KINK_MARGIN = 5e-6      # smallest |pre-activation| of the two LeakyReLUs a case may have: ~7x the fp32 error of evaluating them (7e-7)


def leaky_margin(sd, x, t, feats):
    """min |pre-activation| over the two LeakyReLU(0.2) layers of the 3D mlp, in fp64.  The derivative jumps from 0.2 to 1 at 0: an
    element closer to 0 than the fp32 evaluation error takes either slope depending on the summation order, in torch as in HIP, and
    moves whole gradient rows by O(1) of that element -- a condition on the inputs, like |w| >= 1e-3 on the quaternions."""
    s = {k: v.double() for k, v in sd.items()}
    pos = F.linear(F.gelu(F.linear(x.double(), s["pos_mlp.0.weight"], s["pos_mlp.0.bias"])), s["pos_mlp.2.weight"], s["pos_mlp.2.bias"])
    comb = torch.cat([feats.double(), pos, s["time_emb.weight"][t]], -1)
    h = F.linear(comb, s["mlp.0.weight"], s["mlp.0.bias"])
    o = F.linear(F.leaky_relu(h, 0.2), s["mlp.2.weight"], s["mlp.2.bias"])
    return min(float(h.abs().min()), float(o.abs().min()))


def denoiser_case(arch, sizes_key, steps=50):
    """Inputs + the oracle's forward / autograd of one case: computed once, shared, never modified.  The seed is searched upwards
    until no LeakyReLU pre-activation lies within KINK_MARGIN of 0 (see leaky_margin)."""
    key = (arch, sizes_key)
    if key in _ORACLE:
        return _ORACLE[key]
    sizes = BATCHES[sizes_key]
    P = sum(sizes)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    base = 700 + 10 * (sorted(BATCHES).index(sizes_key) * 3 + ["transformer", "exophormer", "gcn"].index(arch))
    for seed in range(base, base + 10000, 100):
        sd = T3.make_state(arch, steps, seed)
        rng = np.random.default_rng(seed)
        _, feats = W.make_inputs(P, 7, T3.FEAT, seed)
        x = T3.poses(P, seed)
        t = torch.from_numpy(rng.integers(0, steps, size=len(sizes)))[batch]
        if leaky_margin(sd, x, t, feats) >= KINK_MARGIN:
            break
    assert leaky_margin(sd, x, t, feats) >= KINK_MARGIN
    functional = torch.from_numpy(rng.standard_normal((P, 7)).astype(np.float32))       # every output column carries gradient
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fg = feats.clone().requires_grad_(True)
    if arch == "gcn":
        pred = GC.forward_with_feats(sdg, x, t, edge_index, fg, variant="3d")
    else:
        pred, _ = OD.eff_gat_3d_forward_with_feats(sdg, x, t, edge_index, fg, batch, arch, T3.VIRT)
    (pred * functional).sum().backward()
    assert float(pred[:, 0].abs().min()) >= 1e-3
    _ORACLE[key] = dict(sd=sd, x=x, t=t, feats=feats, edge_index=edge_index, batch=batch, functional=functional, pred=pred.detach(),
                        grads={k: v.grad for k, v in sdg.items()}, d_feats=fg.grad)
    return _ORACLE[key]


def make_module(arch, sd, dev, steps=50, freeze=True):
    from diffassemble_amd.model.backbones import Eff_GAT_3d
    m = Eff_GAT_3d(steps=steps, architecture=arch, backbone="vn_dgcnn", n_layers=4, virt_nodes=T3.VIRT, freeze_backbone=freeze)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    return m.to(dev).train()


@pytest.mark.parametrize("sizes_key", sorted(BATCHES))
@pytest.mark.parametrize("arch", ["transformer", "exophormer", "gcn"])
def test_denoiser_backward_matches_oracle_autograd(dev, arch, sizes_key):
    c = denoiser_case(arch, sizes_key)
    m = make_module(arch, c["sd"], dev)
    feats = c["feats"].to(dev).requires_grad_(True)
    out, att = m.forward_with_feats(c["x"].to(dev), c["t"].to(dev), c["edge_index"].to(dev), feats, c["batch"].to(dev))
    assert att is None and out.requires_grad and out.shape == c["pred"].shape
    e_out = rel(out, c["pred"])
    print(f"{arch} {sizes_key}: output rel err {e_out:.3e}")
    assert e_out < 1e-4
    (out * c["functional"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    floor = 1e-4 * max(float(g.abs().max()) for g in c["grads"].values())
    errs = {}
    for k, gr in c["grads"].items():
        assert gr is not None and params[k].grad is not None, k
        errs[k] = float((params[k].grad.detach().double().cpu() - gr.double()).abs().max()) / max(float(gr.abs().max()), floor)
    e_f = rel(feats.grad, c["d_feats"])
    worst = max(errs.items(), key=lambda p: p[1])
    print(f"{arch} {sizes_key}: worst gradient {worst[0]} {worst[1]:.3e}; d_feats {e_f:.3e}; above GTOL / 10: "
          f"{ {k: round(e, 6) for k, e in errs.items() if e > GTOL / 10} }")
    assert all(e < GTOL for e in errs.values()), {k: e for k, e in errs.items() if e >= GTOL}
    assert e_f < GTOL
    te = m.train_engine()
    lo, hi = te.flat_grad.data_ptr(), te.flat_grad.data_ptr() + te.flat_grad.numel() * 4
    assert all(lo <= params[k].grad.data_ptr() < hi for k in c["grads"])
    assert all(p.grad is None for k, p in params.items() if k.startswith("pcd_backbone."))


# ------------------------------------------------------------------------------------------------ p_losses vs golden_v6
def diffusion_module(spec, case, dev, freeze=True, steps=T3.STEPS, max_parts=T3.MAX_PARTS):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=steps, sampling="DDIM", inference_ratio=1, noise_weight=0.0, model_mean_type=ModelMeanType.START_X,
                      backbone="vn_dgcnn", architecture=spec["arch"], max_num_part=max_parts, loss_type="all", freeze_backbone=freeze)
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected
    return m.to(dev).train()


def fixture_step(spec, case, golden6, dev, precision, staged=False):
    name = spec["name"]
    m = diffusion_module(spec, case, dev)
    te = m.model.train_engine(dev)
    te.precision = precision
    te.force_staged = staged
    noise = tuple(torch.from_numpy(golden6[f"{name}/{k}"]).to(dev) for k in ("noise_tr", "axes", "unif"))
    losses = m.p_losses(case["x_start"].to(dev), torch.from_numpy(golden6[f"{name}/t"]).to(dev), noise=noise, loss_type="all",
                        cond=case["pts"].to(dev), edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                        n_batch=len(T3.SIZES), valids=case["valids"].to(dev), pcd_feats=case["feats"].to(dev))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return m, losses


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("spec", T3.TRAIN3D, ids=lambda s: s["name"])
def test_p_losses_matches_the_reference_fixture(dev, golden6, spec, staged):
    """The reference's own 3D p_losses + backward: each entry of the loss dictionary, then every live gradient's first 64 entries
    and its (|g| sum, g^2 sum), with the tolerances test_gpu_gcn.py uses against golden_v5.npz."""
    name = spec["name"]
    case = T3.build_case(spec)
    assert float(np.abs(golden6[f"{name}/prediction"][:, 0]).min()) >= T3.W_MIN
    m, losses = fixture_step(spec, case, golden6, dev, "fp32", staged)
    assert list(losses) == ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss"]
    errs = {}
    for k, v in losses.items():
        ref = float(golden6[f"{name}/loss/{k}"])
        errs[k] = abs(float(v) - ref) / abs(ref) if ref != 0.0 else abs(float(v))
    print(f"{name}: loss entries rel err {errs}")
    assert all(e < 1e-5 for e in errs.values()), errs
    live = {k: p for k, p in m.model.named_parameters() if f"{name}/grad_head/{k}" in golden6.files}
    assert len(live) == len(case["sd"])
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in live.values())
    worst = [0.0, 0.0, 0.0]
    for k, p in live.items():
        ref = torch.from_numpy(golden6[f"{name}/grad_head/{k}"]).double()
        got = p.grad.flatten()[: ref.numel()].double().cpu()
        e0 = float((got - ref).abs().max()) / max(float(ref.abs().max()), floor)
        worst[0] = max(worst[0], e0)
        assert e0 < GTOL, (k, e0)
        g = p.grad.double().cpu()
        st, st_ref = torch.stack([g.sum(), g.abs().sum(), (g * g).sum()]), golden6[f"{name}/grad_stats/{k}"]
        if float(st_ref[1]) > floor * p.numel() * 1e-2:
            e1 = abs(float(st[1]) - float(st_ref[1])) / float(st_ref[1])
            e2 = abs(float(st[2]) - float(st_ref[2])) / float(st_ref[2])
            worst[1], worst[2] = max(worst[1], e1), max(worst[2], e2)
            assert e1 < GTOL and e2 < 2 * GTOL, (k, e1, e2)
    print(f"{name}: worst (head, |g| sum, g^2 sum) {worst}")


@pytest.mark.parametrize("spec", T3.TRAIN3D, ids=lambda s: s["name"])
def test_p_losses_in_the_bf16_mode_vs_the_reference_fixture(dev, golden6, spec):
    """The same fixture against the bf16-operand mode, with the bound test_gpu_train.py documents for it: loss 5e-3; per gradient
    tensor the first 64 entries within 2.5 % of the tensor's largest entry, |g| sum within 1.5 %, g^2 sum within 2 %."""
    name = spec["name"]
    case = T3.build_case(spec)
    m, losses = fixture_step(spec, case, golden6, dev, "bf16")
    errs = {}
    for k, v in losses.items():
        ref = float(golden6[f"{name}/loss/{k}"])
        errs[k] = abs(float(v) - ref) / abs(ref) if ref != 0.0 else abs(float(v))
    total, total_ref = float(sum(losses.values())), sum(float(golden6[f"{name}/loss/{k}"]) for k in losses)
    print(f"{name} bf16: loss entries rel err {errs}; total {abs(total - total_ref) / total_ref:.3e}")
    assert all(e < 5e-3 for e in errs.values()), errs
    live = {k: p for k, p in m.model.named_parameters() if f"{name}/grad_head/{k}" in golden6.files}
    floor = 1e-3 * max(float(p.grad.abs().max()) for p in live.values())
    worst, n = [0.0, 0.0, 0.0], 0
    for k, p in live.items():
        ref = torch.from_numpy(golden6[f"{name}/grad_head/{k}"]).double()
        got = p.grad.flatten()[: ref.numel()].double().cpu()
        st_ref = golden6[f"{name}/grad_stats/{k}"]
        if float(st_ref[1]) <= floor * p.numel() * 1e-1:
            continue                                                     # identically-zero gradients (lin_key.bias): rounding noise
        g = p.grad.double().cpu()
        e = [float((got - ref).abs().max()) / max(float(ref.abs().max()), float(p.grad.abs().max()), floor),
             abs(float(g.abs().sum()) - float(st_ref[1])) / float(st_ref[1]),
             abs(float((g * g).sum()) - float(st_ref[2])) / float(st_ref[2])]
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < 2.5e-2 and e[1] < 1.5e-2 and e[2] < 2e-2, (k, e)
        n += 1
    print(f"{name} bf16 mode vs reference fixture, worst (head, |g| sum, g^2 sum): {worst} over {n} tensors")
    assert n >= 12 and worst[0] > 1e-5


# ------------------------------------------------------------------------------------------------ encoder chain, full step
def small_batch(dev, sizes=(2, 5), n_points=64, n_parts=6, seed=44, steps=20):
    P = sum(sizes)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.integers(0, steps, size=len(sizes)))[batch]
    noise = (torch.from_numpy(rng.standard_normal((P, 3)).astype(np.float32)), torch.from_numpy(rng.standard_normal((P, 3)).astype(np.float32)),
             torch.from_numpy(rng.uniform(0.05, 0.95, P).astype(np.float32)))
    return SimpleNamespace(x=T3.poses(P, seed).to(dev), pcds=W.make_point_clouds(P, n_points, seed).to(dev), edge_index=edge_index.to(dev),
                           batch=batch.to(dev), valids=T3.valids_of(sizes, n_parts).to(dev), data_id=list(range(len(sizes))),
                           t=t.to(dev), noise=tuple(z.to(dev) for z in noise))


def test_encoder_gradients_flow_through_d_feats(dev):
    """Trainable vn_dgcnn, P = 7 (2 + 5), N = 64: the encoder gradients of p_losses().backward() equal those of calling the backbone
    alone and back-propagating the d_feats of the same step into it (the plumbing, not the encoder's accuracy); with
    freeze_backbone the encoder gets none."""
    spec = dict(name="chain", arch="transformer", seed=611)
    sd = T3.make_state("transformer", 20, 611)
    b = small_batch(dev)
    m = diffusion_module(spec, dict(sd=sd), dev, freeze=False, steps=20)
    kw = dict(loss_type="all", cond=b.pcds, edge_index=b.edge_index, batch=b.batch, n_batch=2, valids=b.valids)
    enc = m.model.pcd_backbone
    with pytest.raises(NotImplementedError):
        m.model.pcd_features(b.pcds)                      # the inference-side call still refuses a trainable backbone in train()
    losses = m.p_losses(b.x, b.t, noise=b.noise, **kw)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}
    assert got and all(bool(torch.isfinite(g).all()) for g in got.values()) and any(float(g.abs().max()) > 0 for g in got.values())
    m.zero_grad(set_to_none=True)
    feats = enc(b.pcds).detach().requires_grad_(True)
    losses2 = m.p_losses(b.x, b.t, noise=b.noise, pcd_feats=feats, **kw)
    sum(losses2.values()).backward()
    assert all(p.grad is None for p in enc.parameters())
    enc(b.pcds).backward(feats.grad)
    torch.cuda.synchronize()
    for k, p in enc.named_parameters():
        if p.grad is None:
            assert k not in got, k
            continue
        scale = max(float(p.grad.abs().max()), 1e-30)
        assert float((got[k] - p.grad).abs().max()) / scale <= 1e-6, k          # same kernels, same inputs: fp32 rounding at most
    frozen = diffusion_module(spec, dict(sd=sd), dev, freeze=True, steps=20)
    sum(frozen.p_losses(b.x, b.t, noise=b.noise, **kw).values()).backward()
    assert all(p.grad is None for p in frozen.model.pcd_backbone.parameters())
    assert frozen.model.time_emb.weight.grad is not None


@pytest.mark.parametrize("arch,freeze", [("transformer", True), ("exophormer", False), ("gcn", True)])
def test_one_full_training_step(dev, arch, freeze):
    """training_step -> configure_optimizers().step() -> p_sample_loop in eval(): the parameters moved, the packed inference engine
    was rebuilt (the sampled poses differ from the pre-step ones), everything is finite."""
    from diffassemble_amd.train import FusedAdafactor, HybridAdafactor
    spec = dict(name="step", arch=arch, seed=621)
    b = small_batch(dev)
    m = diffusion_module(spec, dict(sd=T3.make_state(arch, 20, 621)), dev, freeze=freeze, steps=20)
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v))
    m.eval()
    before = m.p_sample_loop(b.x.shape, b.pcds, b.edge_index, batch=b.batch)[0][-1].clone()
    m.train()
    opt = m.configure_optimizers()
    assert isinstance(opt, FusedAdafactor if freeze else HybridAdafactor)
    torch.manual_seed(3)
    loss = m.training_step(b, 1)
    loss.backward()
    te = m.model.train_engine(dev)
    flat0 = te.flat.clone()
    enc0 = [p.detach().clone() for p in m.model.pcd_backbone.parameters()]
    opt.step()
    torch.cuda.synchronize()
    assert set(logged) == {"trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss", "loss"}
    assert math.isfinite(float(loss)) and abs(logged["loss"] - float(loss)) < 1e-6 * max(1.0, abs(float(loss)))
    assert bool(torch.isfinite(te.flat).all()) and bool(torch.isfinite(te.flat_grad).all())
    assert not torch.equal(flat0, te.flat)
    moved = any(not torch.equal(a, p.detach()) for a, p in zip(enc0, m.model.pcd_backbone.parameters()))
    assert moved == (not freeze)
    m.eval()
    after = m.p_sample_loop(b.x.shape, b.pcds, b.edge_index, batch=b.batch)[0][-1]
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
