"""GPU tests of the 3D model with ``use_6dof=True``: ``da_rot6d_to_pose`` and its backward, the 9-channel pose-head backward and
SE(3) noising on their own, then the 13-channel forward, ``p_losses`` + backward, the sampling loop and the evaluation step against
the reference's own run (golden_v11.npz, make_golden_v11.py), one optimizer step per architecture and mode, and a guard that a
13-channel denoiser leaves a 7-channel one of the same process alone.

Bounds.  The per-piece fp32 kernels follow test_gpu_train3d.py's rule (``within_4x``: at most 4x the error of the same expression
evaluated by torch in fp32 against fp64, max-abs scaled by the largest element, floored at 16 fp32 ulps).  The forward keeps
test_gpu_parity.py's 1e-4 against the fixture, the trajectory its TRAJ32 = 5e-4 (quaternions up to sign), the fp32 step
test_p_losses_matches_the_reference_fixture's bounds (loss entries 1e-5, gradients GTOL = 1e-3 with the 1e-4 x max floor) and the
bf16 mode the bound that test documents; the metrics test_gpu_metrics3d.py's (``within_4x`` per column, part accuracy exact)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rot6d_refs as R6
import train3d_6dof_cases as T6
import train3d_cases as T3
from oracle import so3
from oracle import weights as W
from oracle.pyg_restatement import matrix_to_quaternion

pytestmark = pytest.mark.gpu
GTOL = 1e-3
ULP16 = 16 * 2.0 ** -23
RTOL32, TRAJ32 = 1e-4, 5e-4
ARCHS = ["transformer", "exophormer", "gcn"]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden11():
    return T6.load_golden11()


def within_4x(name, hip, f32, f64):
    scale = float(f64.abs().max()) or 1.0
    e32 = float((f32.double() - f64).abs().max()) / scale
    ehip = float((hip.double().cpu() - f64).abs().max()) / scale
    print(f"{name}: scale {scale:.3e}  torch-fp32 err {e32:.3e}  HIP err {ehip:.3e}")
    assert math.isfinite(ehip) and ehip <= max(4 * e32, ULP16), (name, e32, ehip)
    return e32, ehip


def module_6dof(arch, dev, steps=T6.STEPS, ratio=1, noise_weight=0.0, freeze=True, max_parts=T6.MAX_PARTS, sd=None):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    m = GNN_Diffusion(steps=steps, sampling="DDIM", inference_ratio=ratio, noise_weight=noise_weight, model_mean_type=ModelMeanType.START_X,
                      backbone="vn_dgcnn", architecture=arch, max_num_part=max_parts, loss_type="all", freeze_backbone=freeze, use_6dof=True)
    if sd is not None:
        missing, unexpected = m.model.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("pcd_backbone.") for k in missing)
    return m.to(dev)


# ------------------------------------------------------------------------------------------------ da_rot6d_to_pose
N_SPECIAL = 8


def rot6d_rows(n, seed=23):
    """pred [n, 13] fp32 and d_pose [n, 7]: the special rows of rot6d_refs first (a1 parallel to e_x, sine 1e-2, |a1| = 1e-3, w = 1e-3 on
    either side, identity, ...), then N(0, 1) rows; |w| >= 9e-4 on every Gram-Schmidt quaternion by construction of the seed."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, 13, generator=g)
    k = min(n, N_SPECIAL)
    pred[:k, 7:] = R6.special_rows()[:k, 7:].float()
    return pred, torch.randn(n, 7, generator=g)


def run_rot6d(dev, pred, d_pose, ld=13):
    from diffassemble_amd import _lib
    n = pred.shape[0]
    src = torch.full((n, ld), float("nan"), device=dev)
    src[:, :13] = pred.to(dev)
    pose = torch.full((n + 2, 7), -7.25, device=dev)
    d_pred = torch.full((n + 2, 13), -7.25, device=dev)
    g = d_pose.to(dev).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().da_rot6d_to_pose(n, _lib.ptr(src), ld, _lib.ptr(pose), _lib.stream_ptr(dev)))
        _lib.check(_lib.lib().da_rot6d_to_pose_backward(n, _lib.ptr(src), ld, _lib.ptr(g), _lib.ptr(d_pred), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool((pose[n:] == -7.25).all()) and bool((d_pred[n:] == -7.25).all()), "a guard row was written"
    return pose[:n].cpu(), d_pred[:n].cpu()


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_rot6d_to_pose_forward_and_backward(dev, n):
    pred, g = rot6d_rows(n)
    f64, b64 = R6.rot6d_to_pose(pred.double()), R6.rot6d_to_pose_backward(pred.double(), g.double())
    f32, b32 = R6.rot6d_to_pose(pred), R6.rot6d_to_pose_backward(pred, g)
    assert float(f64[:, 0].min()) >= 9e-4                                  # away from the sign flip of the standardisation
    pose, d_pred = run_rot6d(dev, pred, g)
    assert torch.equal(pose[:, 4:], pred[:, 4:7])                          # the translation is copied
    assert torch.equal(d_pred[:, :4], torch.zeros(n, 4)) and torch.equal(d_pred[:, 4:7], g[:, 4:7])
    within_4x(f"rot6d forward n={n}", pose, f32, f64)
    within_4x(f"rot6d backward n={n}", d_pred, b32, b64)
    k = min(n, N_SPECIAL)
    within_4x(f"rot6d forward n={n}, special rows", pose[:k], f32[:k], f64[:k])
    within_4x(f"rot6d backward n={n}, special rows", d_pred[:k], b32[:k], b64[:k])
    if n == 65:                                                            # rows of 16 floats with NaN padding: the same bits
        pose16, d_pred16 = run_rot6d(dev, pred, g, ld=16)
        assert torch.equal(pose16, pose) and torch.equal(d_pred16, d_pred)


def test_rot6d_zero_row_is_finite(dev):
    pred, g = rot6d_rows(5)
    pred[2] = 0.0
    pred[4, 10:] = 2.0 * pred[4, 7:10]                                     # a2 parallel to a1: the second normalisation meets its clamp
    pose, d_pred = run_rot6d(dev, pred, g)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(d_pred).all())
    assert torch.equal(pose[2], torch.tensor([0.5, 0, 0, 0, 0, 0, 0]))     # matrix_to_quaternion of the zero matrix, as torch gives it
    assert torch.equal(pose[2], R6.rot6d_to_pose(pred)[2])
    keep = [0, 1, 3]
    within_4x("rot6d rows beside a zero row", pose[keep], R6.rot6d_to_pose(pred)[keep], R6.rot6d_to_pose(pred.double())[keep])


def test_rot6d_function_links_autograd(dev):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import Rot6dToPoseFn, rot6d_to_pose
    pred, g = rot6d_rows(65)
    x = pred.to(dev).requires_grad_(True)
    pose = Rot6dToPoseFn.apply(x)
    (pose * g.to(dev)).sum().backward()
    want_pose, want_grad = run_rot6d(dev, pred, g)
    assert torch.equal(pose.detach().cpu(), want_pose) and torch.equal(x.grad.cpu(), want_grad)
    wide = torch.zeros(65, 16, device=dev)
    wide[:, :13] = pred.to(dev)
    assert torch.equal(rot6d_to_pose(wide[:, :13]).cpu(), want_pose)      # a strided view is read in place


# ------------------------------------------------------------------------------------------------ k_head3d_bwd, T_CH = 9
SPECIAL_NORMS = (0.0, 1e-6, 9e-5, 1.1e-4, 3.0, 3.3, 4.0, 6.0)      # test_gpu_train3d.py's: r = 0, the series switch, the sign change of w


def head_rows9(n, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    norms = rng.uniform(0.05, 2.0, n)
    norms[: min(n, len(SPECIAL_NORMS))] = SPECIAL_NORMS[: min(n, len(SPECIAL_NORMS))]
    assert np.abs(np.cos(norms / 2)).min() >= 1e-3
    r = torch.from_numpy((d * norms[:, None]).astype(np.float32))
    t = torch.from_numpy(rng.standard_normal((n, 9)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((n, 13)).astype(np.float32))
    return torch.cat([r, t], 1), g


def head_autograd9(pre, g, dtype):
    p = pre.to(dtype).requires_grad_(True)
    q = F.normalize(matrix_to_quaternion(so3.skew_to_rmat(p[:, :3])), p=2, dim=-1)
    (torch.hstack((q, p[:, 3:])) * g.to(dtype)).sum().backward()
    return p.grad.detach()


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_head3d_backward_with_nine_translation_channels(dev, n):
    from diffassemble_amd import _lib
    pre, g = head_rows9(n)
    g64, g32 = head_autograd9(pre, g, torch.float64), head_autograd9(pre, g, torch.float32)
    d_pre = torch.full((n + 1, 12), float("nan"), device=dev)
    pre_d, g_d = pre.to(dev), g.to(dev)
    _lib.check(_lib.lib().da_head3d_backward_ex(n, 9, _lib.ptr(pre_d), _lib.ptr(g_d), _lib.ptr(d_pre), _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_pre[n]).all())
    d_pre = d_pre[:n].cpu()
    assert torch.equal(d_pre[:, 3:], g[:, 4:])                           # all nine channels pass straight through
    within_4x(f"head3d backward (9) n={n}", d_pre[:, :3], g32[:, :3], g64[:, :3])
    k = min(n, len(SPECIAL_NORMS))
    within_4x(f"head3d backward (9) n={n}, special rows", d_pre[:k, :3], g32[:k, :3], g64[:k, :3])
    # the rotation part is the 3-channel kernel's, bit for bit
    d6 = torch.empty((n, 6), device=dev)
    pre6 = torch.cat([pre[:, :3], pre[:, 3:6]], 1).to(dev).contiguous()
    g7 = g[:, :7].to(dev).contiguous()
    _lib.check(_lib.lib().da_head3d_backward(n, _lib.ptr(pre6), _lib.ptr(g7), _lib.ptr(d6), _lib.stream_ptr(dev)))
    assert torch.equal(d6[:, :3].cpu(), d_pre[:, :3])


# ------------------------------------------------------------------------------------------------ da_q_sample_se3_6d
_TRAP = {}


def trap_table(m):
    from diffassemble_amd.engine import igso3_trap_table
    if m.steps not in _TRAP:
        _TRAP[m.steps] = igso3_trap_table(m.sqrt_one_minus_alphas_cumprod.cpu())
    return _TRAP[m.steps]


def schedule_module(steps=T6.STEPS):
    from diffassemble_amd.model.spatial_diffusion_3d_test_double_diffusion import GNN_Diffusion, ModelMeanType
    return GNN_Diffusion(steps=steps, sampling="DDIM", backbone="vn_dgcnn", max_num_part=T6.MAX_PARTS, model_mean_type=ModelMeanType.START_X,
                         use_6dof=True)


def run_noising(m, dev, x_start, t, noise_tr, axes, unif):
    out = m.to(dev).q_sample_se3(x_start.to(dev), t.to(dev), (noise_tr.to(dev), axes.to(dev), unif.to(dev)))
    torch.cuda.synchronize()
    m.cpu()
    return out.cpu()


@pytest.mark.parametrize("spec", T6.TRAIN3D_6DOF, ids=lambda s: s["name"])
def test_q_sample_se3_6d_reproduces_the_reference_noising(dev, golden11, spec):
    case = T6.build_case(spec)
    name = spec["name"]
    t = torch.from_numpy(golden11[f"{name}/t"])
    assert torch.equal(t, case["t"])
    draws = [torch.from_numpy(golden11[f"{name}/{k}"]) for k in ("noise_tr", "axes", "unif")]
    want = torch.from_numpy(golden11[f"{name}/x_noisy"])
    assert want.shape[1] == 13 and float(want[:, 0].abs().min()) >= T6.W_MIN
    m = schedule_module()
    trap = trap_table(m)
    f64 = R6.noising_restatement_6d(m, trap, case["x_start"], t, *draws, torch.float64)
    f32 = R6.noising_restatement_6d(m, trap, case["x_start"], t, *draws, torch.float32)
    got = run_noising(m, dev, case["x_start"], t, *draws)
    assert got.shape == (case["x_start"].shape[0], 13)
    e32, _ = within_4x(f"{name} x_noisy", got, f32, f64)
    eref = float((want.double() - f64).abs().max()) / float(f64.abs().max())
    print(f"{name}: reference fixture vs fp64 restatement {eref:.3e}")
    assert eref <= max(4 * e32, ULP16)


@pytest.mark.parametrize("n", [1, 65])
def test_q_sample_se3_6d_edge_rows(dev, n):
    """unif in {0, just below the first positive CDF entry, 1 - 2^-24, exactly 1.0}, t in {0, steps - 1}, identity and random rotations."""
    m = schedule_module()
    trap = trap_table(m)
    rng = np.random.default_rng(9)
    rows = []
    for t in (0, m.steps - 1):
        first = trap[t][trap[t] > 0][0]
        for u in (0.0, float(torch.nextafter(first, torch.tensor(0.0))), 1.0 - 2.0 ** -24, 1.0):
            for ident in (True, False):
                rows.append((t, u, ident))
    rows = [rows[i % len(rows)] for i in range(n)] if n > 1 else [rows[7]]
    t = torch.tensor([r[0] for r in rows])
    unif = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    assert float(unif.max()) == 1.0
    q = T3.unit_quaternions(rng, n)
    for i, r in enumerate(rows):
        if r[2]:
            q[i] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    x_start = torch.cat([q, torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))], 1)
    noise_tr = torch.from_numpy(rng.standard_normal((n, 9)).astype(np.float32))
    axes = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    f64 = R6.noising_restatement_6d(m, trap, x_start, t, noise_tr, axes, unif, torch.float64)
    f32 = R6.noising_restatement_6d(m, trap, x_start, t, noise_tr, axes, unif, torch.float32)
    keep = f64[:, 0].abs() >= T6.W_MIN                                 # (a row whose w is rounding's to sign is compared up to that sign)
    got = run_noising(m, dev, x_start, t, noise_tr, axes, unif)
    assert got.shape == (n, 13) and bool(torch.isfinite(got).all())
    assert float((got[:, :4].norm(dim=1) - 1).abs().max()) < 1e-5

    def signed(x):
        s = torch.where(keep, torch.ones(n), torch.sign((x[:, :4].double() * f64[:, :4]).sum(1)).float())
        return torch.cat([x[:, :4] * s[:, None], x[:, 4:]], 1)

    within_4x(f"6dof edge rows n={n}", signed(got), signed(f32), f64)


# ------------------------------------------------------------------------------------------------ forward, p_losses vs golden_v11
@pytest.mark.parametrize("spec", T6.TRAIN3D_6DOF, ids=lambda s: s["name"])
def test_forward_matches_the_reference_fixture(dev, golden11, spec):
    name = spec["name"]
    case = T6.build_case(spec)
    want = torch.from_numpy(golden11[f"{name}/prediction"])
    m = module_6dof(spec["arch"], dev, sd=case["sd"]).eval()
    m.model.precision = "fp32"
    with torch.no_grad():
        out, _ = m.forward_with_feats(torch.from_numpy(golden11[f"{name}/x_noisy"]).to(dev), case["t"].to(dev), case["edge_index"].to(dev),
                                      case["feats"].to(dev), case["batch"].to(dev))
    torch.cuda.synchronize()
    assert out.shape == want.shape == (case["x_start"].shape[0], 13)
    e = rel(out, want)
    eq, et = rel(out[:, :4], want[:, :4]), rel(out[:, 4:], want[:, 4:])
    print(f"{name}: prediction rel err {e:.3e} (quaternion {eq:.3e}, nine channels {et:.3e})")
    assert e < RTOL32 and eq < RTOL32 and et < RTOL32
    assert float((out[:, :4].norm(dim=1) - 1).abs().max()) < 1e-5


def fixture_step(spec, case, golden11, dev, precision, staged=False):
    name = spec["name"]
    m = module_6dof(spec["arch"], dev, sd=case["sd"]).train()
    te = m.model.train_engine(dev)
    te.precision = precision
    te.force_staged = staged
    noise = tuple(torch.from_numpy(golden11[f"{name}/{k}"]).to(dev) for k in ("noise_tr", "axes", "unif"))
    losses = m.p_losses(case["x_start"].to(dev), torch.from_numpy(golden11[f"{name}/t"]).to(dev), noise=noise, loss_type="all",
                        cond=case["pts"].to(dev), edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                        n_batch=len(T6.SIZES), valids=case["valids"].to(dev), pcd_feats=case["feats"].to(dev))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return m, losses


def loss_errors(name, losses, golden11):
    errs = {}
    for k, v in losses.items():
        ref = float(golden11[f"{name}/loss/{k}"])
        errs[k] = abs(float(v) - ref) / abs(ref) if ref != 0.0 else abs(float(v))
    return errs


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("spec", T6.TRAIN3D_6DOF, ids=lambda s: s["name"])
def test_p_losses_matches_the_reference_fixture(dev, golden11, spec, staged):
    """The reference's own use_6dof p_losses + backward: each entry of the loss dictionary, then every live gradient's first 64
    entries and its (|g| sum, g^2 sum); every mlp_r.* gradient is exactly zero (the loss never reads the head's quaternion)."""
    name = spec["name"]
    case = T6.build_case(spec)
    m, losses = fixture_step(spec, case, golden11, dev, "fp32", staged)
    assert list(losses) == ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss"]
    errs = loss_errors(name, losses, golden11)
    print(f"{name}: loss entries rel err {errs}")
    assert all(e < 1e-5 for e in errs.values()), errs
    live = {k: p for k, p in m.model.named_parameters() if f"{name}/grad_head/{k}" in golden11.files}
    assert len(live) == len(case["sd"])
    assert tuple(live["mlp_t.2.weight"].grad.shape) == (9, 256) and tuple(live["pos_mlp.0.weight"].grad.shape) == (16, 13)
    for k, p in live.items():
        if k.startswith("mlp_r."):
            assert float(p.grad.abs().max()) == 0.0, k
    assert all(float(live["mlp_t.2.weight"].grad[r].abs().max()) > 0 for r in range(9))
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in live.values())
    worst = [0.0, 0.0, 0.0]
    for k, p in live.items():
        ref = torch.from_numpy(golden11[f"{name}/grad_head/{k}"]).double()
        got = p.grad.flatten()[: ref.numel()].double().cpu()
        e0 = float((got - ref).abs().max()) / max(float(ref.abs().max()), floor)
        worst[0] = max(worst[0], e0)
        assert e0 < GTOL, (k, e0)
        g = p.grad.double().cpu()
        st, st_ref = torch.stack([g.sum(), g.abs().sum(), (g * g).sum()]), golden11[f"{name}/grad_stats/{k}"]
        if float(st_ref[1]) > floor * p.numel() * 1e-2:
            e1 = abs(float(st[1]) - float(st_ref[1])) / float(st_ref[1])
            e2 = abs(float(st[2]) - float(st_ref[2])) / float(st_ref[2])
            worst[1], worst[2] = max(worst[1], e1), max(worst[2], e2)
            assert e1 < GTOL and e2 < 2 * GTOL, (k, e1, e2)
    print(f"{name}: worst (head, |g| sum, g^2 sum) {worst}")


def test_p_losses_in_the_bf16_mode_vs_the_reference_fixture(dev, golden11):
    """The transformer's fixture against the bf16-operand mode, with the bound test_gpu_train3d.py documents for it: loss 5e-3; per
    gradient tensor the first 64 entries within 2.5 % of the tensor's largest entry, |g| sum within 1.5 %, g^2 sum within 2 %."""
    spec = T6.TRAIN3D_6DOF[0]
    name = spec["name"]
    case = T6.build_case(spec)
    m, losses = fixture_step(spec, case, golden11, dev, "bf16")
    errs = loss_errors(name, losses, golden11)
    print(f"{name} bf16: loss entries rel err {errs}")
    assert all(e < 5e-3 for e in errs.values()), errs
    live = {k: p for k, p in m.model.named_parameters() if f"{name}/grad_head/{k}" in golden11.files}
    floor = 1e-3 * max(float(p.grad.abs().max()) for p in live.values())
    worst, n = [0.0, 0.0, 0.0], 0
    for k, p in live.items():
        ref = torch.from_numpy(golden11[f"{name}/grad_head/{k}"]).double()
        got = p.grad.flatten()[: ref.numel()].double().cpu()
        st_ref = golden11[f"{name}/grad_stats/{k}"]
        if k.startswith("mlp_r."):
            assert float(p.grad.abs().max()) == 0.0, k
        if float(st_ref[1]) <= floor * p.numel() * 1e-1:
            continue                                                     # identically-zero gradients: rounding noise
        g = p.grad.double().cpu()
        e = [float((got - ref).abs().max()) / max(float(ref.abs().max()), float(p.grad.abs().max()), floor),
             abs(float(g.abs().sum()) - float(st_ref[1])) / float(st_ref[1]),
             abs(float((g * g).sum()) - float(st_ref[2])) / float(st_ref[2])]
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < 2.5e-2 and e[1] < 1.5e-2 and e[2] < 2e-2, (k, e)
        n += 1
    print(f"{name} bf16 mode vs reference fixture, worst (head, |g| sum, g^2 sum): {worst} over {n} tensors")
    assert n >= 12 and worst[0] > 1e-5


# ------------------------------------------------------------------------------------------------ sampling loop, evaluation
def loop_module(dev, noise_weight=0.0):
    spec = next(s for s in T6.TRAIN3D_6DOF if s["name"] == T6.LOOP_CASE)
    case = T6.build_case(spec)
    m = module_6dof(spec["arch"], dev, ratio=T6.LOOP_RATIO, noise_weight=noise_weight, sd=case["sd"]).eval()
    m.model.precision = "fp32"
    return m, case


def run_loop(m, case, dev):
    imgs, _ = m.p_sample_loop(case["x_start"].shape, None, case["edge_index"].to(dev), batch=case["batch"].to(dev), pcd_feats=case["feats"].to(dev))
    torch.cuda.synchronize()
    return torch.stack([i.clone() for i in imgs]).cpu()


_ROUTES = {}


def loop_routes(dev):
    """The 10-step trajectory through the captured loop and through the per-step route (return_attentions=True): run once, shared."""
    if not _ROUTES:
        m, case = loop_module(dev)
        assert m.use_hip_graph
        _ROUTES["captured loop"] = run_loop(m, case, dev)
        m.return_attentions = True
        _ROUTES["per-step route"] = run_loop(m, case, dev)
    return _ROUTES


def test_p_sample_loop_routes_are_bit_equal(dev):
    """The captured loop and the per-step route give the same bits.  The per-step route asks the forward for every layer's attention
    weights, which only the edge-list kernels produce; in this mode the forward computes them in a pass of their own and the layer's rows
    by the kernels it takes without the request (da_forward.hip: forward_impl), so the request does not move the output.  (With one pass,
    as the other models run it, the two trajectories differed by 5.96e-08 max abs: two summation orders.)"""
    r = loop_routes(dev)
    got, step = r["captured loop"], r["per-step route"]
    print(f"captured loop vs per-step route: max abs difference {float((got - step).abs().max()):.3e}")
    assert torch.equal(got, step)


@pytest.mark.parametrize("spec", T6.TRAIN3D_6DOF[:2], ids=lambda s: s["name"])
def test_attention_request_leaves_the_output_alone_and_returns_the_weights(dev, golden11, spec):
    """forward_with_feats with and without return_attentions (transformer, exophormer with its virtual rows): the same prediction bit for
    bit; one (edge_index, alpha [E, 8]) pair per returned layer, every destination's weights summing to one per head."""
    name = spec["name"]
    case = T6.build_case(spec)
    m = module_6dof(spec["arch"], dev, sd=case["sd"]).eval()
    m.model.precision = "fp32"
    args =(torch.from_numpy(golden11[f"{name}/x_noisy"]).to(dev), case["t"].to(dev), case["edge_index"].to(dev), case["feats"].to(dev),
            case["batch"].to(dev))
    with torch.no_grad():
        plain, none = m.forward_with_feats(*args, return_attentions=False)
        plain = plain.clone()
        asked, atts = m.forward_with_feats(*args, return_attentions=True)
    torch.cuda.synchronize()
    assert none is None and torch.equal(plain, asked)
    assert len(atts) == (4 if spec["arch"] == "transformer" else 1)      # (the exophormer module returns its last layer's weights only)
    for ei, alpha in atts:
        assert alpha.shape == (ei.shape[1], 8) and bool(torch.isfinite(alpha).all()) and float(alpha.min()) >= 0
        sums = torch.zeros(int(ei.max()) + 1, 8, device=dev).index_add_(0, ei[1], alpha)
        assert float((sums[ei[1].unique()] - 1).abs().max()) < 1e-5


def test_p_sample_loop_matches_the_reference_trajectory(dev, golden11):
    """10 DDIM steps (inference_ratio 30, noise_weight 0) through the captured loop and through the per-step route; 13-wide entries."""
    ref = torch.from_numpy(golden11["loop/traj"])
    case = T6.build_case(next(s for s in T6.TRAIN3D_6DOF if s["name"] == T6.LOOP_CASE))
    for name, tr in loop_routes(dev).items():
        assert tr.shape == ref.shape == (T6.LOOP_ITERS, case["x_start"].shape[0], 13)
        et = rel(tr[..., 4:], ref[..., 4:])
        dq = torch.minimum((tr[..., :4] - ref[..., :4]).abs().amax(-1), (tr[..., :4] + ref[..., :4]).abs().amax(-1))
        print(f"{name}: nine channels rel err {et:.3e}, quaternion max abs err {float(dq.max()):.3e}")
        assert et < TRAJ32 and float(dq.max()) < TRAJ32


def test_p_sample_loop_with_noise(dev):
    m, case = loop_module(dev, noise_weight=1.0)
    torch.manual_seed(5)
    got = run_loop(m, case, dev)
    assert got.shape == (T6.LOOP_ITERS, case["x_start"].shape[0], 13) and bool(torch.isfinite(got).all())
    assert float((got[..., :4].norm(dim=-1) - 1).abs().max()) < 1e-5
    torch.manual_seed(6)
    assert not torch.equal(run_loop(m, case, dev), got)                   # the start is drawn: nine noisy channels


def test_eval_step_scores_the_fixture_poses(dev, golden11):
    """_eval_step on the reference's final 13-wide rows (a stub p_sample_loop returns them): pose7 by da_rot6d_to_pose, then the four
    metrics per object against the reference's own (utils_3d.py on its Gram-Schmidt poses)."""
    from diffassemble_amd.metrics3d import batch_metrics
    m, case = loop_module(dev)
    traj = torch.from_numpy(golden11["loop/traj"])
    ref_pose, ref_metrics = torch.from_numpy(golden11["loop/pose7"]), torch.from_numpy(golden11["loop/metrics"])
    m.p_sample_loop = lambda *a, **k: ([traj[-1].to(dev)], [None])
    cats = ["a", "b", "c"]
    m.initialize_torchmetrics(cats)
    batch = SimpleNamespace(x=case["x_start"].to(dev), pcds=case["pts"].to(dev), edge_index=case["edge_index"].to(dev),
                            batch=case["batch"].to(dev), pcd_feats=case["feats"].to(dev), category=cats)
    final = m.validation_step(batch, 0).cpu()
    assert final.shape == (traj.shape[1], 7)
    pose64 = R6.rot6d_to_pose(traj[-1].double())
    within_4x("eval pose7", final, ref_pose, pose64)
    q = pose64[:, :4]
    assert float((2 * (q[:, 0] * q[:, 2] - q[:, 1] * q[:, 3])).abs().max()) <= 0.99      # test_gpu_metrics3d.py's input condition
    got = torch.tensor([[float(m.metrics[f"{k}_{c}"].compute()) for k in ("rmse_t", "rmse_r", "gd_r", "part_acc")] for c in cats], dtype=torch.float64)
    ptr = T6.ptr_of()
    m64 = batch_metrics(case["pts"].double(), pose64, case["x_start"].double(), ptr=ptr)
    print("metrics: module", got.tolist(), "reference", ref_metrics.tolist())
    for c, k in enumerate(("rmse_t", "rmse_r", "gd_r")):
        within_4x(f"eval {k}", got[:, c], ref_metrics[:, c].float(), m64[:, c])
    assert torch.equal(got[:, 3], ref_metrics[:, 3])                      # part accuracy: a count


# ------------------------------------------------------------------------------------------------ one optimizer step
def small_batch(dev, sizes=(2, 5), n_points=64, seed=44, steps=20):
    P = sum(sizes)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    return SimpleNamespace(x=T3.poses(P, seed).to(dev), pcds=W.make_point_clouds(P, n_points, seed).to(dev), edge_index=edge_index.to(dev),
                           batch=batch.to(dev), valids=T3.valids_of(sizes, 6).to(dev), data_id=list(range(len(sizes))))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("arch", ARCHS)
def test_one_full_training_step(dev, arch, precision):
    """training_step -> the fused Adafactor -> p_sample_loop in eval(): the parameters moved, everything is finite, 13-wide poses."""
    from diffassemble_amd.train import FusedAdafactor
    b = small_batch(dev)
    m = module_6dof(arch, dev, steps=20, sd=T6.make_state(arch, 20, 621))
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v))
    m.train()
    te = m.model.train_engine(dev)
    te.precision = precision
    opt = m.configure_optimizers()
    assert isinstance(opt, FusedAdafactor)
    torch.manual_seed(3)
    loss = m.training_step(b, 1)
    loss.backward()
    flat0 = te.flat.clone()
    opt.step()
    torch.cuda.synchronize()
    assert set(logged) == {"trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss", "loss"}
    assert math.isfinite(float(loss)) and bool(torch.isfinite(te.flat).all()) and bool(torch.isfinite(te.flat_grad).all())
    assert not torch.equal(flat0, te.flat)
    params = dict(m.model.named_parameters())
    assert all(float(params[k].grad.abs().max()) == 0.0 for k in params if k.startswith("mlp_r."))
    assert float(params["mlp_t.2.weight"].grad.abs().amax(1).min()) > 0           # all nine rows of mlp_t.2 get gradient
    m.eval()
    after = m.p_sample_loop(b.x.shape, b.pcds, b.edge_index, batch=b.batch)[0][-1]
    assert after.shape == (b.x.shape[0], 13) and bool(torch.isfinite(after).all())


# ------------------------------------------------------------------------------------------------ no shared state with the 7-channel model
def test_seven_channel_denoiser_is_untouched_by_a_13_channel_one(dev):
    """One c_in = 7 forward and one 7-channel DDIM step, bit-equal between a denoiser created before and one created after a
    13-channel denoiser has run in the same process."""
    from diffassemble_amd import DenoiserEngine, Schedule, _lib
    from oracle import diffusion as ODF
    sd7, sd13 = T3.make_state("transformer", 50, 7), T6.make_state("transformer", 50, 7)
    sizes = (5, 2, 6)
    P = sum(sizes)
    edge_index, batch = W.collate([W.dense_edge_index(n, True) for n in sizes], list(sizes))
    _, feats = W.make_inputs(P, 7, T3.FEAT, 3)
    x7 = T3.poses(P, 3)
    t = torch.full((P,), 30, dtype=torch.long)
    sch = Schedule(ODF.make_schedule(50), dev)

    def run7():
        eng = DenoiserEngine(sd7, variant="3d", arch="transformer", precision="fp32", device=dev)
        out = eng.forward(eng.plan(edge_index, batch), x7.to(dev), t.to(dev), feats.to(dev))
        step = eng.ddim_step(sch, x7.to(dev), out, t.to(dev), 10, _lib.MEAN_START_X)
        torch.cuda.synchronize()
        return out.cpu(), step.cpu()

    before = run7()
    eng13 = DenoiserEngine(sd13, variant="3d", arch="transformer", precision="fp32", device=dev)
    assert eng13.c_in == 13 and eng13.c_pose == 13 and eng13.c_out == 12
    x13 = torch.cat([x7, torch.randn(P, 6, generator=torch.Generator().manual_seed(1))], 1)
    out13, pre13 = eng13.forward(eng13.plan(edge_index, batch), x13.to(dev), t.to(dev), feats.to(dev), return_pre_head=True)
    step13 = eng13.ddim_step(sch, x13.to(dev), out13, t.to(dev), 10, _lib.MEAN_START_X)
    torch.cuda.synchronize()
    assert out13.shape == step13.shape == (P, 13) and pre13.shape == (P, 12)
    assert torch.equal(out13[:, 4:].cpu(), pre13[:, 3:].cpu()) and bool(torch.isfinite(step13).all())
    after = run7()
    assert before[0].shape == (P, 7) and torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
