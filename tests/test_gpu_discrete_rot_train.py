"""GPU tests of the discrete position + rotation model's training side: da_d3pm_q_sample_rot and da_d3pm_rot_loss on their own, the
two-head training forward + backward against fp64 autograd, p_losses against the reference's own step (golden_v10.npz,
make_golden_v10.py), one training_step + optimizer step (plain and only_rotation), and the guards of the C entries.

Bounds are those of test_gpu_discrete_train.py.  The per-piece fp32 kernels: ``within_4x`` -- at most 4x the error of the same
expression evaluated by torch in fp32 against fp64, in max-abs terms scaled by the largest element, floored at 16 fp32 ulps; row
terms and loss parts 1e-5.  Argmax outputs are compared where the fp64 top-2 gap is >= 1e-3 (discrete_cases.check_argmax; the cases
are asserted clear of ties by tests/test_discrete_rot_train_host.py).  The denoiser: outputs 1e-4, gradients and d_feats GTOL = 1e-3
with the 1e-4 x max floor.  The fixture: each loss within max(5 x its recorded deviation, 1e-5), gradients by the three checks of
``fixture_errors`` with 1e-3 / 2e-3; the bf16-operand mode is held to 4x the error the restatement itself shows against the fixture
under torch.autocast("cpu", bfloat16), never tighter than the floors documented there (loss 5e-3; heads 2.5e-2, |g| sum 1.5e-2,
g^2 sum 2e-2)."""
import ctypes as C
import math

import pytest
import torch

import discrete_cases as DC
import discrete_rot_cases as RC
import discrete_rot_train_cases as RT

pytestmark = pytest.mark.gpu
GTOL = 1e-3
ULP16 = 16 * 2.0 ** -23
HEAD = ("final_mlp.0.weight", "final_mlp.0.bias", "final_mlp.2.weight", "final_mlp.2.bias")


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g10():
    return RT.load_golden10()


def within_4x(name, hip, f32, f64):
    scale = float(f64.abs().max())
    e32 = float((f32.double() - f64).abs().max()) / scale
    ehip = float((hip.double().cpu() - f64).abs().max()) / scale
    print(f"{name}: scale {scale:.3e}  torch-fp32 err {e32:.3e}  HIP err {ehip:.3e}")
    assert math.isfinite(ehip) and ehip <= max(4 * e32, ULP16), (name, e32, ehip)


_SCHED = {}


def sched_for(dev, steps):
    if steps not in _SCHED:
        from diffassemble_amd.engine import Schedule
        from diffassemble_amd.model import spatial_diffusion as SD
        from diffassemble_amd.model.spatial_diffusion_discrete_rot import GNN_Diffusion
        m = GNN_Diffusion(puzzle_sizes=[(2, 2)], steps=steps, sampling="DDPM", scheduler=SD.ModelScheduler.LINEAR)
        assert torch.equal(m.alphas_cumprod, DC.linear_alphas_cumprod(steps))
        _SCHED[steps] = Schedule({k: getattr(m, k) for k in Schedule.KEYS}, dev)
    return _SCHED[steps]


# ------------------------------------------------------------------------------------------------ da_d3pm_q_sample_rot
@pytest.mark.parametrize("n", RT.Q_NS)
@pytest.mark.parametrize("K", RT.Q_KS)
def test_both_noisings_against_the_fp64_restatement(dev, K, n):
    from diffassemble_amd.engine import d3pm_noise, d3pm_q_sample, d3pm_q_sample_rot
    steps = RT.Q_STEPS
    x0, r0, t, u, ur = RT.q_sample_case(n, K, steps, RT.Q_SEEDS[(K, n)])
    sch, ac = sched_for(dev, steps), DC.linear_alphas_cumprod(steps)
    want_x, gap_x, want_r, gap_r = RT.q_sample2(ac, x0, r0, t, u, ur, K)
    on = [v.to(dev) for v in (x0, r0, t)]
    gx, gr = d3pm_q_sample_rot(sch, *on, K, noise_x=u.to(dev), noise_rot=ur.to(dev))
    assert gx.dtype == gr.dtype == torch.int64 and 0 <= int(gx.min()) and int(gx.max()) < K and 0 <= int(gr.min()) and int(gr.max()) < 4
    DC.check_argmax(gx, want_x, gap_x, f"q_sample_rot x K={K} n={n}")
    DC.check_argmax(gr, want_r, gap_r, f"q_sample_rot rot K={K} n={n}")
    # the seeded route: the x half is the position model's kernel bit for bit, the rot half the injected route fed by the new domain
    seed = torch.tensor([0x2345678 + K, 7 * n], dtype=torch.int64, device=dev)
    sx, sr = d3pm_q_sample_rot(sch, *on, K, seed=seed)
    assert torch.equal(sx, d3pm_q_sample(sch, on[0], on[2], K, seed=seed))
    u_rot = d3pm_noise(seed, 0, n, 4, domain="training_rot")
    assert float(u_rot.min()) > 0.0 and float(u_rot.max()) <= 1.0
    assert torch.equal(sr, d3pm_q_sample_rot(sch, *on, K, noise_x=u.to(dev), noise_rot=u_rot)[1])
    assert 0 <= int(sx.min()) and int(sx.max()) < K and 0 <= int(sr.min()) and int(sr.max()) < 4
    for other in ("sampling", "training", "sampling_rot"):
        assert not torch.equal(u_rot, d3pm_noise(seed, 0, n, 4, domain=other)), other
    # x_noisy = NULL (only_rotation): same rotations, no position output
    nx, nr = d3pm_q_sample_rot(sch, None, on[1], on[2], K, seed=seed, want_x=False)
    assert nx is None and torch.equal(nr, sr)
    _, _, want_s, gap_s = RT.q_sample2(ac, x0, r0, t, None, u_rot.cpu(), K)
    if float((gap_s < DC.GAP).double().mean()) <= DC.GAP_CAP:
        DC.check_argmax(sr, want_s, gap_s, f"q_sample_rot seeded rot K={K} n={n}")


# ------------------------------------------------------------------------------------------------ da_d3pm_rot_loss
def _loss_refs(ac, rows, kind):
    """fp64 and fp32 (x_loss, rot_loss, d_logits, d_rot_logits) of the restatement, by autograd."""
    logits, x0, xt, rl, r0, rt, t = rows
    out = []
    for dt in (torch.float64, torch.float32):
        z, zr = logits.detach().clone().to(dt).requires_grad_(True), rl.detach().clone().to(dt).requires_grad_(True)
        lx, lr = RT.losses(ac, z, zr, x0, xt, r0, rt, t, kind)
        (lx + lr).backward()
        out.append((lx.detach().reshape(1), lr.detach().reshape(1), z.grad, zr.grad))
    return out


def _check_loss(dev, K, n, scale, seed, tag):
    from diffassemble_amd.engine import d3pm_rot_loss
    steps = RT.Q_STEPS
    sch, ac = sched_for(dev, steps), DC.linear_alphas_cumprod(steps)
    rows = RT.row_mix(n, K, steps, seed=seed, scale=scale)
    logits, x0, xt, rl, r0, rt, t = rows
    on = [v.to(dev) for v in (logits, rl, x0, xt, r0, rt, t)]
    for kind in RT.KINDS:
        f64, f32 = _loss_refs(ac, rows, kind)
        loss, d_logits, d_rot, terms = d3pm_rot_loss(sch, *on, kind=kind, lambda_loss=RT.LAMBDA)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d_logits).all()) and bool(torch.isfinite(d_rot).all())
        for i, what in enumerate(("x_loss", "rot_loss")):
            within_4x(f"{tag} {what} K={K} n={n} {kind}", loss[i:i + 1], f32[i], f64[i])
        within_4x(f"{tag} d_logits K={K} n={n} {kind}", d_logits, f32[2], f64[2])
        within_4x(f"{tag} d_rot_logits K={K} n={n} {kind}", d_rot, f32[3], f64[3])
        sx, sr = RT.smoothing(kind)
        vbx, cex = RT.loss_rows(ac, logits.double(), x0, xt, t, sx)
        vbr, cer = RT.loss_rows(ac, rl.double(), r0, rt, t, sr)
        parts = loss.double().cpu()
        for col, (ref, used) in enumerate(((vbx, kind != "cross_entropy"), (cex, kind != "vb"), (vbr, kind != "cross_entropy"), (cer, kind != "vb"))):
            if used and scale <= 3.0:
                assert abs(float(parts[2 + col]) - float(ref.mean())) <= 1e-5 * max(1.0, abs(float(ref.mean()))), (kind, col)
                assert rel(terms[:, col], ref) < 1e-5, (kind, col)
            elif not used:
                assert float(parts[2 + col]) == 0.0
        again = d3pm_rot_loss(sch, *on, kind=kind, lambda_loss=RT.LAMBDA)
        assert all(torch.equal(a, b) for a, b in zip(again, (loss, d_logits, d_rot, terms)))       # fixed summation order
        # logits = NULL (only_rotation): the position half is skipped, a sentinel-filled d_logits stays, the rotation half is the same
        sentinel = torch.full_like(on[0], 7.0)
        l2, dl2, dr2, _ = d3pm_rot_loss(sch, None, on[1], None, None, on[4], on[5], on[6], kind=kind, lambda_loss=RT.LAMBDA, d_logits=sentinel)
        torch.cuda.synchronize()
        assert dl2 is None and float(sentinel.min()) == float(sentinel.max()) == 7.0
        assert float(l2[0]) == float(l2[2]) == float(l2[3]) == 0.0 and torch.equal(l2[[1, 4, 5]], loss[[1, 4, 5]]) and torch.equal(dr2, d_rot)


@pytest.mark.parametrize("n", RT.Q_NS)
@pytest.mark.parametrize("K", RT.Q_KS)
def test_two_head_loss_and_its_gradients_against_fp64(dev, K, n):
    _check_loss(dev, K, n, 3.0, 5 * K + n, "rows")


@pytest.mark.parametrize("K", [2, 144, 1024])
def test_two_head_loss_is_finite_at_logit_scale_30(dev, K):
    _check_loss(dev, K, 63, 30.0, K, "scale 30")


@pytest.mark.parametrize("kind", RT.KINDS)
@pytest.mark.parametrize("K", [2, 65, 1024])
def test_position_half_is_the_position_models_loss_row(dev, K, kind):
    """da_d3pm_loss and the position half of da_d3pm_rot_loss run one device routine (d3pm_loss_row) and differ in one argument, the
    label smoothing: 0.01 in every kind for the position model, 0.01 under "hybrid" and 0 otherwise for this one (RT.smoothing).
    "hybrid" (same smoothing): the logit gradient, both row-term columns and the loss parts are equal bit for bit.
    "vb" (the ce row is not used: weight 0, its loss part reads 0): the gradient, the loss parts and the vb column are equal bit for
    bit; the unused ce column holds the smoothed cross entropy there and the plain one here, so it DIFFERS from this model's "vb"
    column and equals its "hybrid" column bit for bit.
    "cross_entropy" (smoothed there, plain here): the ce parts DIFFER -- the smoothing argument is wired, not ignored.
    row_mix's period of 8 gives every t in {0, 1, mid, last} with x_t == x_0 and x_t != x_0; n = 9 ends in a one-row workgroup;
    K = 2 has the empty "neither" class, K = 65 a second stride with one live lane."""
    from diffassemble_amd.engine import d3pm_loss, d3pm_rot_loss
    sch = sched_for(dev, RT.Q_STEPS)
    logits, x0, xt, rl, r0, rt, t = (v.to(dev) for v in RT.row_mix(9, K, RT.Q_STEPS, seed=31 * K))
    loss, d_logits, rows = d3pm_loss(sch, logits, x0, xt, t, kind=kind, lambda_loss=RT.LAMBDA)
    loss_r, d_logits_r, _, rows_r = d3pm_rot_loss(sch, logits, rl, x0, xt, r0, rt, t, kind=kind, lambda_loss=RT.LAMBDA)
    ce_gap = float((rows[:, 1] - rows_r[:, 1]).abs().max())
    if kind == "cross_entropy":
        assert float(loss[2]) != float(loss_r[3]) and not torch.equal(rows[:, 1], rows_r[:, 1]), (loss.tolist(), loss_r.tolist(), ce_gap)
        return
    assert torch.equal(d_logits, d_logits_r), float((d_logits - d_logits_r).abs().max())
    assert torch.equal(loss, loss_r[[0, 2, 3]]), (loss.tolist(), loss_r.tolist())
    assert torch.equal(rows[:, 0], rows_r[:, 0]), float((rows[:, 0] - rows_r[:, 0]).abs().max())
    if kind == "hybrid":
        assert torch.equal(rows[:, 1], rows_r[:, 1]), ce_gap
    else:
        assert RT.smoothing("vb")[0] == 0.0 and not torch.equal(rows[:, 1], rows_r[:, 1])
        rows_h = d3pm_rot_loss(sch, logits, rl, x0, xt, r0, rt, t, kind="hybrid", lambda_loss=RT.LAMBDA)[3]
        assert torch.equal(rows[:, 1], rows_h[:, 1]), float((rows[:, 1] - rows_h[:, 1]).abs().max())


# ------------------------------------------------------------------------------------------------ denoiser forward + backward
def make_backbone(c, dev):
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete_ROT
    m = Eff_GAT_Discrete_ROT(steps=c["steps"], input_channels=c["K"], output_channels=c["K"])
    missing, unexpected = m.load_state_dict(c["sd"], strict=False)
    assert not unexpected and all(k in ("mean", "std") or k.startswith("visual_backbone.") for k in missing)
    return m.to(dev).train()


def _run_backbone(m, c, dev, fx, fr):
    """forward + backward of sum(logits fx) + sum(rot_logits fr); a functional given as None leaves its head out of the loss."""
    m.zero_grad(set_to_none=True)
    feats = c["feats"].to(dev).requires_grad_(True)
    out, out_rot = m.forward_with_feats(c["idx"].to(dev), None, c["t"].to(dev), None, c["edge_index"].to(dev), feats, c["batch"].to(dev))
    assert out.requires_grad and out_rot.requires_grad and out.shape == c["logits"].shape and out_rot.shape == c["rot_logits"].shape
    loss = (out_rot * fr.to(dev)).sum()
    if fx is not None:
        loss = loss + (out * fx.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), out_rot.detach(), feats.grad, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("key", RT.DENOISER_CASES)
def test_two_head_backward_matches_fp64_autograd(dev, key, staged):
    c = RT.denoiser_case(key)
    m = make_backbone(c, dev)
    te = m.train_engine(dev)
    te.force_staged = staged
    assert te.variant == "discrete_rot" and te.c_out == c["K"] and te.c_in == 1 and len(te.params) == len(c["sd"]) == 46
    out, out_rot, d_feats, grads = _run_backbone(m, c, dev, c["fx"], c["fr"])
    e_out, e_rot = rel(out, c["logits"]), rel(out_rot, c["rot_logits"])
    print(f"{key}: logits rel err {e_out:.3e}, rot_logits {e_rot:.3e}")
    assert e_out < 1e-4 and e_rot < 1e-4
    floor = 1e-4 * max(float(g.abs().max()) for g in c["grads"].values())
    errs = {k: float((grads[k].double().cpu() - gr).abs().max()) / max(float(gr.abs().max()), floor) for k, gr in c["grads"].items()}
    e_f = rel(d_feats, c["d_feats"])
    worst = max(errs.items(), key=lambda p: p[1])
    print(f"{key}: worst gradient {worst[0]} {worst[1]:.3e}; d_feats {e_f:.3e}")
    assert all(e < GTOL for e in errs.values()), {k: e for k, e in errs.items() if e >= GTOL}
    assert e_f < GTOL
    params = dict(m.named_parameters())
    lo, hi = te.flat_grad.data_ptr(), te.flat_grad.data_ptr() + te.flat_grad.numel() * 4
    assert all(lo <= params[k].grad.data_ptr() < hi for k in c["grads"])
    # the first layer of both heads is one gap-free slot
    assert params["final_mlp_rot.0.weight"].data_ptr() == params["final_mlp.0.weight"].data_ptr() + 32 * 1152 * 4
    assert params["final_mlp_rot.0.bias"].data_ptr() == params["final_mlp.0.bias"].data_ptr() + 32 * 4
    again = _run_backbone(m, c, dev, c["fx"], c["fr"])[3]
    assert torch.equal(grads["pos_mlp.weight"], again["pos_mlp.weight"])                        # the embedding gradient repeats bit for bit
    # d_logits = None: the position head's gradients are exactly zero, everything else is the run with an all-zero d_logits
    none = _run_backbone(m, c, dev, None, c["fr"])
    zero = _run_backbone(m, c, dev, torch.zeros_like(c["fx"]), c["fr"])
    assert sorted(none[3]) == sorted(zero[3]) == sorted(c["grads"])
    # "Equals": the two runs do the same arithmetic (a zero d_logits contributes exact zeros), but k_time_scatter and the edge-list
    # attention backward add their terms with float atomics, whose order changes from launch to launch (time_emb.weight differed
    # between two runs of the whole suite).  An address receives at most N = number of pieces terms, and reordering N fp32 terms
    # moves their sum by at most N ulps of the terms' magnitude: N x 2^-23 of the tensor's largest entry.  Deterministic tensors
    # agree exactly under the same check.
    tol = c["feats"].shape[0] * 2.0 ** -23

    def same(a, b):
        return float((a.double() - b.double()).abs().max()) <= tol * float(b.double().abs().max())

    for k in c["grads"]:
        if k in HEAD:
            assert float(none[3][k].abs().max()) == 0.0 and float(zero[3][k].abs().max()) == 0.0, k
        assert same(none[3][k], zero[3][k]), k
    assert same(none[2], zero[2]) and float(none[3]["final_mlp_rot.2.weight"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ p_losses vs golden_v10
def diffusion_module(spec, case, dev):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete_rot import GNN_Diffusion
    m = GNN_Diffusion(only_rotation=spec["only_rot"], puzzle_sizes=[(6, 6)], steps=RT.V10["steps"], sampling="DDPM",
                      scheduler=SD.ModelScheduler.LINEAR, loss_type=spec["kind"], lambda_loss=RT.V10["lambda_loss"],
                      classifier_free_prob=spec["cfg_prob"])
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected
    return m.to(dev).train()


def fixture_step(spec, case, g10, dev, precision, staged=False):
    name = spec["name"]
    m = diffusion_module(spec, case, dev)
    te = m.model.train_engine(dev)
    te.precision = precision
    te.force_staged = staged
    x_start, rot_start, t = RT.v10_inputs(spec)
    T = lambda key: torch.from_numpy(g10[f"{name}/{key}"]).to(dev)      # noqa: E731
    losses = m.p_losses(x_start.to(dev), t.to(dev), rot_start.to(dev), noise=T("uniforms_x"), noise_rot=T("uniforms_rot"),
                        loss_type=spec["kind"], cond=None, edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                        cfg_rand=T("cfg_rand"), patch_feats=case["feats4"][0].to(dev))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    x_noisy, rot_noisy = m.last_noisy
    assert torch.equal(x_noisy.cpu().long(), torch.from_numpy(g10[f"{name}/x_noisy"]))          # the noisings are fp32 in both modes
    assert torch.equal(rot_noisy.cpu().long(), torch.from_numpy(g10[f"{name}/rot_noisy"]))
    assert sorted(losses) == (["rot_loss"] if spec["only_rot"] else ["rot_loss", "x_loss"])
    return m, {k: float(v.detach()) for k, v in losses.items()}


def fixture_errors(name, grads, g10, floor_rel, skip_rel):
    """test_gpu_discrete_train.py's three checks per tensor the fixture lists: (first 64 entries, |g| sum, g^2 sum)."""
    names = [str(k) for k in g10[f"{name}/param_names"]]
    floor = floor_rel * max(float(grads[k].abs().max()) for k in names)
    out = {}
    for k in names:
        g = grads[k].double().cpu()
        ref = torch.from_numpy(g10[f"{name}/grad_head/{k}"]).double()
        st_ref = g10[f"{name}/grad_stats/{k}"]
        e0 = float((g.flatten()[: ref.numel()] - ref).abs().max()) / max(float(ref.abs().max()), floor)
        if float(st_ref[1]) > floor * g.numel() * skip_rel:
            out[k] = (e0, abs(float(g.abs().sum()) - float(st_ref[1])) / float(st_ref[1]), abs(float((g * g).sum()) - float(st_ref[2])) / float(st_ref[2]))
        else:
            out[k] = (e0, None, None)
    return out


def _grads_of(m, spec, g10):
    grads = {k: p.grad for k, p in m.model.named_parameters() if p.grad is not None}
    listed = sorted(str(k) for k in g10[f"{spec['name']}/param_names"])
    if spec["only_rot"]:
        # the fixture lists no final_mlp.* (the reference leaves them None); here they are zero
        assert not set(listed) & set(HEAD) and sorted(grads) == sorted(listed + list(HEAD))
        assert all(float(grads[k].abs().max()) == 0.0 for k in HEAD)
    else:
        assert sorted(grads) == listed
    return grads


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("spec", RT.V10_CASES, ids=lambda s: s["name"])
def test_p_losses_matches_the_reference_fixture(dev, g10, spec, staged):
    name = spec["name"]
    case = RC.v9_case()
    m, losses = fixture_step(spec, case, g10, dev, "fp32", staged)
    for k, v in losses.items():
        ref = float(g10[f"{name}/{k}"])
        bound = max(5 * float(g10[f"{name}/dev_{k}"]), 1e-5)
        print(f"{name}: {k} {v:.7f} vs {ref:.7f}: rel {abs(v - ref) / abs(ref):.3e} (bound {bound:.2e})")
        assert abs(v - ref) / abs(ref) <= bound, k
    parts = m.last_loss_parts.cpu()
    assert parts.shape == (6,) and float(parts[1]) == losses["rot_loss"] and float(parts[0]) == losses.get("x_loss", 0.0)
    errs = fixture_errors(name, _grads_of(m, spec, g10), g10, 1e-4, 1e-2)
    worst = [max(e[i] for e in errs.values() if e[i] is not None) for i in range(3)]
    print(f"{name}: worst (head, |g| sum, g^2 sum) {worst}")
    for k, (e0, e1, e2) in errs.items():
        assert e0 < GTOL, (k, e0)
        assert e1 is None or (e1 < GTOL and e2 < 2 * GTOL), (k, e1, e2)


_AUTOCAST = {}


def autocast_errors(spec, case, g10):
    """The yardstick of the bf16-operand mode: the restatement under torch.autocast("cpu", bfloat16) against the same fixture:
    ({loss: error}, worst head, worst |g| sum, worst g^2 sum)."""
    name = spec["name"]
    if name in _AUTOCAST:
        return _AUTOCAST[name]
    x_start, rot_start, t = RT.v10_inputs(spec)
    x_t, rot_t = torch.from_numpy(g10[f"{name}/x_noisy"]), torch.from_numpy(g10[f"{name}/rot_noisy"])
    sdg = {k: v.clone().requires_grad_(True) for k, v in case["sd"].items()}
    keep = (torch.from_numpy(g10[f"{name}/cfg_rand"])[case["batch"]] > spec["cfg_prob"]).float()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        logits, rot_logits = RC.forward_with_feats(sdg, x_t, t, case["edge_index"], keep[:, None] * case["feats4"][0], dtype=torch.float32)
    lx, lr = RT.losses(DC.linear_alphas_cumprod(RT.V10["steps"]), None if spec["only_rot"] else logits.float(), rot_logits.float(), x_start, x_t,
                       rot_start, rot_t, t, spec["kind"], RT.V10["lambda_loss"])
    (lr if lx is None else lx + lr).backward()
    le = {k: abs(float(v.detach()) - float(g10[f"{name}/{k}"])) / abs(float(g10[f"{name}/{k}"])) for k, v in (("x_loss", lx), ("rot_loss", lr)) if v is not None}
    errs = fixture_errors(name, {k: v.grad for k, v in sdg.items() if v.grad is not None}, g10, 1e-3, 1e-1)
    live = [e for e in errs.values() if e[1] is not None]
    _AUTOCAST[name] = (le,) + tuple(max(e[i] for e in live) for i in range(3))
    return _AUTOCAST[name]


@pytest.mark.parametrize("spec", RT.V10_CASES, ids=lambda s: s["name"])
def test_p_losses_in_the_bf16_mode_vs_the_reference_fixture(dev, g10, spec):
    name = spec["name"]
    case = RC.v9_case()
    yard = autocast_errors(spec, case, g10)
    bounds = [max(4 * y, d) for y, d in zip(yard[1:], (2.5e-2, 1.5e-2, 2e-2))]
    m, losses = fixture_step(spec, case, g10, dev, "bf16")
    for k, v in losses.items():
        ref = float(g10[f"{name}/{k}"])
        e, b = abs(v - ref) / abs(ref), max(4 * yard[0][k], 5e-3)
        print(f"{name} bf16: {k} rel {e:.3e} (autocast {yard[0][k]:.3e}, bound {b:.2e})")
        assert e <= b, k
    errs = fixture_errors(name, _grads_of(m, spec, g10), g10, 1e-3, 1e-1)
    live = {k: e for k, e in errs.items() if e[1] is not None}                                  # (identically-zero gradients -- lin_key.bias -- are rounding noise)
    worst = [max(e[i] for e in live.values()) for i in range(3)]
    print(f"{name} bf16: worst (head, |g| sum, g^2 sum) {worst} over {len(live)} tensors; autocast yardstick {yard[1:]}; bounds {bounds}")
    for k, e in live.items():
        assert e[0] <= bounds[0] and e[1] <= bounds[1] and e[2] <= bounds[2], (k, e)
    assert len(live) >= 12 and worst[0] > 1e-5                                                  # ... and the mode really is a different arithmetic


# ------------------------------------------------------------------------------------------------ one full step
@pytest.mark.parametrize("only_rot", [False, True], ids=["plain", "only_rotation"])
def test_one_training_step_and_optimizer_step(dev, only_rot):
    """training_step -> FusedAdafactor.step: the dict and "loss" are logged, the update equals transformers' Adafactor on the same
    gradients (test_gpu_train.py's 2e-6); under only_rotation final_mlp.* are bit-equal before and after."""
    from types import SimpleNamespace
    from transformers.optimization import Adafactor
    from diffassemble_amd.train import FusedAdafactor
    case = RC.v9_case()
    m = diffusion_module(dict(kind="hybrid", cfg_prob=0.0, only_rot=only_rot), case, dev)
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v.detach()))
    m.log_dict = lambda d, *a, **kw: logged.update({k: float(v.detach()) for k, v in d.items()})
    N = case["feats4"].shape[1]
    b = SimpleNamespace(batch=case["batch"].to(dev), edge_index=case["edge_index"].to(dev), patches=None,
                        indexes=(torch.arange(N) % 36 + 36).to(dev), rot_index=(torch.arange(N) % 4 + 4 * (torch.arange(N) % 3)).to(dev),
                        patch_feats=case["feats4"][0].to(dev))                                  # indexes % K, rot_index % 4 are what trains
    opt = m.configure_optimizers()
    assert isinstance(opt, FusedAdafactor)
    te = m.model.train_engine(dev)
    assert te.variant == "discrete_rot" and len(te.params) == len(case["sd"])
    torch.manual_seed(5)
    loss = m.training_step(b, 0)                                     # (batch_idx 0: no sampling dump here)
    loss.backward()
    keys = {"rot_loss"} if only_rot else {"rot_loss", "x_loss"}
    assert set(logged) == keys | {"loss"} and all(math.isfinite(v) for v in logged.values())
    assert abs(logged["loss"] - sum(logged[k] for k in keys)) <= 1e-6 * max(1.0, abs(logged["loss"])) and abs(logged["loss"] - float(loss)) < 1e-6 * max(1.0, abs(float(loss)))
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in te.params]
    for rp, p in zip(ref_params, te.params):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        rp.grad = p.grad.detach().clone()
    before = te.flat.clone()
    head_before = {k: p.detach().clone() for k, p in zip(te.names, te.params) if k in HEAD}
    opt.step()
    Adafactor(ref_params).step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(te.flat).all()) and not torch.equal(before, te.flat)
    for k, p, rp in zip(te.names, te.params, ref_params):
        assert rel(p, rp) < 2e-6, (k, rel(p, rp))
    frozen = HEAD if only_rot else ()
    for k in frozen:
        assert torch.equal(dict(zip(te.names, te.params))[k].detach(), head_before[k]), k
    still = [k for k, p in zip(te.names, te.params) if torch.equal(p.detach().cpu(), case["sd"][k]) and not k.endswith("lin_key.bias") and k not in frozen]
    assert not still, still
    # a second call noises differently (the seed is refilled from torch's generator per call)
    r0, tt = b.rot_index % 4, torch.full((N,), 60, device=dev)
    assert not torch.equal(m.q_sample_rot(r0, tt), m.q_sample_rot(r0, tt))
    assert not torch.equal(m.q_sample(b.indexes % 36, tt), m.q_sample(b.indexes % 36, tt))
    # vb_terms_bpd(K = rot_K) evaluates the rotation process (da_d3pm_loss at K = 4), held to the kernels' rule
    rl = 3.0 * torch.randn(N, 4)
    rt = m.q_sample_rot(r0, tt)
    got = m.vb_terms_bpd(rl.to(dev), None, r0, rt, tt, K=m.rot_K)
    ac = DC.linear_alphas_cumprod(RT.V10["steps"])
    refs = [RT.loss_rows(ac, rl.to(dt), r0.cpu(), rt.cpu(), tt.cpu(), 0.0)[0].mean().reshape(1) for dt in (torch.float32, torch.float64)]
    within_4x("vb_terms_bpd(K=4)", got.detach().reshape(1), refs[0], refs[1])


# ------------------------------------------------------------------------------------------------ guards
def test_entries_reject_what_they_cannot_run(dev):
    from diffassemble_amd import _lib
    from diffassemble_amd.engine import d3pm_q_sample_rot, d3pm_rot_loss
    from diffassemble_amd.graph_plan import build_plan
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete
    lib = _lib.lib()
    c = RT.denoiser_case("dense36x2")
    mr = make_backbone(c, dev)
    te = mr.train_engine(dev)
    plan = build_plan(c["edge_index"].to(dev), c["batch"].to(dev), 0).with_source_csr()
    g, ws = te._cg(plan), te._workspace(plan)
    N, K = c["feats"].shape[0], c["K"]
    xf = torch.zeros((N, 2), device=dev)
    idx = torch.zeros(N, dtype=torch.int32, device=dev)
    t = torch.zeros(N, dtype=torch.int64, device=dev)
    feats = c["feats"].to(dev)
    out, out_rot = torch.full((N, K), 7.0, device=dev), torch.full((N, 4), 7.0, device=dev)
    st = _lib.stream_ptr(dev)
    A = lambda *ts: [_lib.ptr(v) for v in ts]      # noqa: E731
    # the float-pose and the idx entries with rot weights: refused, naming the rot entries
    for rc in (lib.da_train_forward_ex(C.byref(te.w), C.byref(g), *A(xf, t, feats, out, ws), ws.numel(), 0, st),
               lib.da_train_forward_idx(C.byref(te.w), C.byref(g), *A(idx, t, feats, out, ws), ws.numel(), 0, st),
               lib.da_train_backward_stage(C.byref(te.w), C.byref(te.gw), C.byref(g), *A(xf, t, out), None, _lib.ptr(ws), ws.numel(), 0, 0, st),
               lib.da_train_backward_idx(C.byref(te.w), C.byref(te.gw), C.byref(g), *A(idx, t, out), None, _lib.ptr(ws), ws.numel(), 0, 0, st)):
        assert rc != 0 and b"da_train_forward_rot / da_train_backward_rot" in lib.da_last_error()
    # the rot entries with the position model's weights
    md = Eff_GAT_Discrete(steps=c["steps"], input_channels=K, output_channels=K).to(dev).train()
    td = md.train_engine(dev)
    wsd = td._workspace(plan)
    rc = lib.da_train_forward_rot(C.byref(td.w), C.byref(g), *A(idx, t, feats, out, out_rot, wsd), wsd.numel(), 0, st)
    assert rc != 0 and b"da_train_forward_rot: not a discrete rot denoiser" in lib.da_last_error()
    rc = lib.da_train_backward_rot(C.byref(td.w), C.byref(td.gw), C.byref(g), *A(idx, t, out, out_rot), None, _lib.ptr(wsd), wsd.numel(), 0, 0, st)
    assert rc != 0 and b"da_train_backward_rot: not a discrete rot denoiser" in lib.da_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 7.0 and float(out_rot.min()) == float(out_rot.max()) == 7.0      # nothing was launched
    assert float(td.flat_grad.abs().max()) == 0.0 and float(te.flat_grad.abs().max()) == 0.0
    # K outside [2, 1024]
    sch = sched_for(dev, 100)
    for K_bad in (1, 1025):
        with pytest.raises(_lib.DaError, match=r"outside \[2, 1024\]|K in \[2, 1024\]"):
            d3pm_q_sample_rot(sch, idx[:4], idx[:4], t[:4], K_bad, noise_x=torch.rand(4, K_bad, device=dev), noise_rot=torch.rand(4, 4, device=dev))
        with pytest.raises(_lib.DaError, match=r"outside \[2, 1024\]|K in \[2, 1024\]"):
            d3pm_rot_loss(sch, torch.zeros(4, K_bad, device=dev), torch.zeros(4, 4, device=dev), idx[:4], idx[:4], idx[:4], idx[:4], t[:4])
    te.w.c_out = 1025
    assert lib.da_train_workspace_bytes_ex(C.byref(te.w), C.byref(g), 0) == 0 and b"outside [2, 1024]" in lib.da_last_error()
    te.w.c_out = K
    # CPU tensors
    with pytest.raises(_lib.DaError, match="needs ROCm tensors"):
        d3pm_rot_loss(sch, torch.zeros(4, 8), torch.zeros(4, 4), idx[:4].cpu(), idx[:4].cpu(), idx[:4].cpu(), idx[:4].cpu(), t[:4].cpu())
    with pytest.raises(_lib.DaError, match="needs ROCm tensors"):
        d3pm_q_sample_rot(sch, idx[:4].cpu(), idx[:4].cpu(), t[:4].cpu(), 8, noise_x=torch.rand(4, 8), noise_rot=torch.rand(4, 4))
    # training reads one feature image
    with pytest.raises(ValueError, match="one feature image"):
        mr.forward_with_feats(idx.long(), None, t, None, c["edge_index"].to(dev), torch.zeros(4, N, 1088, device=dev), c["batch"].to(dev))
    with pytest.raises(ValueError, match="one feature image"):
        mr.forward_with_feats(idx.long(), None, t, None, c["edge_index"].to(dev), feats, c["batch"].to(dev), rot_acc=idx.long())
