"""GPU tests of the discrete position model's training side: da_d3pm_q_sample and da_d3pm_loss on their own, the discrete
denoiser's training forward + backward against fp64 autograd, p_losses against the reference's own step (golden_v8.npz,
make_golden_v8.py), one training_step + optimizer step, and the guards of the C entries.

Bounds.  The per-piece fp32 kernels follow test_gpu_train3d.py's rule (``within_4x``): at most 4x the error of the same
expression evaluated by torch in fp32 against fp64, in max-abs terms scaled by the largest element, floored at 16 fp32 ulps.
Argmax outputs are compared where the fp64 top-2 gap is >= 1e-3 (discrete_cases.check_argmax; the cases are asserted clear of
ties by tests/test_discrete_train_host.py).  The denoiser keeps test_gpu_train.py's bounds (output 1e-4, gradients and d_feats
GTOL = 1e-3 with the 1e-4 x max floor), the fixture comparison test_gpu_train3d.py's three checks; the bf16-operand mode is held to
4x the error the restatement itself shows against the fixture under torch.autocast("cpu", bfloat16), never tighter than the
bounds test_gpu_train3d.py documents for that mode (loss 5e-3; heads 2.5e-2, |g| sum 1.5e-2, g^2 sum 2e-2)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import discrete_cases as DC
import discrete_train_cases as DT

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
def g8():
    return DT.load_golden8()


def within_4x(name, hip, f32, f64):
    scale = float(f64.abs().max())
    e32 = float((f32.double() - f64).abs().max()) / scale
    ehip = float((hip.double().cpu() - f64).abs().max()) / scale
    print(f"{name}: scale {scale:.3e}  torch-fp32 err {e32:.3e}  HIP err {ehip:.3e}")
    assert math.isfinite(ehip) and ehip <= max(4 * e32, ULP16), (name, e32, ehip)


def schedule(dev, steps):
    from diffassemble_amd.engine import Schedule
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[(2, 2)], steps=steps, sampling="DDPM", scheduler=SD.ModelScheduler.LINEAR)
    assert torch.equal(m.alphas_cumprod, DC.linear_alphas_cumprod(steps))
    return Schedule({k: getattr(m, k) for k in Schedule.KEYS}, dev)


_SCHED = {}


def sched_for(dev, steps):
    if steps not in _SCHED:
        _SCHED[steps] = schedule(dev, steps)
    return _SCHED[steps]


# ------------------------------------------------------------------------------------------------ da_d3pm_q_sample
@pytest.mark.parametrize("n", DT.Q_NS)
@pytest.mark.parametrize("K", DT.Q_KS)
def test_q_sample_against_the_fp64_restatement(dev, K, n):
    from diffassemble_amd.engine import d3pm_noise, d3pm_q_sample
    steps = DT.Q_STEPS
    x0, t, u = DT.q_sample_case(n, K, steps, DT.Q_SEEDS[(K, n)])
    sch = sched_for(dev, steps)
    ac = DC.linear_alphas_cumprod(steps)
    want, gap = DT.q_sample(ac, x0, t, u, K)
    got = d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, noise=u.to(dev))
    assert got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < K
    DC.check_argmax(got, want, gap, f"q_sample K={K} n={n}")
    # the seeded route draws the uniforms of the TRAINING domain inside the kernel: bit-equal to the injected route fed by them,
    # and another stream than the sampling loop's iteration-0 draws of the same seed
    seed = torch.tensor([0x1234567 + K, 5 * n], dtype=torch.int64, device=dev)
    u_train, u_samp = d3pm_noise(seed, 0, n, K, domain="training"), d3pm_noise(seed, 0, n, K)
    assert float(u_train.min()) > 0.0 and float(u_train.max()) <= 1.0 and not torch.equal(u_train, u_samp)
    a = d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, seed=seed)
    assert torch.equal(a, d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, noise=u_train))
    assert torch.equal(a, d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, seed=seed))
    if n * K >= 63 * 35:            # (enough draws that two streams cannot agree by chance)
        assert not torch.equal(a, d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, noise=u_samp))
        assert not torch.equal(a, d3pm_q_sample(sch, x0.to(dev), t.to(dev), K, seed=seed, iteration=1))
    _, gap_t = DT.q_sample(ac, x0, t, u_train.cpu(), K)
    if float((gap_t < DC.GAP).double().mean()) <= DC.GAP_CAP:
        DC.check_argmax(a, DT.q_sample(ac, x0, t, u_train.cpu(), K)[0], gap_t, f"q_sample seeded K={K} n={n}")


def test_q_sample_marginal_of_the_seeded_route(dev):
    """20 000 pieces at t = 60: the share of x_t == x0 is a_t + (1 - a_t) / K within four standard errors."""
    from diffassemble_amd.engine import d3pm_q_sample
    K, steps, n = 36, 100, 20000
    x0 = torch.randint(0, K, (n,), device=dev)
    t = torch.full((n,), 60, dtype=torch.long, device=dev)
    seed = torch.tensor([77, 0], dtype=torch.int64, device=dev)
    x_t = d3pm_q_sample(sched_for(dev, steps), x0, t, K, seed=seed)
    a = float(DC.linear_alphas_cumprod(steps)[60])
    want = a + (1 - a) / K
    assert abs(float((x_t == x0).double().mean()) - want) < 4 * (want * (1 - want) / n) ** 0.5


# ------------------------------------------------------------------------------------------------ da_d3pm_loss
@pytest.mark.parametrize("n", DT.Q_NS)
@pytest.mark.parametrize("K", DT.Q_KS)
def test_loss_and_its_gradient_against_fp64(dev, K, n):
    from diffassemble_amd.engine import d3pm_loss
    steps = DT.Q_STEPS
    sch, ac = sched_for(dev, steps), DC.linear_alphas_cumprod(steps)
    logits, x0, xt, t = DT.row_mix(n, K, steps, seed=3 * K + n)
    on = [v.to(dev) for v in (logits, x0, xt, t)]
    for kind in DT.KINDS:
        z64 = logits.double().requires_grad_(True)
        l64 = DT.loss(ac, z64, x0, xt, t, kind)
        l64.backward()
        z32 = logits.clone().requires_grad_(True)
        l32 = DT.loss(ac, z32, x0, xt, t, kind)
        l32.backward()
        loss, d_logits, rows = d3pm_loss(sch, *on, kind=kind, lambda_loss=DT.LAMBDA)
        torch.cuda.synchronize()
        within_4x(f"loss K={K} n={n} {kind}", loss[:1], l32.detach().reshape(1), l64.detach().reshape(1))
        within_4x(f"d_logits K={K} n={n} {kind}", d_logits, z32.grad, z64.grad)
        vb64, ce64 = DT.loss_rows(ac, logits.double(), x0, xt, t)
        parts = loss.double().cpu()
        if kind != "cross_entropy":
            assert abs(float(parts[1]) - float(vb64.mean())) <= 1e-5 * max(1.0, abs(float(vb64.mean())))
            assert rel(rows[:, 0], vb64) < 1e-5
        if kind != "vb":
            assert abs(float(parts[2]) - float(ce64.mean())) <= 1e-5 * abs(float(ce64.mean()))
            assert rel(rows[:, 1], ce64) < 1e-5
        again = d3pm_loss(sch, *on, kind=kind, lambda_loss=DT.LAMBDA)
        assert torch.equal(again[0], loss) and torch.equal(again[1], d_logits)               # fixed summation order


@pytest.mark.parametrize("K", [2, 144, 1024])
def test_loss_is_finite_at_logit_scale_30(dev, K):
    from diffassemble_amd.engine import d3pm_loss
    steps, n = DT.Q_STEPS, 63
    sch, ac = sched_for(dev, steps), DC.linear_alphas_cumprod(steps)
    logits, x0, xt, t = DT.row_mix(n, K, steps, seed=K, scale=30.0)
    for kind in DT.KINDS:
        loss, d_logits, _ = d3pm_loss(sch, logits.to(dev), x0.to(dev), xt.to(dev), t.to(dev), kind=kind, lambda_loss=DT.LAMBDA)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d_logits).all())
        z64 = logits.double().requires_grad_(True)
        l64 = DT.loss(ac, z64, x0, xt, t, kind)
        l64.backward()
        z32 = logits.clone().requires_grad_(True)
        DT.loss(ac, z32, x0, xt, t, kind).backward()
        within_4x(f"scale 30 d_logits K={K} {kind}", d_logits, z32.grad, z64.grad)
        assert abs(float(loss[0]) - float(l64.detach())) <= 1e-4 * abs(float(l64.detach()))


# ------------------------------------------------------------------------------------------------ denoiser forward + backward
def make_backbone(c, dev):
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete
    m = Eff_GAT_Discrete(steps=c["steps"], input_channels=c["K"], output_channels=c["K"])
    missing, unexpected = m.load_state_dict(c["sd"], strict=False)
    assert not unexpected and all(k in ("mean", "std") or k.startswith("visual_backbone.") for k in missing)
    return m.to(dev).train()


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("key", DT.DENOISER_CASES)
def test_denoiser_backward_matches_fp64_autograd(dev, key, staged):
    c = DT.denoiser_case(key)
    m = make_backbone(c, dev)
    te = m.train_engine(dev)
    te.force_staged = staged
    assert te.variant == "discrete" and te.c_out == c["K"] and te.c_in == 1

    def run():
        m.zero_grad(set_to_none=True)
        feats = c["feats"].to(dev).requires_grad_(True)
        out, att = m.forward_with_feats(c["idx"].to(dev), c["t"].to(dev), None, c["edge_index"].to(dev), feats, c["batch"].to(dev))
        assert att is None and out.requires_grad and out.shape == c["logits"].shape
        (out * c["functional"].to(dev)).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), feats.grad

    out, d_feats = run()
    e_out = rel(out, c["logits"])
    print(f"{key}: logits rel err {e_out:.3e}")
    assert e_out < 1e-4
    params = dict(m.named_parameters())
    floor = 1e-4 * max(float(g.abs().max()) for g in c["grads"].values())
    errs = {}
    for k, gr in c["grads"].items():
        assert params[k].grad is not None, k
        errs[k] = float((params[k].grad.detach().double().cpu() - gr).abs().max()) / max(float(gr.abs().max()), floor)
    e_f = rel(d_feats, c["d_feats"])
    worst = max(errs.items(), key=lambda p: p[1])
    print(f"{key}: worst gradient {worst[0]} {worst[1]:.3e}; pos_mlp.weight {errs['pos_mlp.weight']:.3e}; d_feats {e_f:.3e}")
    assert all(e < GTOL for e in errs.values()), {k: e for k, e in errs.items() if e >= GTOL}
    assert e_f < GTOL
    lo, hi = te.flat_grad.data_ptr(), te.flat_grad.data_ptr() + te.flat_grad.numel() * 4
    assert all(lo <= params[k].grad.data_ptr() < hi for k in c["grads"])
    # table rows no piece points at get no gradient; the embedding gradient is bit-reproducible
    unused = sorted(set(range(c["K"])) - set(c["idx"].tolist()))
    assert unused and float(params["pos_mlp.weight"].grad[unused].abs().max()) == 0.0
    first = params["pos_mlp.weight"].grad.detach().clone()
    run()
    assert torch.equal(first, params["pos_mlp.weight"].grad)


# ------------------------------------------------------------------------------------------------ p_losses vs golden_v8
def diffusion_module(spec, case, dev, steps=DT.V8["steps"], sizes=(6, 6)):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[sizes], steps=steps, sampling="DDPM", scheduler=SD.ModelScheduler.LINEAR, loss_type=spec["kind"],
                      lambda_loss=DT.V8["lambda_loss"], classifier_free_prob=spec["cfg_prob"])
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected
    return m.to(dev).train()


def fixture_step(spec, case, g8, dev, precision, staged=False):
    name = spec["name"]
    m = diffusion_module(spec, case, dev)
    te = m.model.train_engine(dev)
    te.precision = precision
    te.force_staged = staged
    x_start, t = DT.v8_inputs(spec)
    seen = {}
    inner = m.model.forward_with_feats

    def recording(x_noisy, *a, **k):
        seen["x_noisy"] = x_noisy.detach().clone()
        return inner(x_noisy, *a, **k)

    m.model.forward_with_feats = recording
    loss = m.p_losses(x_start.to(dev), t.to(dev), noise=torch.from_numpy(g8[f"{name}/uniforms"]).to(dev), loss_type=spec["kind"],
                      cond=None, edge_index=case["edge_index"].to(dev), batch=case["batch"].to(dev),
                      cfg_rand=torch.from_numpy(g8[f"{name}/cfg_rand"]).to(dev), patch_feats=case["feats"].to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return m, loss.detach(), seen["x_noisy"]


def fixture_errors(name, grads, g8, floor_rel, skip_rel):
    """test_gpu_train3d.py's three checks per tensor: (first 64 entries, |g| sum, g^2 sum) -> {tensor: (e0, e1 | None, e2 | None)}."""
    names = [str(k) for k in g8["param_names"]]
    floor = floor_rel * max(float(grads[k].abs().max()) for k in names)
    out = {}
    for k in names:
        g = grads[k].double().cpu()
        ref = torch.from_numpy(g8[f"{name}/grad_head/{k}"]).double()
        st_ref = g8[f"{name}/grad_stats/{k}"]
        e0 = float((g.flatten()[: ref.numel()] - ref).abs().max()) / max(float(ref.abs().max()), floor)
        if float(st_ref[1]) > floor * g.numel() * skip_rel:
            out[k] = (e0, abs(float(g.abs().sum()) - float(st_ref[1])) / float(st_ref[1]), abs(float((g * g).sum()) - float(st_ref[2])) / float(st_ref[2]))
        else:
            out[k] = (e0, None, None)
    return out


@pytest.mark.parametrize("staged", [False, True], ids=["all", "early_late"])
@pytest.mark.parametrize("spec", DT.V8_CASES, ids=lambda s: s["name"])
def test_p_losses_matches_the_reference_fixture(dev, g8, spec, staged):
    """The reference's own discrete p_losses + backward: x_noisy equal, the loss within 5x the deviation the fp64 closed form showed
    when the fixture was made (floored at 1e-5), then every live gradient's first 64 entries and its (|g| sum, g^2 sum)."""
    name = spec["name"]
    case = DC.v7_case()
    m, loss, x_noisy = fixture_step(spec, case, g8, dev, "fp32", staged)
    assert torch.equal(x_noisy.cpu().long(), torch.from_numpy(g8[f"{name}/x_noisy"]))
    ref = float(g8[f"{name}/loss"])
    e_loss = abs(float(loss) - ref) / abs(ref)
    bound = max(5 * float(g8[f"{name}/dev_loss"]), 1e-5)
    print(f"{name}: loss {float(loss):.7f} vs {ref:.7f}: rel {e_loss:.3e} (bound {bound:.2e})")
    assert e_loss <= bound
    assert abs(float(m.last_loss_parts[0]) - float(loss)) == 0.0
    grads = {k: p.grad for k, p in m.model.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(str(k) for k in g8["param_names"])
    errs = fixture_errors(name, grads, g8, 1e-4, 1e-2)
    worst = [max(e[i] for e in errs.values() if e[i] is not None) for i in range(3)]
    print(f"{name}: worst (head, |g| sum, g^2 sum) {worst}")
    for k, (e0, e1, e2) in errs.items():
        assert e0 < GTOL, (k, e0)
        assert e1 is None or (e1 < GTOL and e2 < 2 * GTOL), (k, e1, e2)


_AUTOCAST = {}


def autocast_errors(spec, case, g8):
    """The yardstick of the bf16-operand mode: the restatement evaluated under torch.autocast("cpu", bfloat16) (what the reference's
    Linear / matmul calls become under autocast) against the same fixture: (loss error, worst head, worst |g| sum, worst g^2 sum)."""
    name = spec["name"]
    if name in _AUTOCAST:
        return _AUTOCAST[name]
    x_start, t = DT.v8_inputs(spec)
    x_t = torch.from_numpy(g8[f"{name}/x_noisy"])
    sdg = {k: v.clone().requires_grad_(True) for k, v in case["sd"].items()}
    keep = (torch.from_numpy(g8[f"{name}/cfg_rand"])[case["batch"]] > spec["cfg_prob"]).float()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        logits = DC.forward_with_feats(sdg, x_t, t, case["edge_index"], keep[:, None] * case["feats"], dtype=torch.float32)
    loss = DT.loss(DC.linear_alphas_cumprod(DT.V8["steps"]), logits.float(), x_start, x_t, t, spec["kind"], DT.V8["lambda_loss"])
    loss.backward()
    ref = float(g8[f"{name}/loss"])
    errs = fixture_errors(name, {k: v.grad for k, v in sdg.items()}, g8, 1e-3, 1e-1)
    live = [e for e in errs.values() if e[1] is not None]
    _AUTOCAST[name] = (abs(float(loss.detach()) - ref) / abs(ref),) + tuple(max(e[i] for e in live) for i in range(3))
    return _AUTOCAST[name]


@pytest.mark.parametrize("spec", DT.V8_CASES, ids=lambda s: s["name"])
def test_p_losses_in_the_bf16_mode_vs_the_reference_fixture(dev, g8, spec):
    name = spec["name"]
    case = DC.v7_case()
    yard = autocast_errors(spec, case, g8)
    bounds = [max(4 * y, d) for y, d in zip(yard, (5e-3, 2.5e-2, 1.5e-2, 2e-2))]
    m, loss, x_noisy = fixture_step(spec, case, g8, dev, "bf16")
    assert torch.equal(x_noisy.cpu().long(), torch.from_numpy(g8[f"{name}/x_noisy"]))          # the noising is fp32 in both modes
    ref = float(g8[f"{name}/loss"])
    e_loss = abs(float(loss) - ref) / abs(ref)
    grads = {k: p.grad for k, p in m.model.named_parameters() if p.grad is not None}
    errs = fixture_errors(name, grads, g8, 1e-3, 1e-1)
    live = {k: e for k, e in errs.items() if e[1] is not None}                                  # (identically-zero gradients -- lin_key.bias -- are rounding noise)
    worst = [max(e[i] for e in live.values()) for i in range(3)]
    print(f"{name} bf16: loss rel {e_loss:.3e}; worst (head, |g| sum, g^2 sum) {worst} over {len(live)} tensors; autocast yardstick {yard}; bounds {bounds}")
    assert e_loss <= bounds[0]
    for k, e in live.items():
        assert e[0] <= bounds[1] and e[1] <= bounds[2] and e[2] <= bounds[3], (k, e)
    assert len(live) >= 12 and worst[0] > 1e-5                                                  # ... and the mode really is a different arithmetic


# ------------------------------------------------------------------------------------------------ one full step
def test_one_training_step_and_optimizer_step(dev):
    """training_step -> FusedAdafactor.step: the loss is logged, every parameter moved and is finite, and the update equals
    transformers' Adafactor applied on the host side to the same gradients (test_gpu_train.py's 2e-6)."""
    from types import SimpleNamespace
    from transformers.optimization import Adafactor
    from diffassemble_amd.train import FusedAdafactor
    case = DC.v7_case()
    spec = dict(kind="hybrid", cfg_prob=0.0)
    m = diffusion_module(spec, case, dev)
    logged = {}
    m.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v))
    N = case["feats"].shape[0]
    b = SimpleNamespace(batch=case["batch"].to(dev), edge_index=case["edge_index"].to(dev), patches=None,
                        indexes=(torch.arange(N) % 36 + 36).to(dev), patch_feats=case["feats"].to(dev))      # indexes % K is what trains
    opt = m.configure_optimizers()
    assert isinstance(opt, FusedAdafactor)
    te = m.model.train_engine(dev)
    assert te.variant == "discrete" and len(te.params) == len(case["sd"])
    torch.manual_seed(5)
    loss = m.training_step(b, 1)
    loss.backward()
    assert set(logged) == {"loss"} and math.isfinite(logged["loss"]) and abs(logged["loss"] - float(loss)) < 1e-6 * max(1.0, abs(float(loss)))
    ref_params = [torch.nn.Parameter(p.detach().clone()) for p in te.params]
    for rp, p in zip(ref_params, te.params):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        rp.grad = p.grad.detach().clone()
    before = te.flat.clone()
    opt.step()
    Adafactor(ref_params).step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(te.flat).all()) and not torch.equal(before, te.flat)
    for k, p, rp in zip(te.names, te.params, ref_params):
        assert rel(p, rp) < 2e-6, (k, rel(p, rp))
    # (lin_key.bias has an identically-zero gradient in exact arithmetic -- softmax is shift-invariant: it may stay where it was)
    still = [k for k, p in zip(te.names, te.params) if torch.equal(p.detach().cpu(), case["sd"][k]) and not k.endswith("lin_key.bias")]
    assert not still, still
    # a second draw of the same call noises differently (the seed is refilled from torch's generator per call)
    a = m.q_sample(b.indexes % 36, torch.full((N,), 60, device=dev))
    assert not torch.equal(a, m.q_sample(b.indexes % 36, torch.full((N,), 60, device=dev)))


# ------------------------------------------------------------------------------------------------ guards
def test_entries_reject_what_they_cannot_run(dev):
    from diffassemble_amd import _lib
    from diffassemble_amd.engine import d3pm_loss, d3pm_q_sample
    from diffassemble_amd.model.backbones import Eff_GAT
    lib = _lib.lib()
    c = DT.denoiser_case("dense36x2")
    md = make_backbone(c, dev)
    te = md.train_engine(dev)
    from diffassemble_amd.graph_plan import build_plan
    plan = build_plan(c["edge_index"].to(dev), c["batch"].to(dev), 0).with_source_csr()
    g, ws = te._cg(plan), te._workspace(plan)
    N, K = c["feats"].shape[0], c["K"]
    xf = torch.zeros((N, 2), device=dev)
    idx = torch.zeros(N, dtype=torch.int32, device=dev)
    t = torch.zeros(N, dtype=torch.int64, device=dev)
    feats = c["feats"].to(dev)
    out = torch.full((N, K), 7.0, device=dev)
    st = _lib.stream_ptr(dev)
    # a float-pose entry with discrete weights
    rc = lib.da_train_forward_ex(C.byref(te.w), C.byref(g), _lib.ptr(xf), _lib.ptr(t), _lib.ptr(feats), _lib.ptr(out), _lib.ptr(ws), ws.numel(), 0, st)
    assert rc != 0 and b"position indices" in lib.da_last_error()
    rc = lib.da_train_backward_stage(C.byref(te.w), C.byref(te.gw), C.byref(g), _lib.ptr(xf), _lib.ptr(t), _lib.ptr(out), None, _lib.ptr(ws), ws.numel(), 0, 0, st)
    assert rc != 0 and b"position indices" in lib.da_last_error()
    # an idx entry with 2D weights
    m2 = Eff_GAT(steps=20, visual_pretrained=False).to(dev).train()
    t2 = m2.train_engine(dev)
    ws2 = t2._workspace(plan)
    out2 = torch.zeros((N, 2), device=dev)
    rc = lib.da_train_forward_idx(C.byref(t2.w), C.byref(g), _lib.ptr(idx), _lib.ptr(t), _lib.ptr(feats), _lib.ptr(out2), _lib.ptr(ws2), ws2.numel(), 0, st)
    assert rc != 0 and b"not a discrete denoiser" in lib.da_last_error()
    rc = lib.da_train_backward_idx(C.byref(t2.w), C.byref(t2.gw), C.byref(g), _lib.ptr(idx), _lib.ptr(t), _lib.ptr(out2), None, _lib.ptr(ws2), ws2.numel(), 0, 0, st)
    assert rc != 0 and b"not a discrete denoiser" in lib.da_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0                                     # nothing was launched
    # K outside [2, 1024]
    sch = sched_for(dev, 100)
    for K_bad in (1, 1025):
        with pytest.raises(_lib.DaError, match=r"outside \[2, 1024\]|K in \[2, 1024\]"):
            d3pm_q_sample(sch, idx[:4], t[:4], K_bad, noise=torch.rand(4, K_bad, device=dev))
        with pytest.raises(_lib.DaError, match=r"outside \[2, 1024\]|K in \[2, 1024\]"):
            d3pm_loss(sch, torch.zeros(4, K_bad, device=dev), idx[:4], idx[:4], t[:4])
    te.w.c_out = 1025
    assert lib.da_train_workspace_bytes_ex(C.byref(te.w), C.byref(g), 0) == 0 and b"outside [2, 1024]" in lib.da_last_error()
    te.w.c_out = K
    with pytest.raises(_lib.DaError, match="needs ROCm tensors"):
        d3pm_loss(sch, torch.zeros(4, 8), idx[:4].cpu(), idx[:4].cpu(), t[:4].cpu())
