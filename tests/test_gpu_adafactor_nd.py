"""FusedAdafactorND / da_adafactor_nd_step (diffassemble_amd/csrc/da_optim_nd.hip) against transformers.optimization.Adafactor,
the optimizer the reference configures (spatial_diffusion.py:701-705), for tensors of any rank addressed by pointer.

Parity rule (every tensor, every step, parameter and each state tensor, no element excluded): with the reference run in fp64 on
the CPU, ``e_got = max|got - ref64|`` and ``e_ref = max|ref32 - ref64|`` (transformers' own fp32 CPU run),

    e_got <= 16 * e_ref + 4 * 2^-24 * max|ref64|

-- the repository's per-kernel rule (tests/test_gpu_encoder_train_kernels.py): 16 leaves room for a different summation order; a
wrong clip, learning rate or factor moves a parameter by >= 1e-4 of its magnitude and fails by orders of magnitude.

Shapes: the smallest that reach every code path of the kernels -- a P4 bank, the stem with a singleton dimension, a 1x1 shortcut
(tiny slices, one lane each; 3x3 and 1x1 have their own instances), R = 1 and C = 1 slices (the generic tiny path), (70, 4100): more
than one column chunk, not a multiple of 64 or 4, several row blocks with a ragged last one, (3, 16384): the full width, a vector
crossing the 4096-element block and a one-element vector.  Planted: one 3x3 slice with an exactly zero gradient, one all-zero
parameter (learning-rate floor eps2), one parameter without a gradient at step 1 only."""
import copy

import numpy as np
import pytest
import torch

from oracle import encoder as OE
from oracle import weights as W

pytestmark = pytest.mark.gpu

SHAPES = [(8, 4, 4, 3, 3), (8, 3, 1, 3, 3), (8, 4, 4, 1, 1), (5, 1, 7), (3, 1), (1, 9), (70, 4100), (3, 16384), (32,), (4097,), (1,)]
ZERO_PARAM, SKIPPED = 3, 1            # (5, 1, 7) is all zeros; (8, 3, 1, 3, 3) has no gradient at step 1 (0-based)
SCALES = (1.0, 0.1, 0.01)
STATE_KEYS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "RMS")
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


def make_inputs():
    g = torch.Generator().manual_seed(20260)
    params = [torch.randn(s, generator=g) for s in SHAPES]
    params[ZERO_PARAM].zero_()
    grads = []
    for step, sc in enumerate(SCALES):
        gs = [torch.randn(s, generator=g) * sc for s in SHAPES]
        gs[0][0, 0, 0].zero_()                       # one 3x3 slice with an exactly zero gradient
        if step == 1:
            gs[SKIPPED] = None
        grads.append(gs)
    return params, grads


def snapshot(params, sd):
    st = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in sd["state"].items()}
    return [p.detach().cpu().clone() for p in params], st


def run_transformers(params, grads_per_step, dtype, load=None):
    """transformers' Adafactor on CPU copies in ``dtype``; ``load``: a state dict to resume from.  One snapshot per step."""
    from transformers.optimization import Adafactor
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    opt = Adafactor(ps)
    if load is not None:
        opt.load_state_dict(copy.deepcopy(load))
    out = []
    for gs in grads_per_step:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().cpu().to(dtype).clone()
        opt.step()
        out.append(snapshot(ps, opt.state_dict()))
    return out, opt


def make_fused(params, dev, load=None):
    from diffassemble_amd.train import FusedAdafactorND
    ps = [torch.nn.Parameter(p.detach().to(dev, torch.float32).clone()) for p in params]
    opt = FusedAdafactorND(ps)
    if load is not None:
        opt.load_state_dict(load)
    return ps, opt


def run_fused(params, grads_per_step, dev, load=None):
    ps, opt = make_fused(params, dev, load)
    out = []
    for gs in grads_per_step:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.detach().to(dev, torch.float32).clone()
        opt.step()
        out.append(snapshot(ps, opt.state_dict()))
    return out, ps, opt


def rule1(what, got, ref64, ref32):
    got, ref64, ref32 = (torch.as_tensor(x).detach().cpu().double() for x in (got, ref64, ref32))
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), what
    e_got = float((got - ref64).abs().max())
    e_ref = float((ref32 - ref64).abs().max())
    bound = 16 * e_ref + 4 * 2.0 ** -24 * float(ref64.abs().max())
    if e_ref > 0:
        WORST["ratio"] = max(WORST["ratio"], e_got / e_ref)
    print(f"{what}: e_got {e_got:.3e} e_ref {e_ref:.3e} bound {bound:.3e} ratio {e_got / e_ref if e_ref > 0 else float('nan'):.2f}")
    assert e_got <= bound, (what, e_got, e_ref, bound)


def compare_snapshots(tag, got, ref64, ref32, names=None):
    (gp, gs), (rp, rs), (fp, fs) = got, ref64, ref32
    assert set(gs) == set(rs) == set(fs), (tag, sorted(gs), sorted(rs))
    for i in range(len(gp)):
        name = names[i] if names else f"{tuple(gp[i].shape)}"
        rule1(f"{tag} param {i} {name}", gp[i], rp[i], fp[i])
        if i not in rs:
            continue
        assert gs[i]["step"] == rs[i]["step"], (tag, i, gs[i]["step"], rs[i]["step"])
        assert {k for k in gs[i] if k != "step"} == {k for k in rs[i] if k != "step"}, (tag, i, sorted(gs[i]), sorted(rs[i]))
        for k in STATE_KEYS:
            if k in rs[i]:
                rule1(f"{tag} {k} {i} {name}", gs[i][k], rs[i][k], fs[i][k])
    print(f"worst e_got / e_ref so far: {WORST['ratio']:.2f}")


@pytest.fixture(scope="module")
def reference():
    params, grads = make_inputs()
    return params, grads, run_transformers(params, grads, torch.float64)[0], run_transformers(params, grads, torch.float32)[0]


def test_parity_every_tensor_every_step(dev, reference):
    params, grads, ref64, ref32 = reference
    got, _, _ = run_fused(params, grads, dev)
    for s in range(3):
        compare_snapshots(f"step {s + 1}", got[s], ref64[s], ref32[s])
        for i, shape in enumerate(SHAPES):          # transformers' state layout
            if i not in got[s][1]:
                continue
            st = got[s][1][i]
            if len(shape) >= 2:
                assert st["exp_avg_sq_row"].shape == shape[:-1] and st["exp_avg_sq_col"].shape == shape[:-2] + shape[-1:]
            else:
                assert st["exp_avg_sq"].shape == shape
            assert st["RMS"].dim() == 0


def test_per_tensor_step_count(dev, reference):
    params, grads, ref64, ref32 = reference
    got, ps, opt = run_fused(params, grads, dev)
    assert torch.equal(got[1][0][SKIPPED], got[0][0][SKIPPED])                 # bit-unchanged by the step it sat out
    for k in ("exp_avg_sq_row", "exp_avg_sq_col"):
        assert torch.equal(got[1][1][SKIPPED][k], got[0][1][SKIPPED][k])
    steps = {i: s["step"] for i, s in opt.state_dict()["state"].items()}
    assert steps == {i: (2 if i == SKIPPED else 3) for i in range(len(SHAPES))}
    assert opt.steps_dev.cpu().tolist() == [steps[i] for i in range(len(SHAPES))]
    rule1("skipped parameter after three steps", got[2][0][SKIPPED], ref64[2][0][SKIPPED], ref32[2][0][SKIPPED])
    for k in ("exp_avg_sq_row", "exp_avg_sq_col"):
        rule1(f"skipped parameter {k}", got[2][1][SKIPPED][k], ref64[2][1][SKIPPED][k], ref32[2][1][SKIPPED][k])


def test_two_runs_are_bit_identical(dev, reference):
    params, grads, _, _ = reference
    a, _, _ = run_fused(params, grads, dev)
    b, _, _ = run_fused(params, grads, dev)
    for x, y in zip(a[2][0], b[2][0]):
        assert torch.equal(x, y)
    for i in a[2][1]:
        for k, v in a[2][1][i].items():
            assert torch.equal(v, b[2][1][i][k]) if torch.is_tensor(v) else v == b[2][1][i][k], (i, k)


def test_checkpoint_moves_both_ways(dev, reference):
    params, grads, _, _ = reference
    # fused -> transformers: two fused steps, then the third step with each implementation from the fused checkpoint
    ps, opt = make_fused(params, dev)
    for gs in grads[:2]:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(dev)
        opt.step()
    sd = opt.state_dict()
    at2 = [p.detach().cpu().clone() for p in ps]
    assert sd["state"][SKIPPED]["step"] == 1 and sd["state"][0]["step"] == 2
    ref64, _ = run_transformers(at2, grads[2:], torch.float64, load=sd)
    ref32, _ = run_transformers(at2, grads[2:], torch.float32, load=sd)
    for p, g in zip(ps, grads[2]):
        p.grad = g.to(dev)
    opt.step()
    compare_snapshots("fused -> transformers", snapshot(ps, opt.state_dict()), ref64[0], ref32[0])
    # transformers -> fused: two transformers steps (fp32, CPU), then the third step with each implementation from its checkpoint
    two, topt = run_transformers(params, grads[:2], torch.float32)
    tsd = topt.state_dict()
    ref64, _ = run_transformers(two[1][0], grads[2:], torch.float64, load=tsd)
    ref32, _ = run_transformers(two[1][0], grads[2:], torch.float32, load=tsd)
    got, _, fopt = run_fused(two[1][0], grads[2:], dev, load=tsd)
    compare_snapshots("transformers -> fused", got[0], ref64[0], ref32[0])
    assert fopt.state_dict()["state"][SKIPPED]["step"] == 2


def test_version_counters(dev, reference):
    params, grads, _, _ = reference
    ps, opt = make_fused(params, dev)
    for p, g in zip(ps, grads[1]):                   # the step in which SKIPPED has no gradient
        p.grad = None if g is None else g.to(dev)
    before = [p._version for p in ps]
    opt.step()
    for i, p in enumerate(ps):
        assert (p._version == before[i]) if i == SKIPPED else (p._version > before[i]), i


def test_replaced_parameter_storage_is_followed(dev, reference):
    """The kernels write through raw addresses: a parameter whose storage is replaced after construction (``p.data = ...``, what
    ``module.to(...)`` does) must be updated in its NEW storage, and the old one left alone."""
    params, grads, ref64, ref32 = reference
    ps, opt = make_fused(params, dev)
    old = [p.data for p in ps]
    for p in ps:
        p.data = p.data.clone()
    kept = [o.clone() for o in old]
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt.step()
    for i, p in enumerate(ps):
        assert torch.equal(old[i], kept[i]), i
        rule1(f"moved param {i}", p, ref64[0][0][i], ref32[0][0][i])


def test_step_does_not_synchronise_with_the_host(dev, reference):
    """After one warm step (tables uploaded, gradient addresses unchanged) ``step()`` is one library call and nothing that
    waits for the device: torch's sync debug mode raises on any synchronising call made through torch."""
    from diffassemble_amd import _lib
    params, grads, _, _ = reference
    ps, opt = make_fused(params, dev)
    for p, g in zip(ps, grads[0]):
        p.grad = g.to(dev)
    opt.step()
    torch.cuda.synchronize()
    calls = []
    real = opt.lib.da_adafactor_nd_step

    class Counting:
        def __getattr__(self, name):
            if name == "da_adafactor_nd_step":
                return lambda *a: (calls.append(name), real(*a))[1]
            calls.append(name)
            return getattr(_lib.lib(), name)

    opt.lib = Counting()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert calls == ["da_adafactor_nd_step"]
    torch.cuda.synchronize()
    assert opt.steps_dev.cpu().tolist() == [2] * len(SHAPES)


def _encoder_trainables(sd):
    return [(k, v) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point() and "running" not in k]


def test_real_encoder_parameter_list(dev):
    """One step over the piece encoder's real parameter list (the shapes of oracle.weights.make_encoder_state: the 5-D banks,
    BatchNorm affines, linear1 [544, 16384], linear2 [544, 8192]; about 13 M values) with seeded normal gradients."""
    named = _encoder_trainables(W.make_encoder_state(5))
    names = [k for k, _ in named]
    params = [v.float().contiguous() for _, v in named]
    assert any(tuple(p.shape) == (544, 16384) for p in params) and any(p.dim() == 5 for p in params)
    g = torch.Generator().manual_seed(77)
    grads = [[torch.randn(p.shape, generator=g) * 0.05 for p in params]]
    ref64, _ = run_transformers(params, grads, torch.float64)
    ref32, _ = run_transformers(params, grads, torch.float32)
    got, _, _ = run_fused(params, grads, dev)
    compare_snapshots("encoder", got[0], ref64[0], ref32[0], names)


def test_whole_model_step_and_eval_on_the_updated_weights(dev):
    """configure_optimizers() with a trainable piece encoder: one step of the whole model from pixels (one 2x2 puzzle), every
    trainable tensor against transformers' Adafactor fed the SAME gradients (cloned after backward: the optimizer alone, not the
    backward's chaotic slices); then eval() must run on the updated weights (packed-weight caches key on the version counter)."""
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    T, n = 100, 4
    m = GNN_Diffusion(steps=T, sampling="DDIM", rotation=True, model_mean_type=ModelMeanType.EPSILON,
                      visual_pretrained=False, backbone="resnet18equiv", freeze_backbone=False)
    dsd, esd = W.make_denoiser_state(T, 4, 4, seed=41), W.make_encoder_state(41)
    m.model.load_state_dict({**dsd, **{"visual_backbone." + k: v for k, v in esd.items()}}, strict=False)
    m = m.to(dev).train()
    m.model.precision = "fp32"
    opt = m.configure_optimizers()
    assert type(opt).__name__ == "HybridAdafactor" and type(opt.rest).__name__ == "FusedAdafactorND"
    rng = np.random.default_rng(9)
    x0 = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32))
    noise = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32))
    t = torch.full((n,), 17, dtype=torch.int64)
    patches = W.make_patches(n, 12)
    ei, batch = W.dense_edge_index(n, True), torch.zeros(n, dtype=torch.int64)
    opt.zero_grad()
    loss = m.p_losses(x0.to(dev), t.to(dev), noise=noise.to(dev), loss_type="huber", cond=patches.to(dev),
                      edge_index=ei.to(dev), batch=batch.to(dev))
    loss.backward()
    named = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    before = [p.detach().cpu().clone() for _, p in named]
    grads = [[None if p.grad is None else p.grad.detach().cpu().clone() for _, p in named]]
    assert sum(g is not None for g in grads[0]) > 60 and any(g is not None and g.dim() == 5 for g in grads[0])
    # an eval-mode pass BEFORE the step: the inference engine now holds weights packed from the old parameters (the training
    # engine's pack exists since p_losses), so the eval after the step is right only if the step invalidates those caches
    m.eval()
    f_old = m.model.visual_features(patches.to(dev)).detach().clone()
    m.train()
    opt.step()
    torch.cuda.synchronize()
    ref64, _ = run_transformers(before, grads, torch.float64)
    ref32, _ = run_transformers(before, grads, torch.float32)
    for i, (k, p) in enumerate(named):
        if grads[0][i] is None:
            assert torch.equal(p.detach().cpu(), before[i]), k
        else:
            assert not torch.equal(p.detach().cpu(), before[i]), k
            rule1(f"model {k}", p, ref64[0][0][i], ref32[0][0][i])
    print(f"worst e_got / e_ref so far: {WORST['ratio']:.2f}")
    m.eval()
    f_eval = m.model.visual_features(patches.to(dev))
    sd_now = {k: v.detach().cpu() for k, v in m.model.visual_backbone.state_dict().items()}
    ref = OE.visual_features(sd_now, patches)
    err = float((f_eval.detach().double().cpu() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))
    print(f"eval features on the updated weights: rel err {err:.3e}")
    assert err < 1e-4
    assert not torch.equal(f_eval, f_old)                 # (the step moved the features: a stale pack would have reproduced f_old)
    # and the training engine's pack: a second train-mode forward runs on the updated weights
    m.train()
    stats = {}
    f_train = m.model.visual_features(patches.to(dev))
    ref_t = OE.visual_features({k: v.clone() for k, v in sd_now.items()}, patches, stats=stats)
    err_t = float((f_train.detach().double().cpu() - ref_t.double()).abs().max() / (ref_t.double().abs().max() + 1e-30))
    print(f"train-mode features on the updated weights: rel err {err_t:.3e}")
    assert err_t < 1e-4
