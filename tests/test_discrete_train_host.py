"""Host tests of the discrete position model's training side (no GPU): the fp64 restatements of discrete_train_cases.py against
the reference's own p_losses + backward (golden_v8.npz, make_golden_v8.py), their analytic gradient against autograd, the
q_sample cases of the GPU tests, the flat parameter layout and the ABI.

Bounds.  x_noisy: equal (the fixture's seeds keep every top-2 gap >= 1e-3).  Loss: 5 x the deviation the generator measured and
stored (golden_v7's rule).  Gradients: per tensor GTOL / 4 with GTOL = 1e-3 of test_gpu_train*.py and its 1e-4 x max floor -- the
generator measured 8.2e-5 at worst, which leaves the GPU tests their margin."""
import os
import re

import numpy as np
import pytest
import torch

import discrete_cases as DC
import discrete_train_cases as DT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GTOL = 1e-3
NEW_SYMBOLS = ("da_d3pm_q_sample", "da_d3pm_loss", "da_d3pm_noise_ex", "da_train_forward_idx", "da_train_backward_idx")


@pytest.fixture(scope="module")
def g8():
    return DT.load_golden8()


@pytest.fixture(scope="module")
def case():
    return DC.v7_case()


def fp64_step(spec, g8, case):
    """The fixture case evaluated by the restatements in fp64 with autograd: (x_t, gap, loss, {name: grad})."""
    name = spec["name"]
    x_start, t = DT.v8_inputs(spec)
    ac = DC.linear_alphas_cumprod(DT.V8["steps"])
    x_t, gap = DT.q_sample(ac, x_start, t, torch.from_numpy(g8[f"{name}/uniforms"]), DT.V8["K"])
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in case["sd"].items()}
    keep = (torch.from_numpy(g8[f"{name}/cfg_rand"])[case["batch"]] > spec["cfg_prob"]).double()
    logits = DC.forward_with_feats(sdg, x_t, t, case["edge_index"], keep[:, None] * case["feats"].double())
    loss = DT.loss(ac, logits, x_start, x_t, t, spec["kind"], DT.V8["lambda_loss"])
    loss.backward()
    return x_t, gap, loss.detach(), {k: v.grad for k, v in sdg.items()}


@pytest.mark.parametrize("spec", DT.V8_CASES, ids=lambda s: s["name"])
def test_restatement_reproduces_the_reference_step(spec, g8, case):
    name = spec["name"]
    x_start, t = DT.v8_inputs(spec)
    assert torch.equal(x_start, torch.from_numpy(g8[f"{name}/x_start"])) and torch.equal(t, torch.from_numpy(g8[f"{name}/t"]))
    for lo in range(0, x_start.numel(), DT.V8["K"]):
        assert sorted(x_start[lo:lo + DT.V8["K"]].tolist()) == list(range(DT.V8["K"]))          # a permutation per puzzle
    x_t, gap, loss, grads = fp64_step(spec, g8, case)
    assert float(gap.min()) >= DC.GAP and abs(float(gap.min()) - float(g8[f"{name}/min_gap"])) < 1e-9
    assert torch.equal(x_t, torch.from_numpy(g8[f"{name}/x_noisy"]))
    if spec["cfg_prob"] > 0:
        kept = torch.from_numpy(g8[f"{name}/cfg_rand"]) > spec["cfg_prob"]
        assert int(kept.sum()) == 1 and kept.numel() == 2                                       # one puzzle masked, one kept
    ref = float(g8[f"{name}/loss"])
    dev = abs(float(loss) - ref) / abs(ref)
    print(f"{name}: loss {float(loss):.8f} vs reference {ref:.8f}: rel {dev:.3e} (recorded {float(g8[f'{name}/dev_loss']):.3e})")
    assert dev <= 5 * float(g8[f"{name}/dev_loss"])
    names = [str(k) for k in g8["param_names"]]
    assert sorted(names) == sorted(case["sd"])
    heads = {k: torch.from_numpy(g8[f"{name}/grad_head/{k}"]).double() for k in names}
    stats = {k: g8[f"{name}/grad_stats/{k}"] for k in names}
    floor = 1e-4 * max(float(g.abs().max()) for g in grads.values())
    worst = ("", 0.0)
    for k in names:
        got = grads[k].flatten()[:64]
        scale = max(float(grads[k].abs().max()), floor)
        e = float((got - heads[k]).abs().max()) / scale
        worst = max(worst, (k, e), key=lambda p: p[1])
        assert e <= GTOL / 4, (k, e)
        if float(stats[k][1]) > floor * grads[k].numel() * 1e-2:
            e1 = abs(float(grads[k].abs().sum()) - float(stats[k][1])) / float(stats[k][1])
            e2 = abs(float((grads[k] ** 2).sum()) - float(stats[k][2])) / float(stats[k][2])
            assert e1 <= GTOL / 4 and e2 <= GTOL / 2, (k, e1, e2)
    print(f"{name}: worst gradient head {worst[0]} {worst[1]:.3e} (recorded worst {float(g8[f'{name}/dev_grad'].max()):.3e})")
    assert float(g8[f"{name}/dev_grad"].max()) <= GTOL / 4


@pytest.mark.parametrize("K", [2, 36, 144])
@pytest.mark.parametrize("kind", DT.KINDS)
def test_analytic_gradient_equals_fp64_autograd(K, kind):
    """d / dz of the restated losses by the closed formulas against autograd, relative 1e-9; rows with t = 0, 1, mid, steps - 1,
    x_t == x0 and x_t != x0, at logit scales 3 and 30."""
    steps = 100
    ac = DC.linear_alphas_cumprod(steps)
    for scale in (3.0, 30.0):
        logits, x0, xt, t = DT.row_mix(24, K, steps, seed=K + int(scale), scale=scale)
        assert set(t.tolist()) == {0, 1, steps // 2, steps - 1}
        assert bool((xt == x0).any()) and bool((xt != x0).any())
        z = logits.double().requires_grad_(True)
        DT.loss(ac, z, x0, xt, t, kind).backward()
        got = DT.d_logits(ac, logits.double(), x0, xt, t, kind)
        err = float((got - z.grad).abs().max()) / float(z.grad.abs().max())
        print(f"K={K} {kind} scale {scale}: analytic vs autograd {err:.3e}")
        assert bool(torch.isfinite(got).all()) and err <= 1e-9


@pytest.mark.parametrize("K", DT.Q_KS)
@pytest.mark.parametrize("n", DT.Q_NS)
def test_q_sample_cases_are_clear_of_ties(K, n):
    x0, t, u = DT.q_sample_case(n, K, DT.Q_STEPS, DT.Q_SEEDS[(K, n)])
    assert set(t.tolist()) <= {0, 1, DT.Q_STEPS // 2, DT.Q_STEPS - 1} and (n < 4 or len(set(t.tolist())) == 4)
    _, gap = DT.q_sample(DC.linear_alphas_cumprod(DT.Q_STEPS), x0, t, u, K)
    assert float((gap < DC.GAP).double().mean()) <= DC.GAP_CAP, (K, n, int((gap < DC.GAP).sum()))


def test_q_sample_restatement_marginal():
    """The restated noising draws x_t == x0 with probability a_t + (1 - a_t) / K (Gumbel-max over the row of overline_Q[t])."""
    K, steps, n = 6, 100, 40000
    ac = DC.linear_alphas_cumprod(steps)
    gen = torch.Generator().manual_seed(11)
    x0 = torch.randint(0, K, (n,), generator=gen)
    t = torch.full((n,), 60, dtype=torch.long)
    x_t, _ = DT.q_sample(ac, x0, t, torch.rand(n, K, generator=gen), K)
    want = float(ac[60]) + (1 - float(ac[60])) / K
    assert abs(float((x_t == x0).double().mean()) - want) < 4 * (want * (1 - want) / n) ** 0.5


def _discrete_backbone():
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete
    return Eff_GAT_Discrete(steps=20, input_channels=36, output_channels=36)


def test_param_order_covers_exactly_the_discrete_parameters():
    from diffassemble_amd.train import _param_order
    m = _discrete_backbone()
    names, n_layers = _param_order(m)
    own = [k for k, _ in m.named_parameters() if not k.startswith("visual_backbone.")]
    assert n_layers == 4 and len(names) == len(set(names)) and sorted(names) == sorted(own)
    assert "pos_mlp.weight" in names and not any(k.startswith(("pos_mlp.0", "pos_mlp.2")) for k in names)
    shapes = dict(m.named_parameters())
    assert tuple(shapes["pos_mlp.weight"].shape) == (36, 32) and tuple(shapes["final_mlp.2.weight"].shape) == (36, 32)
    # the 2D layout is what it was
    from diffassemble_amd.model.backbones import Eff_GAT
    n2, _ = _param_order(Eff_GAT(steps=20))
    assert n2[:5] == ["time_emb.weight", "pos_mlp.0.weight", "pos_mlp.0.bias", "pos_mlp.2.weight", "pos_mlp.2.bias"]


def test_new_prototypes_are_declared_and_the_abi_is_19():
    from diffassemble_amd import _lib
    header = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define\s+DA_ABI_VERSION\s+19\b", header) and _lib.ABI_VERSION == 19
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _lib.PROTOTYPES, sym
        proto = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.PROTOTYPES[sym][1]), sym
    declared = set(re.findall(r"\b(da_[a-z0-9_]+)\s*\(", header))
    assert set(_lib.PROTOTYPES) <= declared


def test_training_methods_refuse_cpu_tensors_with_the_documented_message():
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=20, sampling="DDPM", scheduler=SD.ModelScheduler.LINEAR, loss_type="hybrid")
    z = torch.zeros(4, dtype=torch.long)
    for call in (lambda: m.q_sample(z, z), lambda: m.p_losses(z, z, loss_type="vb"), lambda: m.vb_terms_bpd(torch.zeros(4, 36), None, z, z, z),
                 lambda: m.training_step(None, 0)):
        with pytest.raises(NotImplementedError, match="discrete training is not built yet.*on ROCm tensors only"):
            call()
