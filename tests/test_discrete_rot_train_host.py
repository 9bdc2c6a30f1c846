"""Host tests of the discrete position + rotation model's training side (no GPU): the fp64 restatements of
discrete_rot_train_cases.py against the reference's own p_losses + backward (golden_v10.npz, make_golden_v10.py), the noising cases
of the GPU tests, the flat parameter layout, the ABI and what happens off the device.

Bounds.  x_noisy / rot_noisy: equal (the fixture's seeds keep every top-2 gap of both noisings >= 1e-3).  Each loss: within the
deviation the generator measured and stored (1 % slack for the BLAS of another machine, floored at 1e-9).  Gradients: per tensor
GTOL / 4 with GTOL = 1e-3 of test_gpu_train*.py and its 1e-4 x max floor, as tests/test_discrete_train_host.py."""
import os
import re

import pytest
import torch

import discrete_cases as DC
import discrete_rot_cases as RC
import discrete_rot_train_cases as RT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GTOL = 1e-3
NEW_SYMBOLS = ("da_d3pm_q_sample_rot", "da_d3pm_rot_loss", "da_train_forward_rot", "da_train_backward_rot")
HEAD = ("final_mlp.0.weight", "final_mlp.0.bias", "final_mlp.2.weight", "final_mlp.2.bias")


@pytest.fixture(scope="module")
def g10():
    return RT.load_golden10()


@pytest.fixture(scope="module")
def case():
    return RC.v9_case()


@pytest.mark.parametrize("spec", RT.V10_CASES, ids=lambda s: s["name"])
def test_restatement_reproduces_the_reference_step(spec, g10, case):
    name, K = spec["name"], RT.V10["K"]
    x_start, rot_start, t = RT.v10_inputs(spec)
    for key, v in (("x_start", x_start), ("rot_start", rot_start), ("t", t)):
        assert torch.equal(v, torch.from_numpy(g10[f"{name}/{key}"])), key
    for lo in range(0, x_start.numel(), K):
        assert sorted(x_start[lo:lo + K].tolist()) == list(range(K))                            # a permutation per puzzle
    assert set(rot_start.tolist()) == {0, 1, 2, 3}
    ac = DC.linear_alphas_cumprod(RT.V10["steps"])
    u_x, u_rot = torch.from_numpy(g10[f"{name}/uniforms_x"]), torch.from_numpy(g10[f"{name}/uniforms_rot"])
    assert u_x.shape == (72, K) and u_rot.shape == (72, 4)
    x_t, gap_x, rot_t, gap_rot = RT.q_sample2(ac, x_start, rot_start, t, u_x, u_rot, K)
    gap = min(float(gap_x.min()), float(gap_rot.min()))
    assert gap >= DC.GAP and abs(gap - float(g10[f"{name}/min_gap"])) < 1e-9
    x_fed = x_start if spec["only_rot"] else x_t
    assert torch.equal(x_fed, torch.from_numpy(g10[f"{name}/x_noisy"])) and torch.equal(rot_t, torch.from_numpy(g10[f"{name}/rot_noisy"]))
    kept = torch.from_numpy(g10[f"{name}/cfg_rand"]) > spec["cfg_prob"]
    assert kept.numel() == 2 and int(kept.sum()) == (1 if spec["cfg_prob"] > 0 else 2)          # one puzzle masked in the cfg case
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in case["sd"].items()}
    feats = kept[case["batch"]].double()[:, None] * case["feats4"][0].double()
    logits, rot_logits = RC.forward_with_feats(sdg, x_fed, t, case["edge_index"], feats)
    x_loss, rot_loss = RT.losses(ac, None if spec["only_rot"] else logits, rot_logits, x_start, x_fed, rot_start, rot_t, t, spec["kind"],
                                 RT.V10["lambda_loss"])
    (rot_loss if x_loss is None else x_loss + rot_loss).backward()
    assert (f"{name}/x_loss" in g10) == (not spec["only_rot"]) and (x_loss is None) == spec["only_rot"]
    for key, got in (("x_loss", x_loss), ("rot_loss", rot_loss)):
        if got is None:
            continue
        ref, rec = float(g10[f"{name}/{key}"]), float(g10[f"{name}/dev_{key}"])
        dev = abs(float(got.detach()) - ref) / abs(ref)
        print(f"{name}: {key} {float(got.detach()):.8f} vs reference {ref:.8f}: rel {dev:.3e} (recorded {rec:.3e})")
        assert dev <= max(1.01 * rec, 1e-9)
    names = [str(k) for k in g10[f"{name}/param_names"]]
    assert sorted(names) == sorted(k for k in case["sd"] if not (spec["only_rot"] and k in HEAD)) and len(names) == (42 if spec["only_rot"] else 46)
    if spec["only_rot"]:
        assert all(sdg[k].grad is None for k in HEAD)
    grads = {k: sdg[k].grad for k in names}
    floor = 1e-4 * max(float(g.abs().max()) for g in grads.values())
    for k in names:
        st = g10[f"{name}/grad_stats/{k}"]
        e = float((grads[k].flatten()[:64] - torch.from_numpy(g10[f"{name}/grad_head/{k}"]).double()).abs().max()) / max(float(grads[k].abs().max()), floor)
        assert e <= GTOL / 4, (k, e)
        if float(st[1]) > floor * grads[k].numel() * 1e-2:
            e1 = abs(float(grads[k].abs().sum()) - float(st[1])) / float(st[1])
            e2 = abs(float((grads[k] ** 2).sum()) - float(st[2])) / float(st[2])
            assert e1 <= GTOL / 4 and e2 <= GTOL / 2, (k, e1, e2)
    assert g10[f"{name}/dev_grad"].shape == (len(names),) and float(g10[f"{name}/dev_grad"].max()) <= GTOL / 4


def test_smoothing_table_differs_from_the_position_model():
    """cross_entropy: neither head smoothed; hybrid: the position head only -- so the position module's weights cannot be reused."""
    import discrete_train_cases as DT
    ac = DC.linear_alphas_cumprod(100)
    z, x0, xt, rl, r0, rt, t = RT.row_mix(24, 36, 100, seed=5)
    z, rl = z.double(), rl.double()
    plain = lambda lo, y: float(torch.nn.functional.cross_entropy(lo, y))      # noqa: E731
    x, r = RT.losses(ac, z, rl, x0, xt, r0, rt, t, "cross_entropy")
    assert abs(float(x) - plain(z, x0)) < 1e-12 and abs(float(r) - plain(rl, r0)) < 1e-12
    assert abs(float(x) - float(DT.loss(ac, z, x0, xt, t, "cross_entropy"))) > 1e-4           # the position module smooths here
    xh, rh = RT.losses(ac, z, rl, x0, xt, r0, rt, t, "hybrid")
    assert abs(float(xh) - float(DT.loss(ac, z, x0, xt, t, "hybrid"))) < 1e-12                # same as the position module's hybrid
    vb_r = RT.losses(ac, z, rl, x0, xt, r0, rt, t, "vb")[1]
    assert abs(float(rh) - (RT.LAMBDA * plain(rl, r0) + float(vb_r))) < 1e-12


@pytest.mark.parametrize("K", RT.Q_KS)
@pytest.mark.parametrize("n", RT.Q_NS)
def test_noising_cases_are_clear_of_ties(K, n):
    x0, r0, t, u, ur = RT.q_sample_case(n, K, RT.Q_STEPS, RT.Q_SEEDS[(K, n)])
    assert set(t.tolist()) <= {0, 1, RT.Q_STEPS // 2, RT.Q_STEPS - 1} and (n < 4 or len(set(t.tolist())) == 4)
    _, gap_x, _, gap_rot = RT.q_sample2(DC.linear_alphas_cumprod(RT.Q_STEPS), x0, r0, t, u, ur, K)
    for what, gap in (("x", gap_x), ("rot", gap_rot)):
        assert float((gap < DC.GAP).double().mean()) <= DC.GAP_CAP, (what, K, n, int((gap < DC.GAP).sum()))


def _rot_backbone():
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete_ROT
    return Eff_GAT_Discrete_ROT(steps=20, input_channels=36, output_channels=36)


def test_param_order_of_the_rot_module():
    from diffassemble_amd.train import _param_order
    m = _rot_backbone()
    names, n_layers = _param_order(m)
    own = [k for k, _ in m.named_parameters() if not k.startswith("visual_backbone.")]
    assert n_layers == 4 and len(names) == len(set(names)) == 46 and sorted(names) == sorted(own)
    assert names[:2] == ["time_emb.weight", "pos_mlp.weight"]
    assert names[-8:] == ["final_mlp.0.weight", "final_mlp_rot.0.weight", "final_mlp.0.bias", "final_mlp_rot.0.bias",
                          "final_mlp.2.weight", "final_mlp.2.bias", "final_mlp_rot.2.weight", "final_mlp_rot.2.bias"]
    # the position model's layout is what it was
    from diffassemble_amd.model.backbones import Eff_GAT_Discrete
    nd, _ = _param_order(Eff_GAT_Discrete(steps=20, input_channels=36, output_channels=36))
    assert nd[-4:] == ["final_mlp.0.weight", "final_mlp.0.bias", "final_mlp.2.weight", "final_mlp.2.bias"] and len(nd) == 42


def test_new_prototypes_are_declared_and_the_abi_is_19():
    from diffassemble_amd import _lib
    from diffassemble_amd import train
    header = open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read()
    assert re.search(r"#define\s+DA_ABI_VERSION\s+19\b", header) and _lib.ABI_VERSION == 19
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _lib.PROTOTYPES, sym
        proto = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_lib.PROTOTYPES[sym][1]), sym
    assert re.search(r"DA_D3PM_DRAW_TRAINING_ROT = 3\b", header) and _lib.D3PM_DRAW_TRAINING_ROT == 3
    assert hasattr(train, "DenoiserTrainFn2")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(sym in integ for sym in NEW_SYMBOLS) and "DA_D3PM_DRAW_TRAINING_ROT" in integ


def test_training_refuses_cpu_tensors_with_the_documented_message(case):
    from diffassemble_amd.model import spatial_diffusion as SD
    from diffassemble_amd.model.spatial_diffusion_discrete_rot import GNN_Diffusion
    m = GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=20, sampling="DDPM", scheduler=SD.ModelScheduler.LINEAR, loss_type="hybrid")
    z = torch.zeros(72, dtype=torch.long)
    m.model.train()
    calls = (lambda: m.p_losses(z, z, z, loss_type="vb", edge_index=case["edge_index"], batch=case["batch"]),
             lambda: m.q_sample_rot(z, z),
             lambda: m.vb_terms_bpd(torch.zeros(72, 4), None, z, z, z, K=4),
             lambda: m.training_step(None, 0),
             lambda: m.model.forward_with_feats(z, z, z, None, case["edge_index"], case["feats4"][0], case["batch"]))
    for call in calls:
        with pytest.raises(NotImplementedError, match="^discrete-rotation training is not built yet off the device.*on ROCm tensors only"):
            call()
