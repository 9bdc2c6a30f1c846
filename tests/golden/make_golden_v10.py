"""Generate tests/golden/golden_v10.npz from the REFERENCE's own code: the TRAINING step of the discrete position + rotation
diffusion -- ``GNN_Diffusion.p_losses`` of model/spatial_diffusion_discrete_rot.py:161-279 (the two q_sample calls, the
classifier-free mask, the two-headed denoiser, cross entropy / vb_terms_bpd / their hybrid per head) + ``backward`` of the SUM of
the returned losses.

BUILD-CONTAINER ONLY (imports the reference's model/*.py under the stubs of ref_import.py, like make_golden_v8.py).  Weights and
graph are v9's (``discrete_rot_cases.v9_case``), the features its image 0; x_start, rot_start and t come from seeds
(``discrete_rot_train_cases.v10_inputs``); the fixture holds arrays only.  The one stand-in is make_golden_v9.py's: the reference
backbone raises as shipped, so ``gnn_backbone.forward`` is wrapped to return its first value.  Per case of
``discrete_rot_train_cases.V10_CASES``:

* the three recorded draws, in the reference's order: [N, K] (position noising), [N, 4] (rotation noising), [G] (classifier-free
  mask) -- ``torch.rand`` is patched for the duration;
* the reference's x_noisy (what the network is fed: x_start under only_rotation), rot_noisy, x_loss, rot_loss (x_loss absent under
  only_rotation);
* for every live parameter the first 64 gradient entries and (sum, |g| sum, g^2 sum) -- golden_v8.npz's layout -- under
  ``{name}/param_names`` (under only_rotation the four final_mlp.* tensors get no gradient and are not listed);
* the measured deviation of the fp64 closed form (discrete_rot_train_cases.losses through discrete_rot_cases.forward_with_feats,
  autograd) from the reference: per loss (relative, ``dev_x_loss`` / ``dev_rot_loss``) and per tensor (``dev_grad``, the first 64
  entries, max-abs over the tensor's largest entry, floored at 1e-4 x the largest gradient entry of the case).

The torch seed of every case is searched upwards until every piece's top-2 gap of BOTH noisings is >= discrete_cases.GAP in fp64
and, in the classifier-free case, exactly one of the two puzzles is masked.  Run:  python tests/golden/make_golden_v10.py
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402  (first: it puts the repository root on sys.path)
import discrete_cases as DC  # noqa: E402
import discrete_rot_cases as RC  # noqa: E402
import discrete_rot_train_cases as RT  # noqa: E402

torch.set_num_threads(8)
ref_import.install_stubs()
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sddr = importlib.import_module("model.spatial_diffusion_discrete_rot")
sd2 = importlib.import_module("model.spatial_diffusion")
OUT = {}
K, STEPS = RT.V10["K"], RT.V10["steps"]


def put(name, t):
    OUT[name] = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def stats(t):
    t = t.double()
    return torch.stack([t.sum(), t.abs().sum(), (t * t).sum()]).float()


case = RC.v9_case()
ei, batch, feats = case["edge_index"], case["batch"], case["feats4"][0]
N, G = feats.shape[0], len(RT.V10["sizes"])
orig_rand = torch.rand


def run_reference(spec, x_start, rot_start, t, torch_seed):
    m = sddr.GNN_Diffusion(only_rotation=spec["only_rot"], cold_diffusion=False, puzzle_sizes=[(6, 6)], steps=STEPS, sampling="DDPM",
                           scheduler=sd2.ModelScheduler.LINEAR, loss_type=spec["kind"], lambda_loss=RT.V10["lambda_loss"],
                           classifier_free_prob=spec["cfg_prob"])
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected and all(k in ("mean", "std") for k in missing), (missing, unexpected)
    m.train()
    gb, fwd = m.model.gnn_backbone, m.model.gnn_backbone.forward
    gb.forward = lambda *a, **k: fwd(*a, **k)[0]                # the one stand-in: unpack (x, attentions)
    m.visual_features = lambda cond, _f=feats: _f              # encoder bypassed: fixed seeded features
    seen, draws = {}, []
    inner = m.forward_with_feats

    def recording(x_noisy, *a, **k):
        seen["x_noisy"] = x_noisy.detach().clone()
        seen["rot_noisy"] = k["rot"].detach().clone()
        return inner(x_noisy, *a, **k)

    def rand(*a, **k):
        u = orig_rand(*a, **k)
        draws.append(u.clone())
        return u

    m.forward_with_feats = recording
    torch.manual_seed(torch_seed)
    torch.rand = rand
    try:
        losses = m.p_losses(x_start, t, rot_start, loss_type=spec["kind"], cond=None, edge_index=ei, batch=batch)
    finally:
        torch.rand = orig_rand
    assert sorted(losses) == (["rot_loss"] if spec["only_rot"] else ["rot_loss", "x_loss"]), sorted(losses)
    sum(losses.values()).backward()
    assert [tuple(d.shape) for d in draws] == [(N, K), (N, 4), (G,)], [d.shape for d in draws]
    return m, {k: v.detach() for k, v in losses.items()}, seen, draws


for spec in RT.V10_CASES:
    name = spec["name"]
    x_start, rot_start, t = RT.v10_inputs(spec)
    ac = DC.linear_alphas_cumprod(STEPS)
    for torch_seed in range(RT.V10["seed"], RT.V10["seed"] + 256):
        torch.manual_seed(torch_seed)
        u_x = orig_rand(size=(N, K))
        u_rot = orig_rand(size=(N, 4))
        cfg = orig_rand(G)
        x_t64, gap_x, rot_t64, gap_rot = RT.q_sample2(ac, x_start, rot_start, t, u_x, u_rot, K)
        kept = cfg > spec["cfg_prob"]
        if min(float(gap_x.min()), float(gap_rot.min())) >= DC.GAP and (spec["cfg_prob"] == 0.0 or int(kept.sum()) == 1):
            break
    else:
        raise SystemExit(f"{name}: no seed found")
    m, ref, seen, draws = run_reference(spec, x_start, rot_start, t, torch_seed)
    assert torch.equal(draws[0], u_x) and torch.equal(draws[1], u_rot) and torch.equal(draws[2], cfg)
    x_fed = x_start if spec["only_rot"] else x_t64                 # (under only_rotation the position draw is made and dropped)
    assert torch.equal(seen["x_noisy"], x_fed), (name, int((seen["x_noisy"] != x_fed).sum()))
    assert torch.equal(seen["rot_noisy"], rot_t64), (name, int((seen["rot_noisy"] != rot_t64).sum()))
    assert torch.equal(m.alphas_cumprod, ac)
    put(f"{name}/torch_seed", torch_seed)
    put(f"{name}/x_start", x_start)
    put(f"{name}/rot_start", rot_start)
    put(f"{name}/t", t)
    put(f"{name}/uniforms_x", draws[0])
    put(f"{name}/uniforms_rot", draws[1])
    put(f"{name}/cfg_rand", draws[2])
    put(f"{name}/x_noisy", seen["x_noisy"])
    put(f"{name}/rot_noisy", seen["rot_noisy"])
    put(f"{name}/min_gap", np.float64(min(float(gap_x.min()), float(gap_rot.min()))))
    for k, v in ref.items():
        put(f"{name}/{k}", v)
    # the fp64 closed form through the restated denoiser, autograd of the sum of the returned losses
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in case["sd"].items()}
    keep = (draws[2][batch] > spec["cfg_prob"]).double()
    logits, rot_logits = RC.forward_with_feats(sdg, x_fed, t, ei, keep[:, None] * feats.double())
    x64, r64 = RT.losses(ac, None if spec["only_rot"] else logits, rot_logits, x_start, x_fed, rot_start, rot_t64, t, spec["kind"],
                         RT.V10["lambda_loss"])
    (r64 if x64 is None else x64 + r64).backward()
    devs = {}
    for k, v64 in (("x_loss", x64), ("rot_loss", r64)):
        if v64 is not None:
            devs[k] = abs(float(v64.detach()) - float(ref[k])) / abs(float(ref[k]))
            put(f"{name}/dev_{k}", np.float64(devs[k]))
    live = {k: p for k, p in m.model.named_parameters() if p.grad is not None and k in case["sd"]}
    dead = sorted(set(case["sd"]) - set(live))
    assert dead == (sorted(k for k in case["sd"] if k.startswith("final_mlp.")) if spec["only_rot"] else []), dead
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in live.values())
    worst, dg = 0.0, []
    for k, p in live.items():
        put(f"{name}/grad_stats/{k}", stats(p.grad))
        put(f"{name}/grad_head/{k}", p.grad.flatten()[:64])
        dev = float((sdg[k].grad.flatten()[:64] - p.grad.flatten()[:64].double()).abs().max()) / max(float(p.grad.abs().max()), floor)
        dg.append(dev)
        worst = max(worst, dev)
    put(f"{name}/dev_grad", np.asarray(dg, dtype=np.float64))          # in the order of {name}/param_names
    put(f"{name}/param_names", np.array(list(live)))
    print(f"{name}: seed {torch_seed}  min gap {float(OUT[name + '/min_gap']):.3e}  losses { {k: round(float(v), 6) for k, v in ref.items()} }  "
          f"fp64 closed form: loss devs { {k: f'{v:.2e}' for k, v in devs.items()} }, worst gradient dev {worst:.3e}  "
          f"{len(live)} live tensors  cfg draw {draws[2].tolist()}", flush=True)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v10.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
