"""Generate tests/golden/golden_v8.npz from the REFERENCE's own code: the TRAINING step of the discrete position diffusion --
``GNN_Diffusion.p_losses`` of model/spatial_diffusion_discrete.py:229-273 (q_sample, the classifier-free mask, the denoiser,
cross entropy / vb_terms_bpd / their hybrid) + ``backward``.

BUILD-CONTAINER ONLY (imports the reference's model/*.py under the stubs of ref_import.py, like make_golden_v7.py).  Weights, graph
and piece features are v7's (``discrete_cases.v7_case``), x_start and t come from seeds (``discrete_train_cases.v8_inputs``); the
fixture holds arrays only.  Per case of ``discrete_train_cases.V8_CASES``:

* the [N, K] uniforms of q_sample and the [G] uniforms of the classifier-free mask (``torch.rand`` is patched for the duration so
  that the draws are recorded), the reference's x_noisy and its loss;
* for every live parameter the first 64 gradient entries and (sum, |g| sum, g^2 sum) -- golden_v6.npz's layout;
* the measured deviation of the fp64 closed form (discrete_train_cases.loss through discrete_cases.forward_with_feats, autograd)
  from the reference: the loss (relative, ``dev_loss``) and, per tensor in the order of ``param_names`` (``dev_grad``), the gradient's first 64 entries (max-abs over the tensor's largest
  entry, floored at 1e-4 x the largest gradient entry of the case).

The torch seed of every case is searched upwards until every node's top-2 gap of the perturbed q_sample logits is >= 1e-3 in fp64
(below that the argmax is decided by rounding) and, in the classifier-free case, exactly one of the two puzzles is masked.
Run:  python tests/golden/make_golden_v8.py
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402  (first: it puts the repository root on sys.path)
import discrete_cases as DC  # noqa: E402
import discrete_train_cases as DT  # noqa: E402

torch.set_num_threads(8)
ref_import.install_stubs()
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sdd = importlib.import_module("model.spatial_diffusion_discrete")
sd2 = importlib.import_module("model.spatial_diffusion")
OUT = {}
K, STEPS = DT.V8["K"], DT.V8["steps"]


def put(name, t):
    OUT[name] = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def stats(t):
    t = t.double()
    return torch.stack([t.sum(), t.abs().sum(), (t * t).sum()]).float()


case = DC.v7_case()
ei, batch, feats = case["edge_index"], case["batch"], case["feats"]
N = feats.shape[0]
orig_rand = torch.rand


def run_reference(spec, x_start, t, torch_seed):
    m = sdd.GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=STEPS, sampling="DDPM", scheduler=sd2.ModelScheduler.LINEAR,
                          loss_type=spec["kind"], lambda_loss=DT.V8["lambda_loss"], classifier_free_prob=spec["cfg_prob"])
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected and all(k in ("mean", "std") for k in missing), (missing, unexpected)
    m.train()
    m.visual_features = lambda cond, _f=feats: _f              # encoder bypassed: fixed seeded features
    seen, draws = {}, []
    inner = m.forward_with_feats

    def recording(x_noisy, *a, **k):
        seen["x_noisy"] = x_noisy.detach().clone()
        return inner(x_noisy, *a, **k)

    def rand(*a, **k):
        u = orig_rand(*a, **k)
        draws.append(u.clone())
        return u

    m.forward_with_feats = recording
    torch.manual_seed(torch_seed)
    torch.rand = rand
    try:
        loss = m.p_losses(x_start, t, loss_type=spec["kind"], cond=None, edge_index=ei, batch=batch)
    finally:
        torch.rand = orig_rand
    loss.backward()
    assert len(draws) == 2 and draws[0].shape == (N, K) and draws[1].shape == (len(DT.V8["sizes"]),), [d.shape for d in draws]
    return m, loss.detach(), seen["x_noisy"], draws[0], draws[1]


for spec in DT.V8_CASES:
    name = spec["name"]
    x_start, t = DT.v8_inputs(spec)
    for torch_seed in range(DT.V8["seed"], DT.V8["seed"] + 256):
        torch.manual_seed(torch_seed)
        u = orig_rand(size=(N, K))
        cfg = orig_rand(len(DT.V8["sizes"]))
        x_t64, gap = DT.q_sample(DC.linear_alphas_cumprod(STEPS), x_start, t, u, K)
        kept = cfg > spec["cfg_prob"]
        if float(gap.min()) >= DC.GAP and (spec["cfg_prob"] == 0.0 or int(kept.sum()) == 1):
            break
    else:
        raise SystemExit(f"{name}: no seed found")
    m, loss, x_noisy, u_rec, cfg_rec = run_reference(spec, x_start, t, torch_seed)
    assert torch.equal(u_rec, u) and torch.equal(cfg_rec, cfg)
    assert torch.equal(x_noisy, x_t64), (name, int((x_noisy != x_t64).sum()))
    put(f"{name}/torch_seed", torch_seed)
    put(f"{name}/x_start", x_start)
    put(f"{name}/t", t)
    put(f"{name}/uniforms", u_rec)
    put(f"{name}/cfg_rand", cfg_rec)
    put(f"{name}/x_noisy", x_noisy)
    put(f"{name}/min_gap", gap.min())
    put(f"{name}/loss", loss)
    # the fp64 closed form through the restated denoiser, autograd
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in case["sd"].items()}
    keep = (cfg_rec[batch] > spec["cfg_prob"]).double()
    logits = DC.forward_with_feats(sdg, x_noisy, t, ei, keep[:, None] * feats.double())
    loss64 = DT.loss(m.alphas_cumprod, logits, x_start, x_noisy, t, spec["kind"], DT.V8["lambda_loss"])
    loss64.backward()
    dev_loss = abs(float(loss64) - float(loss)) / abs(float(loss))
    put(f"{name}/dev_loss", np.float64(dev_loss))
    live = {k: p for k, p in m.model.named_parameters() if p.grad is not None and k in case["sd"]}
    assert len(live) == len(case["sd"]), (len(live), len(case["sd"]))
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in live.values())
    worst, devs = 0.0, []
    for k, p in live.items():
        put(f"{name}/grad_stats/{k}", stats(p.grad))
        put(f"{name}/grad_head/{k}", p.grad.flatten()[:64])
        dev = float((sdg[k].grad.flatten()[:64] - p.grad.flatten()[:64].double()).abs().max()) / max(float(p.grad.abs().max()), floor)
        devs.append(dev)
        worst = max(worst, dev)
    put(f"{name}/dev_grad", np.asarray(devs, dtype=np.float64))          # in the order of param_names
    put("param_names", np.array(list(live)))
    print(f"{name}: seed {torch_seed}  min gap {float(gap.min()):.3e}  loss {float(loss):.6f}  fp64 closed form: loss dev {dev_loss:.3e}, "
          f"worst gradient dev {worst:.3e}  cfg draw {cfg_rec.tolist()}", flush=True)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v8.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
