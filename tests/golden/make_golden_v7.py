"""Generate tests/golden/golden_v7.npz from the REFERENCE's own code: the discrete position diffusion --
``GNN_Diffusion`` of model/spatial_diffusion_discrete.py over ``Eff_GAT_Discrete`` (backbones/efficient_gat_discrete.py).

BUILD-CONTAINER ONLY (imports the reference's model/*.py under the stubs of ref_import.py, like make_golden_v6.py: timm is an
``Identity``, ``TransformerConv`` is the oracle's restatement).  Weights, graph and piece features are regenerated from seeds by
discrete_cases.py (``v7_case``); the fixture holds arrays only:

* ``forward_with_feats`` logits at t in {95, 50, 0} for recorded indices;
* ``q_posterior_logits`` (the reference's fp32 matrix formula) at t in {95, 50, 5} for recorded x_t and logits of scale 3;
* the reference's own 20-iteration ``p_sample_loop`` trajectory [20, 72] with its start indices and its uniforms [20, 72, 36]
  (``torch.rand`` / ``torch.randint`` are patched for the duration so that the draws are recorded);
* three ``p_sample_ddpm`` steps with classifier_free_prob > 0, w = 0.5;
* the state-dict keys and shapes of the module.

steps = 100 on purpose: at the driver's steps = 600 the reference's fp32 ``torch.linalg.inv(overline_Q[p])`` loses digits
(DESIGN.md 3l).  Run:  python tests/golden/make_golden_v7.py
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402  (first: it puts the repository root on sys.path)
import discrete_cases as DC  # noqa: E402

torch.set_num_threads(8)
ref_import.install_stubs()
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sdd = importlib.import_module("model.spatial_diffusion_discrete")
sd2 = importlib.import_module("model.spatial_diffusion")
OUT = {}
C = DC.V7
K, STEPS, RATIO = C["K"], C["steps"], C["ratio"]


def put(name, t):
    OUT[name] = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


case = DC.v7_case()
N = case["feats"].shape[0]
m = sdd.GNN_Diffusion(puzzle_sizes=[(6, 6)], steps=STEPS, inference_ratio=RATIO, sampling="DDPM",
                      scheduler=sd2.ModelScheduler.LINEAR)
missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
assert not unexpected and all(k in ("mean", "std") for k in missing), (missing, unexpected)
m.eval()
m.visual_features = lambda cond, _f=case["feats"]: _f              # encoder bypassed: fixed seeded features
keys = [k for k in m.state_dict() if not k.startswith("model.visual_backbone")]
put("statedict/keys", np.array(keys))
put("statedict/shapes", np.array([str(tuple(m.state_dict()[k].shape)) for k in keys]))
put("alphas_cumprod", m.alphas_cumprod)

g = torch.Generator().manual_seed(C["seed"])
ei, batch, feats = case["edge_index"], case["batch"], case["feats"]
with torch.no_grad():
    # forward
    for t in C["fwd_t"]:
        idx = torch.randint(0, K, (N,), generator=g)
        put(f"fwd/t{t}/idx", idx)
        put(f"fwd/t{t}/logits", m.forward_with_feats(idx, torch.full((N,), t, dtype=torch.long), None, ei, feats, batch))
    # posterior: the reference's matrix formula against recorded inputs
    worst = 0.0
    for t in C["post_t"]:
        x_t = torch.randint(0, K, (N,), generator=g)
        logits = 3.0 * torch.randn(N, K, generator=g)
        tt = torch.full((N,), t, dtype=torch.long)
        post = m.q_posterior_logits(x_t, logits, tt, tt - RATIO)
        put(f"post/t{t}/x_t", x_t)
        put(f"post/t{t}/logits", logits)
        put(f"post/t{t}/post", post)
        worst = max(worst, float((DC.posterior_logits(m.alphas_cumprod, x_t, logits, tt, tt - RATIO) - post.double()).abs().max()))
    print(f"closed form (fp64) vs the reference's fp32 matrix formula: max |diff| of the posterior logits = {worst:.3e}")
    put("post/closed_form_max_abs_diff", np.float64(worst))

    # the reference's own loop, draws recorded
    rec_rand, rec_randint = [], []
    orig_rand, orig_randint = torch.rand, torch.randint

    def rand(*a, **k):
        u = orig_rand(*a, **k)
        rec_rand.append(u.clone())
        return u

    def randint(*a, **k):
        v = orig_randint(*a, **k)
        rec_randint.append(v.clone())
        return v

    torch.manual_seed(C["seed"])
    torch.rand, torch.randint = rand, randint
    try:
        imgs = m.p_sample_loop((N,), None, ei, batch)
    finally:
        torch.rand, torch.randint = orig_rand, orig_randint
    assert len(imgs) == STEPS // RATIO == len(rec_rand) and len(rec_randint) == 1
    put("loop/x_init", rec_randint[0])
    put("loop/uniforms", torch.stack(rec_rand))
    put("loop/traj", torch.stack(imgs))

    # guided steps
    m.classifier_free_prob, m.classifier_free_w = 0.1, C["cfg_w"]
    for t in C["guided_t"]:
        x_t = torch.randint(0, K, (N,), generator=g)
        u = torch.rand(N, K, generator=g)
        torch.rand = lambda *a, _u=u, **k: _u.clone()
        try:
            nxt = m.p_sample_ddpm(x_t, torch.full((N,), t, dtype=torch.long), t, None, ei, feats, batch)
        finally:
            torch.rand = orig_rand
        put(f"guided/t{t}/x_t", x_t)
        put(f"guided/t{t}/uniforms", u)
        put(f"guided/t{t}/x_prev", nxt)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v7.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
