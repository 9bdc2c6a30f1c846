"""Generate tests/golden/golden_v6.npz from the REFERENCE's own code: the 3D training step -- ``GNN_Diffusion.p_losses`` of
spatial_diffusion_3d_test_double_diffusion.py:410-572 (SE(3) noising with IsotropicGaussianSO3, the denoiser, the assembly
losses of utils_3d.py) + ``backward`` -- at train_3d.py's configuration with the transformer, exophormer and gcn backbones,
and the IGSO(3) CDF columns of distributions.py:488-505 for ten timesteps.

BUILD-CONTAINER ONLY (imports the reference's model/*.py under the stubs of ref_import.py, like make_golden_v5.py), with
``torch_geometric.nn.GCNConv`` bound to the restatement of gcn_cases.py.  ``pcd_features`` is replaced by fixed seeded
features.  Inputs and weights are regenerated from seeds by train3d_cases.py; only results are stored: t, the three random
draws of the noising (replayed after re-seeding), x_noisy and the prediction (recorded at forward_with_feats), the five
entries of the loss dictionary and, per gradient, the first 64 entries and (sum, |.| sum, square sum).

The torch seed of every case is searched upwards from the case's seed until (a) every x_noisy and predicted quaternion has
|w| >= 1e-3 (below that the w >= 0 standardisation of matrix_to_quaternion is decided by rounding) and (b) no ground-truth
rotation lies within 1e-3 of pi; the tests assert both on the stored data.   Run:  python tests/golden/make_golden_v6.py
"""
import importlib
import math
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gcn_cases as GC  # noqa: E402
import ref_import  # noqa: E402
import train3d_cases as T3  # noqa: E402

torch.set_num_threads(8)
ref_import.install_stubs()
sys.modules["torch_geometric.nn"].GCNConv = GC.GCNConv          # PyG's GCNConv, restated (gcn_cases.py)
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sd3 = importlib.import_module("model.spatial_diffusion_3d_test_double_diffusion")
dist = importlib.import_module("model.distributions")
OUT = {}


def put(case, field, t):
    OUT[f"{case}/{field}"] = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def stats(t):
    t = t.double()
    return torch.stack([t.sum(), t.abs().sum(), (t * t).sum()]).float()


def load_weights(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    bad = [k for k in missing if not k.startswith(("pcd_backbone.",))]
    assert not bad, bad


def run_case(spec, case, torch_seed):
    m = sd3.GNN_Diffusion(steps=T3.STEPS, sampling="DDIM", inference_ratio=1, noise_weight=1.0,
                          model_mean_type=sd3.ModelMeanType.START_X, backbone="vn_dgcnn", architecture=spec["arch"],
                          max_num_part=T3.MAX_PARTS, loss_type="all")
    load_weights(m.model, case["sd"])
    m.train()
    m.pcd_features = lambda cond, _f=case["feats"]: _f              # encoder bypassed: fixed seeded features
    seen = {}
    inner = m.forward_with_feats

    def recording(x_noisy, *a, **k):
        seen["x_noisy"] = x_noisy.detach().clone()
        out = inner(x_noisy, *a, **k)
        seen["prediction"] = out[0].detach().clone()
        return out

    m.forward_with_feats = recording
    torch.manual_seed(torch_seed)
    loss_dict = m.p_losses(case["x_start"], case["t"], loss_type="all", cond=case["pts"], edge_index=case["edge_index"],
                           batch=case["batch"], n_batch=len(T3.SIZES), valids=case["valids"])
    sum(loss_dict.values()).backward()
    return m, loss_dict, seen


for spec in T3.TRAIN3D:
    case = T3.build_case(spec)
    P = case["x_start"].shape[0]
    gt_angle = 2 * torch.acos(case["x_start"][:, 0].double().clamp(-1, 1))
    assert float((gt_angle - math.pi).abs().min()) > 1e-3, "a ground-truth rotation within 1e-3 of pi"
    for torch_seed in range(spec["seed"], spec["seed"] + 64):
        m, loss_dict, seen = run_case(spec, case, torch_seed)
        if float(seen["x_noisy"][:, 0].abs().min()) >= T3.W_MIN and float(seen["prediction"][:, 0].abs().min()) >= T3.W_MIN:
            break
    else:
        raise SystemExit(f"{spec['name']}: no seed with |w| >= {T3.W_MIN}")
    torch.manual_seed(torch_seed)                                  # replay the reference's stream: randn_like(x_start_tr), then
    noise_tr = torch.randn(P, 3)                                   # IsotropicGaussianSO3.sample: randn(P, 3), rand(P)
    axes = torch.randn(P, 3)
    unif = torch.rand(P)
    name = spec["name"]
    put(name, "torch_seed", torch_seed)
    put(name, "t", case["t"])
    put(name, "noise_tr", noise_tr)
    put(name, "axes", axes)
    put(name, "unif", unif)
    put(name, "x_noisy", seen["x_noisy"])
    put(name, "prediction", seen["prediction"])
    assert list(loss_dict) == ["trans_loss", "rot_pt_cd_loss", "transform_pt_cd_loss", "rot_loss", "rot_pt_l2_loss"], list(loss_dict)
    for k, v in loss_dict.items():
        put(name, f"loss/{k}", v)
    n = 0
    for k, p in m.model.named_parameters():
        if p.grad is not None and k in case["sd"]:
            put(name, f"grad_stats/{k}", stats(p.grad))
            put(name, f"grad_head/{k}", p.grad.flatten()[:64])
            n += 1
    assert n == len(case["sd"]), (n, len(case["sd"]))
    print(name, "seed", torch_seed, {k: float(v) for k, v in loss_dict.items()}, n, "gradients", flush=True)

# the IGSO(3) CDF columns the reference builds for pieces at the timesteps TRAP_T (one column per piece, distributions.py:488-505)
m = sd3.GNN_Diffusion(steps=T3.STEPS, sampling="DDIM", model_mean_type=sd3.ModelMeanType.START_X, backbone="vn_dgcnn",
                      max_num_part=T3.MAX_PARTS)
eps = m.sqrt_one_minus_alphas_cumprod[torch.tensor(T3.TRAP_T)]
put("igso3", "t", np.asarray(T3.TRAP_T))
put("igso3", "trap", dist.IsotropicGaussianSO3(eps).trap.t().contiguous())
put("igso3", "sqrt_one_minus_alphas_cumprod", m.sqrt_one_minus_alphas_cumprod)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v6.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
