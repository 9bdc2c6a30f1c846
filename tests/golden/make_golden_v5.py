"""Generate tests/golden/golden_v5.npz from the REFERENCE's own code: the GCN backbone (``architecture="gcn"``,
backbones/gcn.py:5-22, built by efficient_gat.py:65-70 / efficient_gat_3d.py:114-119) -- forwards with per-layer outputs
on every plan kind (complete graphs with and without self loops, Exphander graphs of even and odd degree, the dataset's
random-dropout edge list, a ragged Batch, the 3D variant), DDIM trajectories of the reference's p_sample_loop, and the
loss of p_losses with every live gradient (t and noise stored) for the training cases.

BUILD-CONTAINER ONLY (imports /root/reference/puzzle_diff/model/*.py under the stubs of ref_import.py, like
make_golden.py), with ``torch_geometric.nn.GCNConv`` bound to the restatement of gcn_cases.py.  Inputs and weights are
regenerated from seeds by gcn_cases.py; only outputs are stored.   Run:  python tests/golden/make_golden_v5.py
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gcn_cases as GC  # noqa: E402
import ref_import  # noqa: E402

torch.set_num_threads(8)
ref_import.install_stubs()
sys.modules["torch_geometric.nn"].GCNConv = GC.GCNConv          # PyG's GCNConv, restated (gcn_cases.py)
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sd2 = importlib.import_module("model.spatial_diffusion")
sd3 = importlib.import_module("model.spatial_diffusion_3d_test_double_diffusion")
OUT = {}


def put(case, field, t):
    OUT[f"{case}/{field}"] = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))


def stats(t):
    t = t.double()
    return torch.stack([t.sum(), t.abs().sum(), (t * t).sum()]).float()


def load_weights(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    dead = ("linear1.", "linear2.", "visual_backbone.", "pcd_backbone.", "mean", "std")
    bad = [k for k in missing if not k.startswith(dead)]
    assert not bad, bad


def model_2d(spec, ratio=1, mean="START_X", steps=None):
    m = sd2.GNN_Diffusion(steps=steps or spec["steps"], sampling="DDIM", inference_ratio=ratio, noise_weight=1.0,
                          rotation=(spec["c"] == 4), model_mean_type=getattr(sd2.ModelMeanType, mean), visual_pretrained=False,
                          architecture="gcn")
    m.eval()
    return m


def model_3d(spec, ratio=1, mean="START_X"):
    m = sd3.GNN_Diffusion(steps=spec["steps"], sampling="DDIM", inference_ratio=ratio, noise_weight=1.0,
                          model_mean_type=getattr(sd3.ModelMeanType, mean), backbone="vn_dgcnn", architecture="gcn")
    m.eval()
    return m


def hook_acts(model):
    acts = []
    hs = [model.mlp.register_forward_hook(lambda m, i, o: acts.append(o))]
    for conv in model.gnn_backbone.module_list:
        hs.append(conv.register_forward_hook(lambda m, i, o: acts.append(o)))
    return acts, hs


def put_acts(name, acts):
    for i, a in enumerate(acts):
        put(name, f"act{i}_stats", stats(a))
        put(name, f"act{i}_rows", a[:: max(1, a.shape[0] // 8), :64])


# the reference's state-dict layout with the GCN backbone (the CPU tests check the module's keys against it)
for variant, spec in (("2d", GC.GCN_FWD2D[0]), ("3d", GC.GCN_FWD3D[0])):
    m = model_2d(spec) if variant == "2d" else model_3d(spec)
    sdk = {k: v for k, v in m.model.state_dict().items() if not k.startswith(("visual_backbone.", "pcd_backbone."))}
    keys = sorted(sdk)
    put(f"statedict_gcn_{variant}", "keys", np.array(keys))
    put(f"statedict_gcn_{variant}", "shapes", np.array([str(tuple(sdk[k].shape)) for k in keys]))

for spec in GC.GCN_FWD2D:
    case = GC.build_case(spec)
    m = model_2d(spec)
    load_weights(m.model, case["sd"])
    acts, hs = hook_acts(m.model)
    with torch.no_grad():
        out, att = m.forward_with_feats(case["x"], case["t"], None, case["edge_index"], case["feats"], case["batch"],
                                        return_attentions=True)
    for h in hs:
        h.remove()
    assert att is None, "GCN.forward returns (x, None)"
    put(spec["name"], "out", out)
    put_acts(spec["name"], acts)
    print("fwd2d", spec["name"], tuple(out.shape), "E", case["edge_index"].shape[1], flush=True)

for lp in GC.GCN_LOOPS2D:
    spec = GC.by_name(lp["base"])
    case = GC.build_case(spec)
    m = model_2d(spec, ratio=lp["ratio"], mean=lp["mean"], steps=lp["T"])
    load_weights(m.model, case["sd"])
    m.visual_features = lambda cond, _f=case["feats"]: _f           # encoder bypassed
    torch.manual_seed(123)
    put(lp["name"], "x_init", torch.randn(case["x"].shape))
    torch.manual_seed(123)
    with torch.no_grad():
        imgs, _ = m.p_sample_loop(case["x"].shape, None, case["edge_index"], case["batch"])
    put(lp["name"], "imgs", torch.stack(imgs))
    print("loop2d", lp["name"], len(imgs), flush=True)

for spec in GC.GCN_FWD3D:
    case = GC.build_case(spec, "3d")
    m = model_3d(spec)
    load_weights(m.model, case["sd"])
    acts, hs = hook_acts(m.model)
    with torch.no_grad():
        out, att = m.forward_with_feats(case["x"], case["t"], case["edge_index"], case["feats"], case["batch"])
    for h in hs:
        h.remove()
    assert att is None
    put(spec["name"], "out", out)
    put_acts(spec["name"], acts)
    print("fwd3d", spec["name"], tuple(out.shape), flush=True)

for lp in GC.GCN_LOOPS3D:
    spec = GC.by_name(lp["base"])
    case = GC.build_case(spec, "3d")
    m = model_3d(spec, ratio=lp["ratio"], mean=lp["mean"])
    load_weights(m.model, case["sd"])
    b = case["x"].shape[0]
    torch.manual_seed(321)
    tr = torch.randn((b, 3))
    img = torch.cat([sd3.matrix_to_quaternion(torch.eye(3).repeat(b, 1, 1)), tr], 1)
    put(lp["name"], "x_init", img)
    imgs = []
    with torch.no_grad():
        for i in list(reversed(range(0, lp["T"], lp["ratio"])))[: lp["max_iters"]]:
            img, _ = m.p_sample(img, torch.full((b,), i, dtype=torch.long), i, edge_index=case["edge_index"],
                                pcd_feats=case["feats"], batch=case["batch"])
            imgs.append(img)
    put(lp["name"], "imgs", torch.stack(imgs))
    print("loop3d", lp["name"], len(imgs), flush=True)

for tr in GC.GCN_TRAIN2D:
    spec = GC.by_name(tr["base"])
    case = GC.build_case(spec)
    m = model_2d(spec, mean=tr["mean"])
    load_weights(m.model, case["sd"])
    m.train()
    m.visual_features = lambda cond, _f=case["feats"]: _f
    rng = np.random.default_rng(tr["seed"])
    noise = torch.from_numpy(rng.standard_normal(tuple(case["x"].shape)).astype(np.float32))
    loss = m.p_losses(case["x"], case["t"], noise=noise, loss_type="huber", cond=None, edge_index=case["edge_index"],
                      batch=case["batch"])
    loss.backward()
    put(tr["name"], "loss", loss)
    put(tr["name"], "t", case["t"])
    put(tr["name"], "noise", noise)
    n = 0
    for k, p in m.model.named_parameters():
        if p.grad is not None and k in case["sd"]:
            put(tr["name"], f"grad_stats/{k}", stats(p.grad))
            put(tr["name"], f"grad_head/{k}", p.grad.flatten()[:64])
            n += 1
    print("train", tr["name"], float(loss), n, "gradients", flush=True)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v5.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
