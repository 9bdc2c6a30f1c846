"""Generate tests/golden/pcd_train_v1.npz from the REFERENCE's own 3D piece encoder in train() mode.

BUILD-CONTAINER ONLY (imports /root/reference/puzzle_diff/model/backbones/vnn/vn_dgcnn.py from where it lies, under the
stubs of ref_import.py, with the ``torch.device('cuda')`` of get_graph_feature answered by "cpu" as in make_golden_v3.py).
Per case of PCD_TRAIN the reference module runs train() forward + backward of  sum(out * G)  (G a seeded cotangent) twice:
in fp64 (``net.double()``, the stored values) and in fp32 (only its disagreement with fp64 is stored, per tensor, as
``err32/<name>`` = max-abs difference / max-abs of the fp64 value).  Stored (fp32):

* ``out``                         the (last) forward's output
* ``grad/<param>``                every parameter gradient that is not None, ``grad/points``
* ``none/<param>``                the names of the parameters whose gradient is None (one string array)
* ``bn/<layer>/{running_mean,running_var,num_batches_tracked}``   all eight BatchNorms after the case's forwards

A case passes only if the fp32 and fp64 neighbour lists agree at all three stages and every list is separated from the
next candidate by a margin (``MARGIN`` of the cloud's squared radius; the 2000 lists of p2_n1000 only need to agree);
otherwise the next seed is tried.  Inputs come from
oracle.weights seeds: ``make_vn_dgcnn_state(feat, wseed)``, ``make_point_clouds(P, N, seed)``, G from ``gseed``.
Run:  python tests/golden/make_pcd_train_golden.py
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cases as C  # noqa: E402,F401  (puts the repository on sys.path)
from ref_import import REF, install_stubs  # noqa: E402
from oracle import weights as W  # noqa: E402

install_stubs()
sys.path.insert(0, REF)
vn = importlib.import_module("model.backbones.vnn.vn_dgcnn")


class _TorchOnCPU:
    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def device(*a, **k):
        return torch.device("cpu")


vn.torch = _TorchOnCPU()
MARGIN = 1e-7
BN_NAMES = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "VnInv.vn1", "VnInv.vn2")
# name, fragments, points, feat_dim, inv, forwards (the last one is differentiated)
PCD_TRAIN = [
    dict(name="p3_n64", P=3, N=64, feat=64, inv=False, fwd=1),
    dict(name="p4_n128_inv", P=4, N=128, feat=32, inv=True, fwd=1),
    dict(name="p2_n1000", P=2, N=1000, feat=32, inv=False, fwd=1, margin=0.0),
    dict(name="p5_n37", P=5, N=37, feat=32, inv=False, fwd=1),
    dict(name="p3_n48_two_forwards", P=3, N=48, feat=32, inv=False, fwd=2),
]


def run(spec, sd, clouds, G, dtype):
    net = vn.VN_DGCNN(spec["feat"], inv=spec["inv"])
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).train()
    lists, real = [], vn.knn

    def spy(x, k):
        idx = real(x, k)
        lists.append((x.detach().clone(), idx))
        return idx

    vn.knn = spy
    try:
        for pts in clouds:
            lists.clear()
            pts = pts.to(dtype).clone().requires_grad_(True)
            out = net(pts)
        (out * G.to(dtype)).sum().backward()
    finally:
        vn.knn = real
    return net, out.detach(), pts.grad, [(x, i.clone()) for x, i in lists]


def margin_ok(lists64, margin):
    for x, _ in lists64:                                        # x [B, F, N]
        xt = x.transpose(2, 1)
        inner = -2 * xt @ x
        xx = (x * x).sum(1, keepdim=True)
        pd = -xx - inner - xx.transpose(2, 1)
        top = pd.topk(21, dim=-1)[0]
        gap = (top[..., 19] - top[..., 20]) / xx.amax(-1, keepdim=True).clamp_min(1e-12)
        if float(gap.min()) < margin:
            return False
    return True


def one_case(spec):
    for attempt in range(64):
        wseed, seed, gseed = 100 + attempt, 200 + attempt, 300 + attempt
        sd = W.make_vn_dgcnn_state(spec["feat"], wseed)
        clouds = [W.make_point_clouds(spec["P"], spec["N"], seed + 17 * f) for f in range(spec["fwd"])]
        odim = 2 * spec["feat"] if spec["inv"] else 6 * spec["feat"]
        G = torch.from_numpy(np.random.default_rng(gseed).standard_normal((spec["P"], odim)).astype(np.float32))
        n64, o64, g64, l64 = run(spec, sd, clouds, G, torch.float64)
        n32, o32, g32, l32 = run(spec, sd, clouds, G, torch.float32)
        same = all(torch.equal(a[1].sort(-1)[0], b[1].sort(-1)[0]) for a, b in zip(l64, l32))
        if same and margin_ok(l64, spec.get("margin", MARGIN)):
            return dict(wseed=wseed, seed=seed, gseed=gseed), (n64, o64, g64), (n32, o32, g32)
        print(spec["name"], "seed offset", attempt, "rejected (neighbour lists not separated)")
    raise RuntimeError(f"{spec['name']}: no seed with separated neighbour lists")


def err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


OUT = {}
for spec in PCD_TRAIN:
    seeds, (n64, o64, g64), (n32, o32, g32) = one_case(spec)
    k = f"pcd_train/{spec['name']}"
    OUT[f"{k}/seeds"] = np.array([seeds["wseed"], seeds["seed"], seeds["gseed"]], dtype=np.int64)
    OUT[f"{k}/out"] = o64.float().numpy()
    OUT[f"{k}/err32/out"] = np.float64(err(o32, o64))
    OUT[f"{k}/grad/points"] = g64.float().numpy()
    OUT[f"{k}/err32/grad/points"] = np.float64(err(g32, g64))
    p32 = dict(n32.named_parameters())
    none = []
    for name, p in n64.named_parameters():
        if p.grad is None:
            none.append(name)
            continue
        OUT[f"{k}/grad/{name}"] = p.grad.float().numpy()
        OUT[f"{k}/err32/grad/{name}"] = np.float64(err(p32[name].grad, p.grad))
    OUT[f"{k}/none"] = np.array(none)
    b32 = dict(n32.named_buffers())
    for name, b in n64.named_buffers():
        OUT[f"{k}/bn/{name}"] = b.numpy() if b.dtype == torch.int64 else b.float().numpy()
        if b.is_floating_point():
            OUT[f"{k}/err32/bn/{name}"] = np.float64(err(b32[name], b))
    print(spec["name"], seeds, "out", tuple(o64.shape), "worst fp32 gradient error",
          max(float(v) for kk, v in OUT.items() if kk.startswith(f"{k}/err32/grad")))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pcd_train_v1.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, len(OUT), "arrays,", os.path.getsize(path), "bytes")
