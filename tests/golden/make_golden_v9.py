"""Generate tests/golden/golden_v9.npz from the REFERENCE's own code: the discrete position + rotation diffusion --
``GNN_Diffusion`` of model/spatial_diffusion_discrete_rot.py over ``Eff_GAT_Discrete_ROT``
(backbones/efficient_gat_discrete_rotation.py).

BUILD-CONTAINER ONLY (imports the reference's model/*.py under the stubs of ref_import.py, like make_golden_v7.py).  Weights, graph
and the four feature images are regenerated from seeds by discrete_rot_cases.py (``v9_case``); the fixture holds arrays only.

Three stand-ins, all recorded in DESIGN.md 1 / 3m:
* the reference backbone raises as shipped (efficient_gat_discrete_rotation.py:106-110 adds the ``(x, attentions)`` pair that
  ``Transformer_GNN.forward`` returns to a tensor): ``gnn_backbone.forward`` is wrapped to return its first value;
* ``rotate_images(cond_start, -rot_acc)`` is replaced by ``(-rot_index) % 4``: the "crops" travel as their rotation index ...
* ... and ``visual_features(cond)`` by the lookup of that index in the four feature images.

Recorded: the two-headed forward at t in {95, 50, 0} with mixed feature images; the reference's own 20-iteration ``p_sample_loop``
for (cold_diffusion, only_rotation) in {(F, F), (T, F), (T, T)} with every draw, each step's input state (index, rot, rot_acc) and
each step's output triple; the state-dict keys and shapes; the closed-form-vs-reference difference of the rotation posterior.
The script ASSERTS that the fp64 restatement reproduces the reference's trajectories outside near ties and that near ties stay
within GAP_CAP per quantity.  Run:  python tests/golden/make_golden_v9.py
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

torch.set_num_threads(8)
ref_import.install_stubs()
if ref_import.REF not in sys.path:
    sys.path.insert(0, ref_import.REF)
sddr = importlib.import_module("model.spatial_diffusion_discrete_rot")
sd2 = importlib.import_module("model.spatial_diffusion")
OUT = {}
C = RC.V9
K, STEPS, RATIO = C["K"], C["steps"], C["ratio"]


def put(name, t):
    OUT[name] = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


case = RC.v9_case()
feats4 = case["feats4"]
N = feats4.shape[1]
ei, batch = case["edge_index"], case["batch"]
sddr.rotate_images = lambda patches, rot_index: (-rot_index) % 4


def module(cold, only_rot):
    m = sddr.GNN_Diffusion(only_rotation=only_rot, cold_diffusion=cold, puzzle_sizes=[(6, 6)], steps=STEPS, inference_ratio=RATIO,
                           sampling="DDPM", scheduler=sd2.ModelScheduler.LINEAR)
    missing, unexpected = m.model.load_state_dict(case["sd"], strict=False)
    assert not unexpected and all(k in ("mean", "std") for k in missing), (missing, unexpected)
    m.eval()
    gb, fwd = m.model.gnn_backbone, m.model.gnn_backbone.forward
    gb.forward = lambda *a, **k: fwd(*a, **k)[0]                        # the one deviation: unpack (x, attentions)
    m.visual_features = lambda cond: RC.select_feats(feats4, cond)     # cond IS the rotation index (see rotate_images above)
    return m


m = module(False, False)
keys = [k for k in m.state_dict() if not k.startswith("model.visual_backbone")]
put("statedict/keys", np.array(keys))
put("statedict/shapes", np.array([str(tuple(m.state_dict()[k].shape)) for k in keys]))
put("alphas_cumprod", m.alphas_cumprod)
ac = m.alphas_cumprod

g = torch.Generator().manual_seed(C["seed"])
with torch.no_grad():
    for t in C["fwd_t"]:
        idx = torch.randint(0, K, (N,), generator=g)
        acc = torch.randint(0, 4, (N,), generator=g)
        tt = torch.full((N,), t, dtype=torch.long)
        lo, rl = m.forward_with_feats(idx, tt, None, ei, RC.select_feats(feats4, acc), torch.zeros(N, dtype=torch.long), batch)
        put(f"fwd/t{t}/idx", idx)
        put(f"fwd/t{t}/rot_acc", acc)
        put(f"fwd/t{t}/logits", lo)
        put(f"fwd/t{t}/rot_logits", rl)
    # rotation posterior: the reference's matrix formula (K = 4, overline_Q_rot) against the closed form
    worst = 0.0
    for t in C["post_t"]:
        r_t = torch.randint(0, 4, (N,), generator=g)
        rl = 3.0 * torch.randn(N, 4, generator=g)
        tt = torch.full((N,), t, dtype=torch.long)
        post = m.q_posterior_logits(r_t, rl, tt, tt - RATIO, K=4, overline_Q=m.overline_Q_rot)
        put(f"post/t{t}/rot_t", r_t)
        put(f"post/t{t}/rot_logits", rl)
        put(f"post/t{t}/post", post)
        worst = max(worst, float((DC.posterior_logits(ac, r_t, rl, tt, tt - RATIO) - post.double()).abs().max()))
    print(f"rotation posterior, closed form (fp64) vs the reference's fp32 matrix formula: max |diff| = {worst:.3e}")
    put("post/closed_form_max_abs_diff", np.float64(worst))

    orig_rand, orig_randint = torch.rand, torch.randint
    x_start = torch.randint(0, K, (N,), generator=g)
    put("loop/x_start", x_start)
    for cold, only_rot in C["modes"]:
        name = RC.MODE_NAME[(cold, only_rot)]
        m = module(cold, only_rot)
        rec_rand, rec_randint, rec_in, rec_out = [], [], [], []

        def rand(*a, **k):
            u = orig_rand(*a, **k)
            rec_rand.append(u.clone())
            return u

        def randint(*a, **k):
            v = orig_randint(*a, **k)
            rec_randint.append(v.clone())
            return v

        inner = m.p_sample

        def p_sample(index, rot, t, i, **kw):
            rec_in.append((index.clone(), rot.clone(), kw["cond"].clone()))
            out = inner(index, rot, t, i, **kw)
            rec_out.append(tuple(o.clone() for o in out))
            return out

        m.p_sample = p_sample
        torch.manual_seed(C["seed"] + 1)
        torch.rand, torch.randint = rand, randint
        try:
            imgs = m.p_sample_loop((N,), torch.zeros(N, dtype=torch.long), ei, batch, x_start=x_start)
        finally:
            torch.rand, torch.randint = orig_rand, orig_randint
        n_it = STEPS // RATIO
        assert len(imgs) == n_it and len(rec_rand) == 2 * n_it and len(rec_randint) == 2
        u_x, u_rot = torch.stack(rec_rand[0::2]), torch.stack(rec_rand[1::2])
        assert u_x.shape == (n_it, N, K) and u_rot.shape == (n_it, N, 4)
        put(f"loop/{name}/x_init", rec_randint[0])
        put(f"loop/{name}/rot_init", rec_randint[1])
        put(f"loop/{name}/u_x", u_x)
        put(f"loop/{name}/u_rot", u_rot)
        for j, what in enumerate(("index", "rot", "rot_acc")):
            put(f"loop/{name}/in_{what}", torch.stack([r[j] for r in rec_in]))
        for j, what in enumerate(("x_prev", "rot_0", "rot_prev")):
            put(f"loop/{name}/{what}", torch.stack([r[j] for r in rec_out]))
        put(f"loop/{name}/traj_index", torch.stack([im[0] for im in imgs]))
        # the loop's own bookkeeping.  The rot_acc tensors the reference RETURNS are aliased: `rot_acc += rot` (:370) updates in place
        # the tensor appended to `imgs` one step earlier, so every returned entry but the last already carries the next step's
        # rotation, not reduced mod 4.  The trajectory recorded here is each step's own rot_acc, i.e. the state the next step reads
        # (its `cond`); the last returned entry is not aliased and must equal it.
        accs = []
        for it in range(n_it):
            nxt_rot = rec_out[it][2] if cold else rec_out[it][1]
            accs.append((rec_in[it][2] + nxt_rot) % 4)
            assert torch.equal(imgs[it][0], rec_out[it][0])
            if it + 1 < n_it:
                assert torch.equal(rec_in[it + 1][2], accs[it]) and torch.equal(rec_in[it + 1][1], nxt_rot)
                assert torch.equal(imgs[it][1], accs[it] + (rec_out[it + 1][2] if cold else rec_out[it + 1][1]))      # the alias
            if only_rot:
                assert torch.equal(rec_in[it][0], x_start)
        assert torch.equal(imgs[-1][1], accs[-1])
        put(f"loop/{name}/traj_rot_acc", torch.stack(accs))
        # the fp64 restatement, teacher-forced on the recorded inputs, against the reference's own outputs
        near = dict(x=0, rot0=0, rot=0)
        for it, i in enumerate(reversed(range(0, STEPS, RATIO))):
            idx, rot, acc = rec_in[it]
            tt = torch.full((N,), i, dtype=torch.long)
            lo, rl = RC.forward_with_feats(case["sd"], idx, tt, ei, RC.select_feats(feats4, acc))
            s = RC.rot_step(ac, idx, rot, lo, rl, tt, RATIO, u_x[it], u_rot[it])
            for q, gap, ref in (("x", "gap_x", rec_out[it][0]), ("rot0", "gap_rot0", rec_out[it][1]), ("rot", "gap_rot", rec_out[it][2])):
                clear = s[gap] >= RC.GAP
                near[q] += int((~clear).sum())
                got = s[{"x": "x_prev", "rot0": "rot_0", "rot": "rot_prev"}[q]]
                assert torch.equal(got[clear], ref[clear]), (name, it, q)
        print(f"{name}: restatement == reference outside near ties; near ties of {n_it * N}: {near}")
        assert all(v <= RC.GAP_CAP * n_it * N for v in near.values()), near
        put(f"loop/{name}/near_ties", np.array([near["x"], near["rot0"], near["rot"]]))

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_v9.npz")
np.savez_compressed(path, **OUT)
print("wrote", path, os.path.getsize(path), "bytes,", len(OUT), "arrays")
