"""Which kernels ONE forward of the denoiser launches, per route of its dispatch (csrc/da_forward.hip: forward_impl), pinned as literal
per-class launch counts of `da_profile_enable` / `profile_read()`.

The parity suites compare results; a layer that quietly fell through to a slower but correct route (the edge list instead of the
matrix-core attention, three tail kernels instead of one, a projection kernel in front of an attention kernel that could have projected
itself) passes all of them.  Here every route is selected at the smallest shape that selects it, and the number of launches per
profile class must equal `EXPECTED`.

`EXPECTED` was recorded from the library of commit 0bef16d (the parent of the commit that split forward_impl into stages), in the same
GPU visit as this test's first run, by running `run_route` over `ROUTES` against that library; it is a statement about that commit's
dispatch, not about the code under test.  Profiling keeps the exophormer's virtual rows off the side stream, so the fork of Batches of
8 192 pieces and more is left to the parity suites (test_gpu_benched_mode.py, test_gpu_scripted.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def state(kind):
    """Seeded weights, one set per model kind (shared by the routes over it)."""
    import discrete_cases as DC
    import discrete_rot_cases as DR
    import gcn_cases as GC
    if kind == "tr":
        return W.make_denoiser_state(100, 4, 4, seed=81, qk_gain=2.0)
    if kind == "exo":
        return W.make_denoiser_state(300, 4, 4, arch="exophormer", virt_nodes=8, seed=82, qk_gain=3.0)
    if kind == "3d":
        return W.make_denoiser_state(300, 7, None, D=832, hidden=256, variant="3d", seed=83, qk_gain=2.0)
    if kind == "gcn":
        return GC.make_gcn_state(100, 4, 4, 1152, 128, "2d", 84)
    if kind == "discrete":
        return DC.make_discrete_state(36, 100, 85)
    if kind == "discrete_rot":
        return DR.make_rot_state(36, 100, 86)
    raise KeyError(kind)


def complete(sizes):
    return W.collate([W.dense_edge_index(n, True) for n in sizes], sizes)


def scripted(sides, seed):
    """A ragged Batch of Exphander puzzles at the scripted degree (60 %): a hybrid plan."""
    from diffassemble_amd import expander
    ei, batch, _ = expander.ragged_regular_batch(sides, 60, np.random.default_rng(seed))
    return ei, batch


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def timesteps(batch, steps, seed):
    n_graphs = int(batch.max()) + 1
    return torch.randint(0, steps, (n_graphs,), generator=torch.Generator().manual_seed(seed))[batch]


# name -> (state kind, engine keywords, da_config fields held while the engine is created and run, graph, call)
# call: "pose" forward; "alpha_last" / "alpha_all" forward with the attention weights; "idx" / "rot" the discrete models' forwards
def R(kind, prec, graph, call="pose", cfg=None, **eng):
    return dict(kind=kind, prec=prec, graph=graph, call=call, cfg=cfg or {}, eng=eng)


TWO36 = lambda: complete([36, 36])                                  # noqa: E731
ONE576 = lambda: complete([576])                                    # noqa: E731
SMALL_EXO = lambda: scripted([6, 16, 10, 20, 8, 18, 12, 14], 5)      # noqa: E731  (1 520 pieces: the virtual rows ride the masked launch)
EXO = dict(arch="exophormer", virt_nodes=8)
ROUTES = {
    # complete graphs, 36 pieces: both folds and the one-kernel tail (bf16); the folds one by one
    "tr36_bf16": R("tr", "bf16", TWO36),
    "tr36_fp32": R("tr", "fp32", TWO36),
    **{f"tr36_bf16_folds{b}": R("tr", "bf16", TWO36, cfg=dict(disable_folds=b)) for b in (1, 2, 3, 64, 128, 256)},
    # one 576-piece complete graph: hidden layers projected by their attention kernel, rows handed over fragment-major, Q of the last
    # layer projected in its attention kernel -- and each of the three switched off
    "tr576_bf16": R("tr", "bf16", ONE576),
    **{f"tr576_bf16_folds{b}": R("tr", "bf16", ONE576, cfg=dict(disable_folds=b)) for b in (64, 128, 256)},
    # exophormer over a hybrid plan below 8 192 pieces
    "exo_small_bf16": R("exo", "bf16", SMALL_EXO, **EXO),
    "exo_small_fp32": R("exo", "fp32", SMALL_EXO, **EXO),
    # the attention weights (edge list): of the last layer, of every layer
    "tr36_alpha_last": R("tr", "bf16", TWO36, call="alpha_last"),
    "tr36_alpha_all": R("tr", "bf16", TWO36, call="alpha_all"),
    "exo_small_alpha_all": R("exo", "fp32", SMALL_EXO, call="alpha_all", **EXO),
    # the two kill switches
    "tr36_no_dense": R("tr", "bf16", TWO36, cfg=dict(disable_dense=1)),
    "tr36_no_mfma": R("tr", "bf16", TWO36, cfg=dict(disable_mfma=1)),
    # the 3D model over 20-fragment objects (C = 104: one workgroup per graph, K | V in LDS)
    "3d_p20_bf16": R("3d", "bf16", lambda: complete([20, 7, 13]), variant="3d"),
    "3d_p20_fp32": R("3d", "fp32", lambda: complete([20, 7, 13]), variant="3d"),
    "gcn36_bf16": R("gcn", "bf16", TWO36, arch="gcn"),
    "discrete36_bf16": R("discrete", "bf16", TWO36, call="idx", variant="discrete"),
    "discrete36_fp32": R("discrete", "fp32", TWO36, call="idx", variant="discrete"),
    "discrete_rot36_bf16": R("discrete_rot", "bf16", TWO36, call="rot", variant="discrete_rot"),
}


def run_route(name, dev, profile=True):
    """-> (the forward's outputs as CPU tensors, {profile class: launches} without the classes that did not launch -- None unless `profile`)"""
    from diffassemble_amd import DenoiserEngine, _lib
    r = ROUTES[name]
    old = _lib.set_config(**r["cfg"])
    try:
        sd = state(r["kind"])
        eng = DenoiserEngine(sd, precision=r["prec"], device=dev, **r["eng"])
        ei, batch = r["graph"]()
        plan = eng.plan(ei.to(dev), batch.to(dev))
        n = plan.n_real
        t = timesteps(batch, eng.steps, 7).to(dev)
        feats = randn((n, eng.F), 8).to(dev)
        eng.profile(profile)
        if r["call"] == "idx":
            idx = torch.randint(0, 36, (n,), generator=torch.Generator().manual_seed(9))
            outs = [eng.forward_idx(plan, idx.to(dev), t, feats)]
        elif r["call"] == "rot":
            g = torch.Generator().manual_seed(9)
            idx, acc = torch.randint(0, 36, (n,), generator=g), torch.randint(0, 4, (n,), generator=g)
            feats4 = torch.stack([randn((n, eng.F), 8 + k) for k in range(4)]).to(dev)
            outs = list(eng.forward_rot(plan, idx.to(dev), t, feats4, rot_acc=acc.to(dev)))
        else:
            x = randn((n, eng.c_in), 9)
            if r["eng"].get("variant") == "3d":
                x[:, :4] = torch.nn.functional.normalize(x[:, :4], dim=-1)
            al = r["call"].startswith("alpha")
            res = eng.forward(plan, x.to(dev), t, feats, return_alpha=al, alpha_all_layers=r["call"] == "alpha_all")
            outs = list(res) if al else [res]
        torch.cuda.synchronize()
        counts = {k: v[1] for k, v in eng.profile_read().items() if v[1]} if profile else None
        eng.profile(False)
        return [o.cpu() for o in outs], counts
    finally:
        _lib.set_config(**{k: getattr(old, k) for k in r["cfg"]})


EXPECTED = {
    "tr36_bf16": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    "tr36_fp32": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 4},
    "tr36_bf16_folds1": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 2},
    "tr36_bf16_folds2": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "tr36_bf16_folds3": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 2},
    "tr36_bf16_folds64": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    "tr36_bf16_folds128": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    "tr36_bf16_folds256": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    # (conv_fused: a hidden layer that is ONE kernel, its attention kernel projecting it; linear_qkvs 1: the last layer's K | V' projection)
    "tr576_bf16": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 1, "conv_fused": 3, "attn_last": 1, "head": 1},
    "tr576_bf16_folds64": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    "tr576_bf16_folds128": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 1, "conv_fused": 3, "attn_last": 1, "head": 1},
    "tr576_bf16_folds256": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 1, "conv_fused": 3, "attn_last": 1, "head": 1},
    # (bf16: the virtual rows inside the masked launch, one attention launch per hidden layer; fp32: their own kernel behind it, two)
    "exo_small_bf16": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 1},
    "exo_small_fp32": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 6, "attn_last": 1, "head": 4},
    "tr36_alpha_last": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "tr36_alpha_all": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "exo_small_alpha_all": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "tr36_no_dense": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    # (no mfma: neither fold, mlp.2 runs; every layer tries the one-workgroup-per-graph kernel, which does not take C = 32 / 144, then the edge list)
    "tr36_no_mfma": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 4, "attn_hidden": 6, "attn_last": 2, "head": 2},
    "3d_p20_bf16": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 2},
    "3d_p20_fp32": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 2},
    "gcn36_bf16": {"embed": 1, "linear_mlp": 2, "linear_qkvs": 2, "attn_hidden": 1, "attn_last": 1, "head": 2},
    "discrete36_bf16": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "discrete36_fp32": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
    "discrete_rot36_bf16": {"embed": 1, "linear_mlp": 1, "linear_qkvs": 4, "attn_hidden": 3, "attn_last": 1, "head": 3},
}


def test_every_route_is_pinned():
    assert sorted(EXPECTED) == sorted(ROUTES)


@pytest.mark.parametrize("name", list(ROUTES))
def test_forward_launches_per_class(dev, name):
    outs, counts = run_route(name, dev)
    print(name, counts)
    assert all(torch.isfinite(o).all() for o in outs), name
    assert counts == EXPECTED[name], (name, counts, EXPECTED[name])
