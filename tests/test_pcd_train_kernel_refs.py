"""Host checks of the fp64 contracts of the 3D encoder's training passes (tests/golden/pcd_train_kernel_refs.py), no GPU:

  * composition: the contracts chained pass by pass over a stage (two layers, one layer), conv6 with the head in both
    ``inv`` settings and VnInv's statistics reproduce torch autograd of pcd_train_torch.torch_layer / torch_graph in fp64
    on the same neighbour lists to 1e-9 (max-abs error over max-abs reference), running statistics included;
  * sensitivity: the rule rejects every one of a list of subtly wrong contracts evaluated in fp32 and accepts the right
    contract evaluated in fp32 in another summation order;
  * the adjoint identity of premap and gather.
"""
import numpy as np
import pytest
import torch

import pcd_train_kernel_refs as K
import pcd_train_torch as PT
from oracle import weights as W

F32, F64 = torch.float32, torch.float64
MOM, BN_EPS = 0.1, 1e-5


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def state(feat, seed):
    return {k: v.double() for k, v in W.make_vn_dgcnn_state(feat, seed).items() if v.is_floating_point()}


def bn_of(sd, name):
    p = f"{name}.batchnorm.bn."
    return dict(gamma=sd[p + "weight"], beta=sd[p + "bias"], rm=sd[p + "running_mean"], rv=sd[p + "running_var"], mom=MOM, eps=BN_EPS)


def stage_operands(P, N, feat, two_layers, C, seed):
    """operands of one stage on the synthetic weights: stage 1 (C = 1, the points) or a 21-channel input map"""
    sd = state(feat, seed)
    a, b = ("conv1", "conv2") if C == 1 else (("conv3", "conv4") if two_layers else ("conv5", None))
    if C == 1 and not two_layers:
        b = None
    g = torch.Generator().manual_seed(seed)
    if C == 1:
        X = W.make_point_clouds(P, N, seed).double().reshape(P * N, 3)
    else:
        X = torch.zeros(P * N, K.ROW, dtype=F64)
        X[:, :K.V3] = 0.3 * torch.randn(P * N, K.V3, generator=g, dtype=F64)
    wfa, wda = sd[f"{a}.map_to_feat.weight"], sd[f"{a}.map_to_dir.weight"]
    ops = dict(X=X, C=C, N=N, idx=K.knn_lists(X[:, :3 * C], N), Wm=K.pack_premap(wfa, wda, C), bn_a=bn_of(sd, a), wb=None, bn_b=None,
               G=torch.randn(P * N, K.VC, 3, generator=g, dtype=F64))
    w = dict(wfa=wfa, wda=wda)
    if b is not None:
        w.update(wfb=sd[f"{b}.map_to_feat.weight"], wdb=sd[f"{b}.map_to_dir.weight"])
        ops.update(wb=K.pack_wb(w["wfb"], w["wdb"]), bn_b=bn_of(sd, b))
    return ops, w


def autograd_stage(ops, w, P):
    """the same stage through pcd_train_torch in fp64 -> the quantities stage_chain returns"""
    N, C = ops["N"], ops["C"]
    x = ops["X"][:, :3 * C].reshape(P, N, C, 3).clone().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    bns = {"a": ops["bn_a"], "b": ops["bn_b"]}
    aff = {t: {k: bns[t][k].clone().requires_grad_(True) for k in ("gamma", "beta")} for t in bns if bns[t] is not None}
    feat = PT.torch_graph(x)
    # the lists torch_graph selects are the lists the contracts were given
    j = K.glob(ops["idx"], N).view(P, N, K.KNN)
    xf = x.detach().reshape(P * N, C, 3)
    mine = torch.cat([xf[j] - xf.view(P, N, 1, C, 3), xf.view(P, N, 1, C, 3).expand(P, N, K.KNN, C, 3)], 3)
    assert torch.equal(mine, feat.detach())
    e = (0, 1, 2)
    out, h = {}, feat
    for t in ("a", "b"):
        if bns[t] is None:
            continue
        wf, wd = leaves[f"wf{t}"], leaves[f"wd{t}"]
        n = torch.einsum("oc,...ck->...ok", wf, h).detach().norm(dim=-1) + 1e-6
        cnt = n[..., 0].numel()
        out[f"run_mean_{t}"] = (1 - MOM) * bns[t]["rm"] + MOM * n.mean(e)
        out[f"run_var_{t}"] = (1 - MOM) * bns[t]["rv"] + MOM * n.var(e, unbiased=False) * cnt / (cnt - 1)
        h = PT.torch_layer(h, wf, wd, aff[t]["gamma"], aff[t]["beta"], e, eps=BN_EPS)
    y = h.mean(2)                                                           # [P, N, 21, 3]
    (y * ops["G"].view(P, N, K.VC, 3)).sum().backward()
    out["X"] = torch.nn.functional.pad(y.detach().reshape(P * N, K.V3), (0, 1))
    dx = x.grad.reshape(P * N, C, 3)
    out["dXp"] = dx.reshape(-1) if C == 1 else K.to_cmajor(dx)
    for t in aff:
        out[f"dwf_{t}"], out[f"dwd_{t}"] = leaves[f"wf{t}"].grad, leaves[f"wd{t}"].grad
        out[f"dgamma_{t}"], out[f"dbeta_{t}"] = aff[t]["gamma"].grad, aff[t]["beta"].grad
    return out


@pytest.mark.parametrize("P,N,feat,two,C", [(3, 70, 32, True, 1), (2, 40, 8, True, 21), (2, 45, 8, False, 21)],
                         ids=["conv1-conv2", "conv3-conv4", "conv5"])
def test_stage_composition_matches_autograd(P, N, feat, two, C):
    ops, w = stage_operands(P, N, feat, two, C, seed=P + N)
    got, _, op = K.stage_chain(dt=F64, **ops)
    ref = autograd_stage(ops, w, P)
    assert set(ref) <= set(got)
    for k in sorted(ref):
        e = rel(got[k].reshape(ref[k].shape), ref[k])
        print(f"[pcd-refs] stage {k}: {e:.2e}")
        assert e <= 1e-9, (k, e)
    print(f"[pcd-refs] open share {op.share:.2e}")
    op.assert_cap("composition")


@pytest.mark.parametrize("inv", [0, 1])
def test_conv6_and_head_composition_matches_autograd(inv):
    P, N, feat = 3, 50, 8
    sd = state(feat, 5)
    g = torch.Generator().manual_seed(11 + inv)
    X = [torch.nn.functional.pad(0.3 * torch.randn(P * N, K.V3, generator=g, dtype=F64), (0, 1)) for _ in range(3)]
    w6, wd6 = sd["conv6.map_to_feat.weight"], sd["conv6.map_to_dir.weight"]
    lin_w, lin_b = sd["linear0.weight"], sd["linear0.bias"]
    bn = bn_of(sd, "conv6")
    blob = K.pack_w6(w6, wd6)
    G = torch.randn(P, 2 * feat if inv else 6 * feat, generator=g, dtype=F64)
    # ---- contracts
    fin = K.bn_fin_fwd(K.c6_stat(*X, blob, feat)["partial"], float(P * N), bn["gamma"], bn["beta"], MOM, BN_EPS, bn["rm"], bn["rv"])
    rec = K.fin_to_rec(fin, bn["gamma"], bn["beta"])
    dm = K.head_bwd(G, inv, feat, torch.cat([lin_w.reshape(-1), lin_b]))["dm"]
    fb = K.bn_fin_bwd(K.c6_bwd(1, *X, blob, feat, N, rec, dm)["partial"], float(P * N), torch.zeros(feat, dtype=F64), torch.zeros(feat, dtype=F64))
    rec[K.R_MDY, :feat], rec[K.R_MDYX, :feat] = fb["mdy"], fb["mdyx"]
    b2 = K.c6_bwd(2, *X, blob, feat, N, rec, dm)
    dxs = K.c6_dx(torch.nn.functional.pad(b2["G6"], (0, K.g6_ld(feat) - feat - 1)), blob, feat)
    dw6 = K.gemm_tn(b2["G6"][:, :feat], b2["F"][:, :K.V3], torch.zeros(feat, K.V3, dtype=F64))["C"]
    dwd6 = K.gemm_tn(b2["G6"][:, feat:], b2["F"][:, :K.V3], torch.zeros(1, K.V3, dtype=F64))["C"]
    # ---- autograd
    xs = [x[:, :K.V3].reshape(P, N, K.VC, 3).clone().requires_grad_(True) for x in X]
    lv = [t.clone().requires_grad_(True) for t in (w6, wd6, bn["gamma"], bn["beta"], lin_w, lin_b)]
    cat = torch.cat(xs, 2)
    m = PT.torch_layer(cat, lv[0], lv[1], lv[2], lv[3], (0, 1), eps=BN_EPS).mean(1)
    y = torch.cat([m, m], 1)
    out = (y @ lv[4].T + lv[5]).mean(1) if inv else y.reshape(P, -1)
    (out * G).sum().backward()
    n = torch.einsum("oc,...ck->...ok", w6, cat.detach()).norm(dim=-1) + 1e-6
    pairs = {"run_mean": (fin["run_mean"], (1 - MOM) * bn["rm"] + MOM * n.mean((0, 1))),
             "run_var": (fin["run_var"], (1 - MOM) * bn["rv"] + MOM * n.var((0, 1), unbiased=True)),
             "dw6": (dw6, lv[0].grad), "dwd6": (dwd6, lv[1].grad), "dgamma": (fb["dgamma"], lv[2].grad), "dbeta": (fb["dbeta"], lv[3].grad)}
    for i in range(3):
        pairs[f"dX{i + 1}"] = (dxs[f"dX{i + 1}"][:, :K.VC], K.to_cmajor(xs[i].grad.reshape(P * N, K.VC, 3))[:, :K.VC])
    if inv:
        M = torch.cat([m, m], 1).detach().reshape(P, -1)
        lg = K.lin0_grad(G, M, feat, torch.zeros(2 * feat * 3, dtype=F64), torch.zeros(2 * feat, dtype=F64))
        pairs.update(dW0=(lg["dW0"], lv[4].grad), db0=(lg["db0"], lv[5].grad))
    for k, (a, b) in pairs.items():
        e = rel(a.reshape(b.shape), b)
        print(f"[pcd-refs] conv6 inv={inv} {k}: {e:.2e}")
        assert e <= 1e-9, (k, e)


def test_vn_inv_statistics_match_torch():
    P, feat = 5, 8
    sd = state(feat, 2)
    g = torch.Generator().manual_seed(3)
    M = torch.randn(P, 6 * feat, generator=g, dtype=F64)
    x = M.view(P, 2 * feat, 3)
    for v, (name, cin, cout) in enumerate((("VnInv.vn1", 2 * feat, feat), ("VnInv.vn2", feat, feat // 2))):
        wf, wd, bn = sd[f"{name}.map_to_feat.weight"], sd[f"{name}.map_to_dir.weight"], bn_of(sd, name)
        rows = x.reshape(P, -1)
        lin = K.vn_lin(rows, wf, wd, cin)
        fin = K.bn_fin_fwd(K.vn_stat(lin["vP"])["partial"], float(P), bn["gamma"], bn["beta"], MOM, BN_EPS, bn["rm"], bn["rv"])
        n = torch.einsum("oc,pck->pok", wf, x).norm(dim=-1) + 1e-6
        assert rel(fin["run_mean"], (1 - MOM) * bn["rm"] + MOM * n.mean(0)) <= 1e-9
        assert rel(fin["run_var"], (1 - MOM) * bn["rv"] + MOM * n.var(0, unbiased=True)) <= 1e-9
        y = K.vn_apply(lin["vP"], lin["vD"], K.fin_to_rec(fin, bn["gamma"], bn["beta"]))["vY"]
        assert rel(y, PT.torch_layer(x, wf, wd, bn["gamma"], bn["beta"], (0,), eps=BN_EPS)) <= 1e-9
        x = y


def test_premap_gather_adjoint():
    """<dT, premap(x)> == <gather_dx(dT), x> in fp64, with E assembled so that the gathered dT is a given dT: the premap
    is linear in x and the gather's dXp is its transpose applied to dT."""
    P, N = 2, 30
    g = torch.Generator().manual_seed(9)
    for C in (1, K.VC):
        X = torch.randn(P * N, 3 * C, generator=g, dtype=F64)
        Wm = torch.randn(4 * K.VC * C, generator=g, dtype=F64)
        idx = K.hub_lists(P, N, 4)
        E = torch.randn(P * N * K.KNN, K.E_LD, generator=g, dtype=F64)
        E[:, K.V3], E[:, K.ROW + K.V3] = 0, 0
        cnt, ptr, rev = (torch.from_numpy(v) for v in K.rev_adj(idx.numpy(), N))
        zero = torch.zeros(P * N * 3 if C == 1 else P * N * 3 * K.ROW, dtype=F64)
        ga = K.gather(E, cnt, rev, Wm, X, C, zero)
        dT = ga["dTc"].view(P * N, 3, 4, K.VC).permute(0, 2, 3, 1)                     # [pts, 4, 21, 3]
        T = K.segs(K.premap(X, Wm, C)["T"])
        lhs = float((dT * T).sum())
        dx = ga["dXp"].view(P * N, 3) if C == 1 else ga["dXp"].view(P * N, 3, K.ROW)[:, :, :C].transpose(1, 2)
        rhs = float((dx.reshape(P * N, C, 3) * X.view(P * N, C, 3)).sum())
        assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + 1), (C, lhs, rhs)
        # and the gathered dT is the scatter of the edges: every edge's dp_a lands at its END point, its own sums at the source
        j = K.glob(idx, N).reshape(-1)
        into = torch.zeros(P * N, K.V3, dtype=F64).index_add_(0, j, E[:, :K.V3])
        assert torch.allclose(dT[:, 0].reshape(P * N, K.V3), into, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.fixture(scope="module")
def edge_ops():
    """operands of the backward edge passes of a two-layer stage (fp32 values as the kernels store them), records complete"""
    P, N = 3, 100
    ops, _ = stage_operands(P, N, 32, True, 1, seed=7)
    f32 = lambda t: t.float().double()                                     # noqa: E731
    X, Wm, wb = f32(ops["X"]), f32(ops["Wm"]), f32(ops["wb"])
    T = f32(K.premap(X, Wm, 1)["T"])
    idx = ops["idx"]
    cnt = float(P * N * K.KNN)
    fa = K.bn_fin_fwd(K.edge_stat_a(T, idx, N)["partial"], cnt, *[ops["bn_a"][k] for k in ("gamma", "beta", "mom", "eps", "rm", "rv")])
    recA = f32(K.fin_to_rec(fa, ops["bn_a"]["gamma"], ops["bn_a"]["beta"]))
    fb = K.bn_fin_fwd(K.edge_stat_b(T, idx, N, recA, wb)["partial"], cnt, *[ops["bn_b"][k] for k in ("gamma", "beta", "mom", "eps", "rm", "rv")])
    recB = f32(K.fin_to_rec(fb, ops["bn_b"]["gamma"], ops["bn_b"]["beta"]))
    dX = f32(K.to_cmajor(ops["G"]).reshape(-1))
    z = torch.zeros(K.VC, dtype=F64)
    b1 = K.bn_fin_bwd(K.edge_bwd(1, T, idx, N, recA, recB, wb, dX)["partial"], cnt, z, z)
    recB[K.R_MDY, :K.VC], recB[K.R_MDYX, :K.VC] = f32(b1["mdy"]), f32(b1["mdyx"])
    b2 = K.bn_fin_bwd(K.edge_bwd(2, T, idx, N, recA, recB, wb, dX)["partial"], cnt, z, z)
    recA[K.R_MDY, :K.VC], recA[K.R_MDYX, :K.VC] = f32(b2["mdy"]), f32(b2["mdyx"])
    return dict(T=T.float(), idx=idx, N=N, recA=recA.float(), recB=recB.float(), wb=wb.float(), dX=dX.float(), X=X.float(), Wm=Wm.float(), P=P)


def _edge(mode, o, dt, **kw):
    c = lambda t: t.to(dt)                                                 # noqa: E731
    r = K.edge_bwd(mode, c(o["T"]), o["idx"], o["N"], c(o["recA"]), c(o["recB"]), c(o["wb"]), c(o["dX"]), **kw)
    r.pop("_open")
    return r


def verdicts(ref, S, plain, wrong, masks=None):
    return {k: K.judge_pass(wrong[k], ref[k], S[k], plain[k], mask=None if masks is None else masks.get(k)) for k in wrong if k in ref}


@pytest.mark.parametrize("mode,defect,key", [(3, "c079", "E"), (2, "c079", "Gb"), (3, "no_ddsq2", "E"), (2, "no_ddsq2", "Gb"),
                                             (3, "no_dyy", "E"), (2, "no_dyy", "Gb"), (1, "c079", "partial")])
def test_rule_rejects_wrong_activation_backward(edge_ops, mode, defect, key):
    o = edge_ops
    ref, S, plain, slack, masks, op = K.edge_case(mode, o["T"], o["idx"], o["N"], o["recA"], o["recB"], o["wb"], o["dX"])
    right = verdicts(ref, S, plain, plain, masks)
    assert all(j["ok"] for j in right.values()), right
    wrong = _edge(mode, o, F32, defect=(defect,))
    j = K.judge_pass(wrong[key], ref[key], S[key], plain[key], mask=masks.get(key), slack=slack.get(key))
    print(f"[pcd-refs] {defect} in pass {mode}: {j['bad']}/{j['n']} over the bound, e {j['e_hip']:.2e} vs e_acc {j['e_acc']:.2e}")
    assert not j["ok"] and j["e_hip"] > 16 * j["e_acc"]


def test_rule_accepts_another_summation_order(edge_ops):
    """the right contracts in fp32 with the 20 edges of every point walked in reverse: block sums and gathers add in
    another order"""
    o = edge_ops
    rev_o = dict(o, idx=o["idx"].flip(1))
    for mode in (1, 2):
        ref, S, plain, slack, masks, _ = K.edge_case(mode, o["T"], o["idx"], o["N"], o["recA"], o["recB"], o["wb"], o["dX"])
        other = _edge(mode, rev_o, F32)
        j = K.judge_pass(other["partial"], ref["partial"], S["partial"], plain["partial"], slack=slack.get("partial"))
        assert j["ok"] and j["e_hip"] > 0, j                               # (it IS another order: not bitwise the plain evaluation)
    E = _edge(3, o, F64)["E"].float()
    cnt, ptr, rev = (torch.from_numpy(v) for v in K.rev_adj(o["idx"].numpy(), o["N"]))
    pts = cnt.numel()
    z = torch.zeros(pts * 3)
    ref, S, plain = K.evaluate(K.gather, E, cnt, rev, o["Wm"], o["X"], 1, z)
    # every point's incoming list reversed
    rr = rev.clone()
    for j0, c in zip(ptr.tolist(), cnt.tolist()):
        rr[j0:j0 + c] = rev[j0:j0 + c].flip(0)
    other = K.gather(E, cnt, rr, o["Wm"], o["X"], 1, z)
    for k in ("dTc", "dXp"):
        assert K.judge_pass(other[k], ref[k], S[k], plain[k])["ok"], k
    wrong = K.gather(E, cnt, rev, o["Wm"], o["X"], 1, z, drop_edge=int(ptr[5]))       # one incoming edge of point 5 lost
    j = K.judge_pass(wrong["dTc"], ref["dTc"], S["dTc"], plain["dTc"])
    assert not j["ok"] and j["bad"] <= 2 * K.V3, j


def test_rule_rejects_wrong_statistics(edge_ops):
    o = edge_ops
    cnt = float(o["P"] * o["N"] * K.KNN)
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.rand(K.VC, generator=g) + 0.5, torch.randn(K.VC, generator=g)
    rm, rv = torch.rand(K.VC, generator=g), torch.rand(K.VC, generator=g) + 0.1
    part = K.edge_stat_a(o["T"].double(), o["idx"], o["N"])["partial"]
    ref, S, plain = K.evaluate(K.bn_fin_fwd, part, cnt, gamma, beta, MOM, BN_EPS, rm, rv)
    shuffled = K.bn_fin_fwd(part.flip(0).float(), cnt, gamma, beta, MOM, BN_EPS, rm, rv)
    assert all(K.judge_pass(shuffled[k], ref[k], S[k], plain[k])["ok"] for k in ref)
    # biased instead of unbiased running variance: n / (n - 1) is 1 + 1.7e-4 at this count, times momentum 0.1 times a variance
    # far below the running one -- under the fp32 evaluation's own error of E n^2 - mean^2.  It shows where the count is small:
    # VnInv's BatchNorm1d over the fragments, count = 2 (the unbiased variance is twice the biased one) and count = 5
    p2 = torch.tensor([[[3.0, 1.0], [5.0, 0.5]]], dtype=F64)
    r2, S2, pl2 = K.evaluate(K.bn_fin_fwd, p2, 2.0, gamma[:2], beta[:2], MOM, BN_EPS, rm[:2], rv[:2])
    w2 = K.bn_fin_fwd(p2.float(), 2.0, gamma[:2], beta[:2], MOM, BN_EPS, rm[:2], rv[:2], biased=True)
    assert not K.judge_pass(w2["run_var"], r2["run_var"], S2["run_var"], pl2["run_var"])["ok"]
    assert K.judge_pass(pl2["run_var"], r2["run_var"], S2["run_var"], pl2["run_var"])["ok"]
    p5 = torch.tensor([[[2.5, 1.0], [1.75, 0.3]]], dtype=F64)
    r5, S5, pl5 = K.evaluate(K.bn_fin_fwd, p5, 5.0, gamma[:2], beta[:2], MOM, BN_EPS, rm[:2], rv[:2])
    w5 = K.bn_fin_fwd(p5.float(), 5.0, gamma[:2], beta[:2], MOM, BN_EPS, rm[:2], rv[:2], biased=True)
    assert not K.judge_pass(w5["run_var"], r5["run_var"], S5["run_var"], pl5["run_var"])["ok"]
    # mean(dy xhat) over count - 1
    bp = K.edge_bwd(1, o["T"].double(), o["idx"], o["N"], o["recA"].double(), o["recB"].double(), o["wb"].double(), o["dX"].double())["partial"]
    z = torch.zeros(K.VC)
    ref, S, plain = K.evaluate(K.bn_fin_bwd, bp, cnt, z, z)
    wrong = K.bn_fin_bwd(bp.float(), cnt, z, z, count_minus_one=True)
    assert not K.judge_pass(wrong["mdyx"], ref["mdyx"], S["mdyx"], plain["mdyx"])["ok"]
    assert K.judge_pass(wrong["mdy"], ref["mdy"], S["mdy"], plain["mdy"])["ok"]


def test_rule_rejects_wrong_sums_and_maps(edge_ops):
    o = edge_ops
    # the last channel (20) of layer b left at zero
    ref, S, plain = K.evaluate(K.edge_stat_b, o["T"], o["idx"], o["N"], o["recA"], o["wb"])
    wrong = K.edge_stat_b(o["T"], o["idx"], o["N"], o["recA"], o["wb"], zero_last=True)
    j = K.judge_pass(wrong["partial"], ref["partial"], S["partial"], plain["partial"])
    assert not j["ok"] and j["bad"] == 2 * ref["partial"].shape[0], j       # channel 20 of both sums of every block
    # a tail lane's value added to a block sum: the last point's sums counted once more in the last (partial) block
    ref, S, plain = K.evaluate(K.edge_stat_a, o["T"], o["idx"], o["N"])
    p, _ = K.edge_inputs(o["T"].double(), o["idx"], o["N"])
    n_last = ((p.v[-1] * p.v[-1]).sum(-1).sqrt() + K.EPS).sum(0)
    wrong = plain["partial"].clone()
    wrong[-1, 0] += n_last.float()
    j = K.judge_pass(wrong, ref["partial"], S["partial"], plain["partial"])
    assert not j["ok"] and j["bad"] == K.VC, j
    # the U share of dW[:, :C] not subtracted
    g = torch.Generator().manual_seed(2)
    for C in (1, K.VC):
        dWm, f0, d0 = (torch.randn(n, generator=g) for n in (4 * K.VC * C, 2 * K.VC * C, 2 * K.VC * C))
        ref, S, plain = K.evaluate(K.premap_wgrad, dWm, C, f0, d0)
        assert all(K.judge_pass(plain[k], ref[k], S[k], plain[k])["ok"] for k in ref)
        wrong = K.premap_wgrad(dWm, C, f0, d0, keep_u=True)
        assert not K.judge_pass(wrong["dwf"], ref["dwf"], S["dwf"], plain["dwf"])["ok"]
        assert not K.judge_pass(wrong["dwd"], ref["dwd"], S["dwd"], plain["dwd"])["ok"]


def test_reverse_adjacency_reference():
    """the numpy counting sort against a direct enumeration, with a hub (cnt = N) and an orphan (cnt = 0) per cloud"""
    P, N = 2, 23
    idx = K.hub_lists(P, N, 0)
    cnt, ptr, rev = K.rev_adj(idx.numpy(), N)
    j = K.glob(idx, N).reshape(-1).numpy()
    for q in range(P * N):
        assert list(rev[ptr[q]:ptr[q] + cnt[q]]) == [e for e in range(P * N * K.KNN) if j[e] == q]
    assert cnt[0] == N and cnt[N] == N and cnt[N - 1] == 0 and cnt[2 * N - 1] == 0 and int(cnt.sum()) == P * N * K.KNN
    assert np.array_equal(np.sort(K.perm_lists(2, 20, 1).numpy(), 1), np.tile(np.arange(20), (40, 1)))


def test_pass_args_layout_matches_the_c_header(tmp_path):
    """da_pcd_pass_args as plain C sees it == the ctypes mirror, and the pass names follow the header's enum"""
    import ctypes
    import os
    import re
    import subprocess
    from diffassemble_amd import _lib
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    lines = ['printf("size %zu\\n", sizeof(da_pcd_pass_args));']
    lines += [f'printf("{n} %zu\\n", offsetof(da_pcd_pass_args, {n}));' for n, _ in _lib.DaPcdPassArgs._fields_]
    lines += [f'printf("pass_{n} %d\\n", DA_PCD_PASS_{n});' for n in _lib.PCD_PASSES]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "diffassemble_hip.h"\nint main(void){' + "".join(lines) + "return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.DaPcdPassArgs)
    for n, _ in _lib.DaPcdPassArgs._fields_:
        assert int(got[n]) == getattr(_lib.DaPcdPassArgs, n).offset, n
    for i, n in enumerate(_lib.PCD_PASSES):
        assert int(got[f"pass_{n}"]) == i, n
    hdr = open(os.path.join(inc, "diffassemble_hip.h")).read()
    assert len(re.findall(r"DA_PCD_PASS_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) == len(_lib.PCD_PASSES)
