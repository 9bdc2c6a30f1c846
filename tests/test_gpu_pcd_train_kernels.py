"""Kernel-level parity tests of the 3D piece encoder's training passes (da_pcd_train_pass: the launch code of
da_pcd_train_forward / da_pcd_train_backward, one pass at a time) and of da_gemm_tn_f32 at this path's operand shapes.

Every pass is held against its fp64 contract on the STORED operands (tests/golden/pcd_train_kernel_refs.py, pinned by
tests/test_pcd_train_kernel_refs.py) under the rule of tests/golden/encoder_kernel_refs.py,

    |got_i - ref_i| <= 2^-24 |ref_i| + FACTOR e_acc(plain) S_i        for every element i of every output,

FACTOR = 16, S_i the contract's condition term, e_acc(plain) the error of the same contract evaluated by torch in fp32 on
the CPU, per case, never from the HIP output.  Leaky-ReLU decisions with |cos(q, d)| < 1e-4 in fp64 are open: their per-edge
outputs are left out, sums get the flipped-decision slack; every case asserts from the reference alone that at most 1e-3 of
its decisions are open.  Passes that only move or count (the reverse adjacency, the F / Xc rows, zeroed pad columns) are
compared exactly; Hb holds layer b's COMPUTED input h (the activation of layer a), so it is judged by the rule.  Destination
buffers are pre-filled with a sentinel and carry guard rows: an unwritten row, a tail lane's write and a touched pad column
all show.  Shapes are the smallest at which each kernel can still go wrong.  Every case prints e(HIP), e_acc(plain) and the
open share (run with -s).
"""
import numpy as np
import pytest
import torch

import pcd_train_kernel_refs as K
from oracle import weights as W

pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT = 7.0
MOM, BN_EPS = float(np.float32(0.1)), float(np.float32(1e-5))
RATIOS = {}                                                  # pass -> worst e(HIP) / e_acc(plain) seen (printed by the last test)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def lib():
    from diffassemble_amd import _lib
    return _lib


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def sent(dev, *shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def check(tag, kernel, got, ref, S, plain, slack=None, masks=None, op=None):
    """judge every output of ``ref`` by the rule; print the figures; assert at the end"""
    fails = []
    for k in ref:
        j = K.judge_pass(got[k], ref[k], S[k], plain[k], kernel=kernel, slack=(slack or {}).get(k), mask=(masks or {}).get(k))
        ratio = j["e_hip"] / j["e_acc"] if j["e_acc"] > 0 else (0.0 if j["e_hip"] == 0 else float("inf"))
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
        share = "" if op is None else f"  open {op.n_open}/{op.total} ({op.share:.1e})"
        print(f"[pcd-kernels] {tag} {k}: e(HIP) {j['e_hip']:.3e}  e_acc(plain) {j['e_acc']:.3e}  ratio {ratio:.2f}  over the bound "
              f"{j['bad']}/{j['n']}  left out {j['left_out']}{share}")
        if not j["ok"]:
            fails.append((k, j))
    assert not fails, (tag, fails)


def state(feat, seed):
    return {k: v for k, v in W.make_vn_dgcnn_state(feat, seed).items() if v.is_floating_point()}


def bn_of(sd, name):
    p = f"{name}.batchnorm.bn."
    return dict(gamma=sd[p + "weight"], beta=sd[p + "bias"], rm=sd[p + "running_mean"], rv=sd[p + "running_var"], mom=MOM, eps=BN_EPS)


# ------------------------------------------------------------------------------------------------ operands of a stage
EDGE_SHAPES = [(2, 20, "perm"), (3, 100, "knn"), (2, 128, "hub"), (2, 300, "knn")]
_STAGE = {}


def stage(P, N, lists, C=1):
    """stored operands (fp32, CPU) of one stage: premap rows, lists, both layers' complete records, the pooled gradient.
    The records come from the fp64 chain of the contracts, rounded to fp32.  The (3, 100) case has a point at the origin
    (its self edge is a zero vector)."""
    key = (P, N, lists, C)
    if key in _STAGE:
        return _STAGE[key]
    seed = 100 * P + N
    g = gen(seed)
    sd = state(8, seed)
    if C == 1:
        X = W.make_point_clouds(P, N, seed).reshape(P * N, 3).clone()
        if (P, N) == (3, 100):
            X[0] = 0.0
        a, b = "conv1", "conv2"
    else:
        X = torch.zeros(P * N, K.ROW)
        X[:, :K.V3] = 0.3 * randn(g, P * N, K.V3)
        a, b = "conv3", "conv4"
    idx = {"perm": lambda: K.perm_lists(P, N, seed), "hub": lambda: K.hub_lists(P, N, seed),
           "knn": lambda: K.knn_lists(X[:, :3 * C], N)}[lists]()
    if (P, N) == (3, 100) and C == 1:
        assert 0 in idx[0].tolist()                                          # the origin's self edge
    Wm = K.pack_premap(sd[f"{a}.map_to_feat.weight"], sd[f"{a}.map_to_dir.weight"], C)
    wb = K.pack_wb(sd[f"{b}.map_to_feat.weight"], sd[f"{b}.map_to_dir.weight"])
    T = K.premap(X, Wm, C)["T"]                                              # fp32 on the CPU: the stored premap rows
    dX = randn(g, P * N * 3 * K.ROW)
    o = dict(P=P, N=N, C=C, X=X, idx=idx, Wm=Wm, wb=wb, T=T, dX=dX, bn_a=bn_of(sd, a), bn_b=bn_of(sd, b))
    cnt = float(P * N * K.KNN)
    d = lambda t: t.double()                                                 # noqa: E731
    z = torch.zeros(K.VC, dtype=F64)

    def fwd_rec(part, bn):
        f = K.bn_fin_fwd(part, cnt, d(bn["gamma"]), d(bn["beta"]), MOM, BN_EPS, d(bn["rm"]), d(bn["rv"]))
        return K.fin_to_rec(f, d(bn["gamma"]), d(bn["beta"])).float()

    for hb in (True, False):
        w = d(wb) if hb else None
        recA = fwd_rec(K.edge_stat_a(d(T), idx, N)["partial"], o["bn_a"])
        recB = fwd_rec(K.edge_stat_b(d(T), idx, N, d(recA), d(wb))["partial"], o["bn_b"]) if hb else None
        last = recB if hb else recA
        f = K.bn_fin_bwd(K.edge_bwd(1, d(T), idx, N, d(recA), None if recB is None else d(recB), w, d(dX))["partial"], cnt, z, z)
        last[K.R_MDY, :K.VC], last[K.R_MDYX, :K.VC] = f["mdy"].float(), f["mdyx"].float()
        if hb:
            f = K.bn_fin_bwd(K.edge_bwd(2, d(T), idx, N, d(recA), d(recB), w, d(dX))["partial"], cnt, z, z)
            recA[K.R_MDY, :K.VC], recA[K.R_MDYX, :K.VC] = f["mdy"].float(), f["mdyx"].float()
        o["rec", hb] = (recA, recB)
    _STAGE[key] = o
    return o


def run_edge(lib, dev, name, o, hb, recA, recB):
    """one edge pass on device copies -> dict of the written buffers (with guards)"""
    pts = o["P"] * o["N"]
    ne, nb = pts * K.KNN, (pts + 255) // 256
    buf = dict(partial=sent(dev, nb + 1, 2, K.VC, dtype=F64), Gb=sent(dev, ne * 3 + 64, K.GB_LD), Hb=sent(dev, ne * 3 + 64, K.H_LD),
               E=sent(dev, ne + 64, K.E_LD))
    keep = [t.to(dev) for t in (o["T"], o["idx"], recA, recB if recB is not None else recA, o["wb"], o["dX"])]
    lib.pcd_train_pass(name, n_parts=o["P"], n_points=o["N"], has_b=int(hb), T=keep[0], idx=keep[1], rec_a=keep[2],
                       rec_b=keep[3] if hb else None, w=keep[4] if hb else None, dX_in=keep[5], **buf)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in buf.items()}


@pytest.mark.parametrize("P,N,lists", EDGE_SHAPES, ids=[f"p{p}_n{n}_{l}" for p, n, l in EDGE_SHAPES])
def test_pt_edge_every_mode(P, N, lists, lib, dev):
    """k_pt_edge: STAT_A, BWD1, BWD3 with and without layer b; STAT_B, BWD2 with it."""
    o = stage(P, N, lists)
    pts, ne, nb = P * N, P * N * K.KNN, (P * N + 255) // 256
    T, idx, wb, dX = o["T"], o["idx"], o["wb"], o["dX"]
    for hb in (True, False):
        recA, recB = o["rec", hb]
        w = wb if hb else None
        tag = f"edge p{P}_n{N}_{lists} b={int(hb)}"
        # ---- statistics
        got = run_edge(lib, dev, "EDGE_STAT_A", o, hb, recA, recB)
        ref, S, plain = K.evaluate(K.edge_stat_a, T, idx, N)
        check(f"{tag} STAT_A", "edge_stat", {"partial": got["partial"][:nb]}, ref, S, plain)
        assert bool((got["partial"][nb] == SENT).all()) and all(bool((got[k] == SENT).all()) for k in ("Gb", "Hb", "E"))
        if hb:
            got = run_edge(lib, dev, "EDGE_STAT_B", o, hb, recA, recB)
            ref, S, plain = K.evaluate(K.edge_stat_b, T, idx, N, recA, wb)
            check(f"{tag} STAT_B", "edge_stat", {"partial": got["partial"][:nb]}, ref, S, plain)
            assert bool((got["partial"][nb] == SENT).all())
        # ---- backward
        for mode in ((1, 2, 3) if hb else (1, 3)):
            got = run_edge(lib, dev, f"EDGE_BWD{mode}", o, hb, recA, recB)
            ref, S, plain, slack, masks, op = K.edge_case(mode, T, idx, N, recA, recB, w, dX)
            g = {}
            if "partial" in ref:
                g["partial"] = got["partial"][:nb]
                assert bool((got["partial"][nb] == SENT).all())
            else:
                assert bool((got["partial"] == SENT).all())
            if mode == 2:
                g["Gb"], g["Hb"] = got["Gb"][:ne * 3, :2 * K.VC], got["Hb"][:ne * 3, :K.VC]
                assert bool((got["Gb"][:, 2 * K.VC:] == SENT).all()) and bool((got["Gb"][ne * 3:] == SENT).all())
                assert bool((got["Hb"][:, K.VC:] == SENT).all()) and bool((got["Hb"][ne * 3:] == SENT).all())
            else:
                assert bool((got["Gb"] == SENT).all()) and bool((got["Hb"] == SENT).all())
            if mode == 3:
                g["E"] = got["E"][:ne]
                assert bool((got["E"][ne:] == SENT).all())
                assert bool((g["E"][:, K.V3] == 0).all()) and bool((g["E"][:, K.ROW + K.V3] == 0).all())
                assert bool(torch.isfinite(g["E"]).all())
            else:
                assert bool((got["E"] == SENT).all())
            check(f"{tag} BWD{mode}", f"edge_bwd{mode}", g, ref, S, plain, slack, masks, op)
    if (P, N) == (3, 100):
        # the origin's self edge: a zero vector, no gradient through the norm -- dp_a of that edge is exactly (y / n) dq
        e0 = idx[0].tolist().index(0)
        p, d = K.edge_inputs(T.double(), idx, N)
        assert bool((p.v[0, e0] == 0).all())


def test_pt_edge_21_channel_input(lib, dev):
    """the same passes on a 21-channel stage (premap of a map, not of the points), all modes with layer b"""
    o = stage(2, 100, "knn", C=K.VC)
    recA, recB = o["rec", True]
    nb, ne = 1, 200 * K.KNN
    for mode in (1, 2, 3):
        got = run_edge(lib, dev, f"EDGE_BWD{mode}", o, True, recA, recB)
        ref, S, plain, slack, masks, op = K.edge_case(mode, o["T"], o["idx"], o["N"], recA, recB, o["wb"], o["dX"])
        g = {k: {"partial": got["partial"][:nb], "Gb": got["Gb"][:ne * 3, :2 * K.VC], "Hb": got["Hb"][:ne * 3, :K.VC], "E": got["E"][:ne]}[k] for k in ref}
        check(f"edge c21 BWD{mode}", f"edge_bwd{mode}", g, ref, S, plain, slack, masks, op)


# ------------------------------------------------------------------------------------------------ premap
@pytest.mark.parametrize("C,pts", [(1, 40), (1, 300), (K.VC, 300)])
def test_premap(C, pts, lib, dev):
    g = gen(C + pts)
    ldx = 3 if C == 1 else K.ROW
    X = randn(g, pts, ldx)
    Wm = randn(g, 4 * K.VC * C) / C ** 0.5
    T = sent(dev, pts + 8, 4 * K.ROW)
    keep = X.to(dev), Wm.to(dev)
    lib.pcd_train_pass("PREMAP", n_parts=1, n_points=pts, cin=C, ld_x=ldx, x=keep[0], w=keep[1], T=T)
    T = T.cpu()
    ref, S, plain = K.evaluate(K.premap, X, Wm, C)
    check(f"premap C={C} pts={pts}", "premap", {"T": T[:pts]}, ref, S, plain)
    assert bool((T[pts:] == SENT).all()) and bool((T[:pts].view(pts, 4, K.ROW)[:, :, K.V3] == 0).all())


# ------------------------------------------------------------------------------------------------ conv6
@pytest.mark.parametrize("feat", [2, 30, 128])
def test_c6_passes(feat, lib, dev):
    """k_c6 in its three modes and k_c6_dx: 300 points over 3 clouds; ld(G6) = 4, 32, 132; feat = 128 fills the 256 sum slots"""
    P, N = 3, 100
    pts, nb, ld = P * N, 2, K.g6_ld(feat)
    assert ld == {2: 4, 30: 32, 128: 132}[feat]
    g = gen(feat)
    X = [torch.cat([0.3 * randn(g, pts, K.V3), torch.full((pts, 1), 5.0)], 1) for _ in range(3)]       # column 63 is not read
    w6 = torch.cat([randn(g, (feat + 1) * K.V3) / K.V3 ** 0.5, torch.zeros(2 * feat)])
    gamma, beta, rm, rv = torch.rand(feat, generator=g) + 0.5, 0.5 + 0.2 * randn(g, feat), torch.rand(feat, generator=g), torch.rand(feat, generator=g) + 0.1
    dm = randn(g, P, feat * 3)
    Xd, wd_, dmd = [x.to(dev) for x in X], w6.to(dev), dm.to(dev)
    common = dict(n_parts=P, n_points=N, feat=feat, X1=Xd[0], X2=Xd[1], X3=Xd[2], w=wd_)
    # STAT
    part = sent(dev, nb + 1, 2, feat, dtype=F64)
    lib.pcd_train_pass("C6_STAT", partial=part, **common)
    part = part.cpu()
    ref, S, plain = K.evaluate(K.c6_stat, *X, w6, feat)
    check(f"c6 feat={feat} STAT", "c6_stat", {"partial": part[:nb]}, ref, S, plain)
    assert bool((part[nb] == SENT).all())
    d = lambda t: t.double()                                                 # noqa: E731
    f = K.bn_fin_fwd(ref["partial"], float(pts), d(gamma), d(beta), MOM, BN_EPS, d(rm), d(rv))
    rec = K.fin_to_rec(f, d(gamma), d(beta)).float()
    # BWD1
    part = sent(dev, nb + 1, 2, feat, dtype=F64)
    recd = rec.to(dev)
    lib.pcd_train_pass("C6_BWD1", partial=part, rec_a=recd, dm_in=dmd, **common)
    part = part.cpu()
    ref, S, plain, slack, masks, op = K.c6_case(1, *X, w6, feat, N, rec, dm)
    check(f"c6 feat={feat} BWD1", "c6_bwd1", {"partial": part[:nb]}, ref, S, plain, slack, masks, op)
    assert bool((part[nb] == SENT).all())
    fb = K.bn_fin_bwd(ref["partial"], float(pts), torch.zeros(feat, dtype=F64), torch.zeros(feat, dtype=F64))
    rec[K.R_MDY, :feat], rec[K.R_MDYX, :feat] = fb["mdy"].float(), fb["mdyx"].float()
    # BWD2
    G6, Fm = sent(dev, pts * 3 + 16, ld), sent(dev, pts * 3 + 16, K.ROW)
    recd = rec.to(dev)
    lib.pcd_train_pass("C6_BWD2", rec_a=recd, dm_in=dmd, G6=G6, F=Fm, ld_g=ld, **common)
    G6, Fm = G6.cpu(), Fm.cpu()
    ref, S, plain, slack, masks, op = K.c6_case(2, *X, w6, feat, N, rec, dm)
    check(f"c6 feat={feat} BWD2", "c6_bwd2", {"G6": G6[:pts * 3, :feat + 1]}, {"G6": ref["G6"]}, S, plain, slack, masks, op)
    assert torch.equal(Fm[:pts * 3].double(), ref["F"])                       # a move: exact, column 63 zero
    assert bool((G6[:, feat + 1:] == SENT).all()) and bool((G6[pts * 3:] == SENT).all()) and bool((Fm[pts * 3:] == SENT).all())
    # C6_DX on stored rows (pad columns hold the sentinel: they must not be read into the result)
    Gop = torch.cat([randn(g, pts * 3, feat + 1), torch.full((pts * 3, ld - feat - 1), SENT)], 1)
    dXs = [sent(dev, pts * 3 + 16, K.ROW) for _ in range(3)]
    Gd = Gop.to(dev)
    lib.pcd_train_pass("C6_DX", n_parts=P, n_points=N, feat=feat, G6=Gd, ld_g=ld, w=wd_, dX1=dXs[0], dX2=dXs[1], dX3=dXs[2])
    dXs = [t.cpu() for t in dXs]
    ref, S, plain = K.evaluate(K.c6_dx, Gop, w6, feat)
    check(f"c6 feat={feat} DX", "c6_dx", {f"dX{i + 1}": dXs[i][:pts * 3, :K.VC + 1] for i in range(3)}, ref, S, plain)
    for t in dXs:
        assert bool((t[:pts * 3, K.VC] == 0).all()) and bool((t[:, K.VC + 1:] == SENT).all()) and bool((t[pts * 3:] == SENT).all())


# ------------------------------------------------------------------------------------------------ finalisers
def synth_partial(nblk, C, per, seed, same_channel=None):
    """fp64 block partials of ``per`` norms per block and channel: (sum n, sum n^2); one channel with identical norms"""
    g = gen(seed)
    n = torch.rand(nblk, per, C, generator=g, dtype=F64) * 0.9 + 0.1
    if same_channel is not None:
        n[:, :, same_channel] = 0.37
    return torch.stack([n.sum(1), (n * n).sum(1)], 1).contiguous()


@pytest.mark.parametrize("nblk,C,per,with_ss", [(1, 21, 8, True), (2, 2, 8, False), (257, 21, 8, True), (300, 128, 8, False), (1, 2, 2, False), (257, 128, 3, True)])
def test_bn_fin_fwd(nblk, C, per, with_ss, lib, dev):
    """k_bn_fin_fwd on synthetic fp64 partials: the strided loop (nblk > 256), count = 2 (VnInv: count / (count - 1) = 2),
    channel 0 with identical norms (variance <= 0 after rounding, clamped), ss slots with and without a pointer"""
    count = float(nblk * per)
    part = synth_partial(nblk, C, per, nblk + C, same_channel=0)
    g = gen(C)
    gamma, beta, rm, rv = torch.rand(C, generator=g) + 0.5, randn(g, C), torch.rand(C, generator=g), torch.rand(C, generator=g) + 0.1
    rec, run = sent(dev, K.REC, K.CMAX), sent(dev, 2, K.CMAX)
    ss_ld = C + 3
    ss = sent(dev, 2, ss_ld) if with_ss else None
    keep = [t.to(dev) for t in (part, gamma, beta, rm, rv)]
    lib.pcd_train_pass("BN_FIN_FWD", partial=keep[0], nblk=nblk, channels=C, count=count, gamma=keep[1], beta=keep[2], momentum=MOM, eps=BN_EPS,
                       running_mean=keep[3], running_var=keep[4], rec_a=rec, run_out=run, ss=ss, ld_m=ss_ld)
    rec, run = rec.cpu(), run.cpu()
    ref, S, plain = K.evaluate(K.bn_fin_fwd, part, count, gamma, beta, MOM, BN_EPS, rm, rv)
    got = {"mean": rec[K.R_MEAN, :C], "rstd": rec[K.R_RSTD, :C], "run_mean": run[0, :C], "run_var": run[1, :C]}
    if with_ss:
        ss = ss.cpu()
        got.update(scale=ss[0, :C], shift=ss[1, :C])
        assert bool((ss[:, C:] == SENT).all())
    check(f"bn_fin_fwd nblk={nblk} C={C} count={count:g}", "bn_fin_fwd", got, {k: ref[k] for k in got}, S, plain)
    assert torch.equal(rec[K.R_GAMMA, :C], gamma) and torch.equal(rec[K.R_BETA, :C], beta)
    assert bool((rec[:, C:] == SENT).all()) and bool((rec[K.R_MDY:] == SENT).all()) and bool((run[:, C:] == SENT).all())
    assert float(ref["rstd"][0]) > 0.99 / BN_EPS ** 0.5                       # channel 0 really is the clamped one


@pytest.mark.parametrize("nblk,C", [(1, 21), (2, 2), (257, 128), (300, 21)])
def test_bn_fin_bwd(nblk, C, lib, dev):
    g = gen(nblk * C)
    part = torch.randn(nblk, 2, C, generator=g, dtype=F64)
    count = float(nblk * 256 * K.KNN)
    dg0, db0 = randn(g, C), randn(g, C)
    rec, dg, db = sent(dev, K.REC, K.CMAX), dg0.to(dev), db0.to(dev)
    keep = part.to(dev)
    lib.pcd_train_pass("BN_FIN_BWD", partial=keep, nblk=nblk, channels=C, count=count, rec_a=rec, dgamma=dg, dbeta=db)
    rec = rec.cpu()
    ref, S, plain = K.evaluate(K.bn_fin_bwd, part, count, dg0, db0)
    check(f"bn_fin_bwd nblk={nblk} C={C}", "bn_fin_bwd", {"mdy": rec[K.R_MDY, :C], "mdyx": rec[K.R_MDYX, :C], "dgamma": dg.cpu(), "dbeta": db.cpu()}, ref, S, plain)
    assert bool((rec[:K.R_MDY] == SENT).all()) and bool((rec[:, C:] == SENT).all())


# ------------------------------------------------------------------------------------------------ reverse adjacency, gather
def lists_for(P, N, kind, seed):
    if kind == "knn":
        return K.knn_lists(W.make_point_clouds(P, N, seed).reshape(P * N, 3), N)
    return K.perm_lists(P, N, seed) if N == K.KNN else K.hub_lists(P, N, seed)


def run_rev(lib, dev, P, N, idx):
    pts = P * N
    out = [sent(dev, pts + 8, dtype=I32), sent(dev, pts + 8, dtype=I32), sent(dev, pts + 8, dtype=I32), sent(dev, pts * K.KNN + 8, dtype=I32)]
    keep = idx.to(dev)
    lib.pcd_train_pass("REV_ADJ", n_parts=P, n_points=N, idx=keep, cnt=out[0], ptr=out[1], cur=out[2], rev=out[3])
    return [t.cpu() for t in out]


@pytest.mark.parametrize("kind", ["hub", "knn"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N", [20, 255, 257, 300])
def test_reverse_adjacency_exact(N, P, kind, lib, dev):
    """count, scan, fill, sort as one pass against a numpy counting sort, exactly: N around the scan's 256 threads, one and
    three clouds, a hub (cnt = N) and an orphan (cnt = 0) per cloud (N = 20: every list a permutation, cnt = 20 for all)"""
    idx = lists_for(P, N, kind, N + P)
    pts = P * N
    cnt, ptr, cur, rev = run_rev(lib, dev, P, N, idx)
    rc, rp, rr = K.rev_adj(idx.numpy(), N)
    assert np.array_equal(cnt[:pts].numpy(), rc) and np.array_equal(ptr[:pts].numpy(), rp) and np.array_equal(rev[:pts * K.KNN].numpy(), rr)
    assert all(bool((t[n:] == int(SENT)).all()) for t, n in ((cnt, pts), (ptr, pts), (cur, pts), (rev, pts * K.KNN)))
    if kind == "hub" and N > K.KNN:
        assert rc[0] == N and rc[N - 1] == 0


@pytest.mark.parametrize("C", [1, K.VC])
@pytest.mark.parametrize("P,N,kind", [(3, 100, "hub"), (1, 300, "knn"), (2, 20, "hub"), (1, 257, "hub")])
def test_gather(P, N, kind, C, lib, dev):
    """k_gather<1> / <21>: dTc (sums over the reverse lists and the own edges), Xc (a move: exact), dXp added to"""
    idx = lists_for(P, N, kind, N + P + C)
    pts = P * N
    g = gen(pts + C)
    E = randn(g, pts * K.KNN, K.E_LD)
    E[:, K.V3], E[:, K.ROW + K.V3] = 0, 0
    ldx = 3 if C == 1 else K.ROW
    X, Wm = randn(g, pts, ldx), randn(g, 4 * K.VC * C) / C ** 0.5
    dXp0 = randn(g, pts * 3) if C == 1 else randn(g, pts * 3, K.ROW)
    rc, rp, rr = (torch.from_numpy(v) for v in K.rev_adj(idx.numpy(), N))
    dXp = torch.cat([dXp0.reshape(-1), torch.full((64,), SENT)]).to(dev)
    dTc, Xc = sent(dev, pts * 3 + 8, K.DT_LD), sent(dev, pts * 3 + 8, K.XC_LD)
    keep = [t.to(dev) for t in (E, rc, rp, rr, Wm, X)]
    lib.pcd_train_pass("GATHER", n_parts=P, n_points=N, cin=C, ld_x=ldx, E=keep[0], cnt=keep[1], ptr=keep[2], rev=keep[3], w=keep[4], x=keep[5],
                       dXp=dXp, dTc=dTc, Xc=Xc)
    dXp, dTc, Xc = dXp.cpu(), dTc.cpu(), Xc.cpu()
    ref, S, plain = K.evaluate(K.gather, E, rc, rr, Wm, X, C, dXp0.reshape(-1))
    got = {"dTc": dTc[:pts * 3], "dXp": dXp[:dXp0.numel()].view(ref["dXp"].shape)}
    check(f"gather C={C} p{P}_n{N}_{kind}", f"gather{C}", got, {k: ref[k] for k in got}, S, plain)
    assert torch.equal(Xc[:pts * 3, :C].double(), ref["Xc"])
    assert bool((Xc[:, C:] == SENT).all()) and bool((Xc[pts * 3:] == SENT).all()) and bool((dTc[pts * 3:] == SENT).all())
    assert bool((dXp[dXp0.numel():] == SENT).all())
    if C > 1:                                                                # the map's unused columns are left alone
        assert torch.equal(dXp[:dXp0.numel()].view(pts * 3, K.ROW)[:, K.VC:], dXp0[:, K.VC:])
    if kind == "hub" and N > K.KNN:                                          # the orphan's incoming sums are exact zeros
        assert bool((dTc[(N - 1) * 3:(N - 1) * 3 + 3, :2 * K.VC] == 0).all())


@pytest.mark.parametrize("C", [1, K.VC])
def test_premap_wgrad(C, lib, dev):
    g = gen(C)
    dWm, f0, d0 = randn(g, 4 * K.VC * C), randn(g, 2 * K.VC * C), randn(g, 2 * K.VC * C)
    f, d_ = torch.cat([f0, torch.full((8,), SENT)]).to(dev), torch.cat([d0, torch.full((8,), SENT)]).to(dev)
    keep = dWm.to(dev)
    lib.pcd_train_pass("PREMAP_WGRAD", cin=C, dWm=keep, dwf=f, dwd=d_)
    ref, S, plain = K.evaluate(K.premap_wgrad, dWm, C, f0, d0)
    n = 2 * K.VC * C
    check(f"premap_wgrad C={C}", "premap_wgrad", {"dwf": f.cpu()[:n].view(K.VC, 2 * C), "dwd": d_.cpu()[:n].view(K.VC, 2 * C)}, ref, S, plain)
    assert bool((f.cpu()[n:] == SENT).all()) and bool((d_.cpu()[n:] == SENT).all())


# ------------------------------------------------------------------------------------------------ head, VnInv
@pytest.mark.parametrize("feat", [2, 128])
@pytest.mark.parametrize("inv", [0, 1])
def test_head_bwd_and_lin0_grad(inv, feat, lib, dev):
    P = 5
    g = gen(10 * feat + inv)
    ldg = (2 * feat if inv else 6 * feat) + 5                                # a row stride wider than the row
    G = randn(g, P, ldg)
    lin0 = torch.cat([randn(g, 2 * feat * 3), randn(g, 2 * feat)])
    dm = sent(dev, P * feat * 3 + 8)
    keep = G.to(dev), lin0.to(dev)
    lib.pcd_train_pass("HEAD_BWD", n_parts=P, feat=feat, inv=inv, ld_g=ldg, grad_out=keep[0], w=keep[1], dm=dm)
    dm = dm.cpu()
    ref, S, plain = K.evaluate(K.head_bwd, G, inv, feat, lin0)
    check(f"head_bwd inv={inv} feat={feat}", "head_bwd", {"dm": dm[:P * feat * 3].view(P, feat * 3)}, ref, S, plain)
    assert bool((dm[P * feat * 3:] == SENT).all())
    if inv:
        ldm = 6 * feat + 2
        M = randn(g, P, ldm)
        W0, b0 = randn(g, 2 * feat * 3), randn(g, 2 * feat)
        dW, db = torch.cat([W0, torch.full((8,), SENT)]).to(dev), torch.cat([b0, torch.full((8,), SENT)]).to(dev)
        Md = M.to(dev)
        lib.pcd_train_pass("LIN0_GRAD", n_parts=P, feat=feat, ld_g=ldg, ld_x=ldm, grad_out=keep[0], x=Md, dwf=dW, dwd=db)
        dW, db = dW.cpu(), db.cpu()
        ref, S, plain = K.evaluate(K.lin0_grad, G, M, feat, W0, b0)
        check(f"lin0_grad feat={feat}", "lin0_grad", {"dW0": dW[:6 * feat].view(2 * feat, 3), "db0": db[:2 * feat]}, ref, S, plain)
        assert bool((dW[6 * feat:] == SENT).all()) and bool((db[2 * feat:] == SENT).all())


@pytest.mark.parametrize("P", [2, 300])
def test_vn_inv_passes(P, lib, dev):
    """k_vn_lin, k_vn_stat, k_bn_fin_fwd at count = P, k_vn_apply, as VnInv.vn1 runs them (feat = 8: 16 -> 8 channels)"""
    feat, cin, cout = 8, 16, 8
    g = gen(P)
    ldx = 6 * feat
    X, Wf, Wd = randn(g, P, ldx), randn(g, cout, cin) / 4, randn(g, cout, cin) / 4
    vP, vD, vY = (sent(dev, P * cout * 3 + 8) for _ in range(3))
    keep = [t.to(dev) for t in (X, Wf, Wd)]
    lib.pcd_train_pass("VN_LIN", n_parts=P, vn_cin=cin, channels=cout, ld_x=ldx, x=keep[0], w=keep[1], w2=keep[2], vP=vP, vD=vD)
    n = P * cout * 3
    ref, S, plain = K.evaluate(K.vn_lin, X, Wf, Wd, cin)
    check(f"vn_lin P={P}", "vn_lin", {"vP": vP.cpu()[:n].view(P, cout, 3), "vD": vD.cpu()[:n].view(P, cout, 3)}, ref, S, plain)
    assert bool((vP.cpu()[n:] == SENT).all()) and bool((vD.cpu()[n:] == SENT).all())
    sP, sD = vP.cpu()[:n].view(P, cout, 3).clone(), vD.cpu()[:n].view(P, cout, 3).clone()       # stored operands of the next passes
    part = sent(dev, 2, 2, cout, dtype=F64)
    lib.pcd_train_pass("VN_STAT", n_parts=P, channels=cout, vP=vP, partial=part)
    part = part.cpu()
    ref, S, plain = K.evaluate(K.vn_stat, sP)
    check(f"vn_stat P={P}", "vn_stat", {"partial": part[:1]}, ref, S, plain)
    assert bool((part[1] == SENT).all())
    gamma, beta, rm, rv = torch.rand(cout, generator=g) + 0.5, randn(g, cout), torch.rand(cout, generator=g), torch.rand(cout, generator=g) + 0.1
    rec, run = sent(dev, K.REC, K.CMAX), sent(dev, 2, K.CMAX)
    keep2 = [t.to(dev) for t in (part[:1].contiguous(), gamma, beta, rm, rv)]
    lib.pcd_train_pass("BN_FIN_FWD", partial=keep2[0], nblk=1, channels=cout, count=float(P), gamma=keep2[1], beta=keep2[2], momentum=MOM, eps=BN_EPS,
                       running_mean=keep2[3], running_var=keep2[4], rec_a=rec, run_out=run)
    ref, S, plain = K.evaluate(K.bn_fin_fwd, part[:1], float(P), gamma, beta, MOM, BN_EPS, rm, rv)
    recc, runc = rec.cpu(), run.cpu()
    got = {"mean": recc[K.R_MEAN, :cout], "rstd": recc[K.R_RSTD, :cout], "run_mean": runc[0, :cout], "run_var": runc[1, :cout]}
    check(f"vn fin P={P}", "bn_fin_fwd", got, {k: ref[k] for k in got}, S, plain)
    lib.pcd_train_pass("VN_APPLY", n_parts=P, channels=cout, vP=vP, vD=vD, rec_a=rec, vY=vY)
    ref, S, plain = K.evaluate(K.vn_apply, sP, sD, recc)
    check(f"vn_apply P={P}", "vn_apply", {"vY": vY.cpu()[:n].view(P, cout, 3)}, ref, S, plain)
    assert bool((vY.cpu()[n:] == SENT).all())


# ------------------------------------------------------------------------------------------------ da_gemm_tn_f32
def run_gemm(lib, dev, A, a_off, n, lda, B, k, ldb, C0):
    """C0 += A[:, a_off:a_off + n]^T B[:, :k] through da_gemm_tn_f32 on device copies (A, B with their full row strides)"""
    L = lib.lib()
    M = A.shape[0]
    Ad, Bd, Cd = A.to(dev), B.to(dev), C0.to(dev).clone()
    scratch = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    import ctypes
    lib.check(L.da_gemm_tn_f32(M, n, k, ctypes.c_void_p(Ad.data_ptr() + 4 * a_off), lda, lib.ptr(Bd), ldb, lib.ptr(Cd), k, lib.ptr(scratch),
                               lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    return Cd.cpu()


GEMM_SHAPES = ([("Gb.Hb dd", 21, 21, K.GB_LD, K.H_LD, 21), ("dTc.Xc C=1", 84, 1, K.DT_LD, K.XC_LD, 0)]
               + [(f"G6.F feat={f}", f, 63, K.g6_ld(f), K.ROW, 0) for f in (2, 30, 128)]
               + [(f"G6.F dir feat={f}", 1, 63, K.g6_ld(f), K.ROW, f) for f in (2, 30, 128)])


@pytest.mark.parametrize("M", [120, 6000])
@pytest.mark.parametrize("tag,n,k,lda,ldb,a_off", GEMM_SHAPES, ids=[s[0].replace(" ", "_") for s in GEMM_SHAPES])
def test_gemm_tn_at_this_paths_shapes(tag, n, k, lda, ldb, a_off, M, lib, dev):
    """da_gemm_tn_f32 at the operand shapes of da_pcd_train_backward: A offset by 21 floats in rows of 44 (the unaligned
    scalar-load path), K = 1, rows of ld(G6), A offset by feat; one split (M = 120) and several (M = 6000); C pre-filled"""
    g = gen(M + n + k + a_off)
    A, B, C0 = randn(g, M, lda), randn(g, M, ldb), randn(g, n, k)
    got = run_gemm(lib, dev, A, a_off, n, lda, B, k, ldb, C0)
    ref, S, plain = K.evaluate(K.gemm_tn, A[:, a_off:a_off + n], B[:, :k], C0)
    check(f"gemm_tn {tag} M={M}", "gemm_tn", {"C": got}, ref, S, plain)


# ------------------------------------------------------------------------------------------------ a stage, pass by pass
def test_stage_composition_on_the_gpu(lib, dev):
    """A two-layer stage (conv1 + conv2 on 3 clouds of 100 points, lists given) pass by pass through the entries: premap ->
    STAT_A -> fin -> STAT_B -> fin, then BWD1 -> fin -> BWD2 + the two weight GEMMs -> fin -> BWD3 -> reverse adjacency ->
    gather + the premap GEMM -> premap_wgrad, every operand of a pass being what the previous HIP pass left.  dx and every
    gradient must meet the chain of the fp64 contracts under the rule, with S the FINAL pass's own condition term on the
    chain's operands and e_acc the error of the whole chain evaluated in fp32 on the CPU (it includes what the earlier passes'
    rounding does to the later ones); open decisions give the flipped-chain slack."""
    P, N, C = 3, 100, 1
    o = stage(P, N, "knn")
    pts, ne, nb = P * N, P * N * K.KNN, 2
    g = gen(5)
    G = randn(g, pts, K.VC, 3)
    ops = dict(X=o["X"], C=C, N=N, idx=o["idx"], Wm=o["Wm"], bn_a=o["bn_a"], wb=o["wb"], bn_b=o["bn_b"], G=G)
    ref, S, op = K.stage_chain(dt=F64, **ops)
    plain, _, _ = K.stage_chain(dt=F32, **ops)
    flipped, _, _ = K.stage_chain(dt=F64, flip=True, **ops)
    op.assert_cap("stage composition")
    # ---- the HIP chain
    d = lambda t: t.to(dev)                                                  # noqa: E731
    X, idx, Wm, wb = d(o["X"]), d(o["idx"]), d(o["Wm"]), d(o["wb"])
    dX = d(K.to_cmajor(G).reshape(-1).contiguous())
    T = torch.zeros(pts, 4 * K.ROW, device=dev)
    part = torch.zeros(nb, 2, K.VC, dtype=F64, device=dev)
    recA, recB = torch.zeros(K.REC, K.CMAX, device=dev), torch.zeros(K.REC, K.CMAX, device=dev)
    run = torch.zeros(2, K.CMAX, device=dev)
    count = float(ne)
    common = dict(n_parts=P, n_points=N, has_b=1, T=T, idx=idx, rec_a=recA, rec_b=recB, w=wb, dX_in=dX, partial=part)
    grads = {k: torch.zeros(K.VC, device=dev) for k in ("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b")}
    lib.pcd_train_pass("PREMAP", n_parts=P, n_points=N, cin=C, ld_x=3, x=X, w=Wm, T=T)

    def fin(rec, bn):
        keep = [d(bn[k]) for k in ("gamma", "beta", "rm", "rv")]
        lib.pcd_train_pass("BN_FIN_FWD", partial=part, nblk=nb, channels=K.VC, count=count, gamma=keep[0], beta=keep[1], momentum=MOM, eps=BN_EPS,
                           running_mean=keep[2], running_var=keep[3], rec_a=rec, run_out=run)
        torch.cuda.synchronize()

    lib.pcd_train_pass("EDGE_STAT_A", **common)
    fin(recA, o["bn_a"])
    lib.pcd_train_pass("EDGE_STAT_B", **common)
    fin(recB, o["bn_b"])
    lib.pcd_train_pass("EDGE_BWD1", **common)
    lib.pcd_train_pass("BN_FIN_BWD", partial=part, nblk=nb, channels=K.VC, count=count, rec_a=recB, dgamma=grads["dgamma_b"], dbeta=grads["dbeta_b"])
    Gb, Hb, E = torch.zeros(ne * 3, K.GB_LD, device=dev), torch.zeros(ne * 3, K.H_LD, device=dev), torch.zeros(ne, K.E_LD, device=dev)
    lib.pcd_train_pass("EDGE_BWD2", Gb=Gb, Hb=Hb, **common)
    got = {}
    z = torch.zeros(K.VC, K.VC)
    got["dwf_b"] = run_gemm(lib, dev, Gb, 0, K.VC, K.GB_LD, Hb, K.VC, K.H_LD, z)
    got["dwd_b"] = run_gemm(lib, dev, Gb, K.VC, K.VC, K.GB_LD, Hb, K.VC, K.H_LD, z)
    lib.pcd_train_pass("BN_FIN_BWD", partial=part, nblk=nb, channels=K.VC, count=count, rec_a=recA, dgamma=grads["dgamma_a"], dbeta=grads["dbeta_a"])
    lib.pcd_train_pass("EDGE_BWD3", E=E, **common)
    cnt, ptr, cur = (torch.zeros(pts, dtype=I32, device=dev) for _ in range(3))
    rev = torch.zeros(ne, dtype=I32, device=dev)
    lib.pcd_train_pass("REV_ADJ", n_parts=P, n_points=N, idx=idx, cnt=cnt, ptr=ptr, cur=cur, rev=rev)
    dXp, dTc, Xc = torch.zeros(pts * 3, device=dev), torch.zeros(pts * 3, K.DT_LD, device=dev), torch.zeros(pts * 3, K.XC_LD, device=dev)
    lib.pcd_train_pass("GATHER", n_parts=P, n_points=N, cin=C, ld_x=3, E=E, cnt=cnt, ptr=ptr, rev=rev, w=Wm, x=X, dXp=dXp, dTc=dTc, Xc=Xc)
    dWm = run_gemm(lib, dev, dTc, 0, 4 * K.VC, K.DT_LD, Xc, C, K.XC_LD, torch.zeros(4 * K.VC, C))
    dwf, dwd = torch.zeros(K.VC * 2 * C, device=dev), torch.zeros(K.VC * 2 * C, device=dev)
    dWmd = dWm.to(dev)
    lib.pcd_train_pass("PREMAP_WGRAD", cin=C, dWm=dWmd, dwf=dwf, dwd=dwd)
    torch.cuda.synchronize()
    got.update(dXp=dXp.cpu().view(pts, 3), dwf_a=dwf.cpu().view(K.VC, 2 * C), dwd_a=dwd.cpu().view(K.VC, 2 * C), **{k: v.cpu() for k, v in grads.items()})
    keys = sorted(got)
    slack = {k: (flipped[k] - ref[k]).abs().reshape(got[k].shape) for k in keys} if op.n_open else None
    sel = lambda dct: {k: dct[k].reshape(got[k].shape) for k in keys}        # noqa: E731
    check("stage conv1-conv2 p3_n100", "stage", got, sel(ref), sel(S), sel(plain), slack, None, op)


def test_zz_print_ratios():
    """the worst e(HIP) / e_acc(plain) of every pass over the cases above (the table of DESIGN.md 3f); FACTOR must hold them"""
    for k in sorted(RATIOS):
        print(f"[pcd-kernels] worst ratio {k}: {RATIOS[k]:.2f}")
    assert all(v <= 16.0 or k in K.FACTOR for k, v in RATIOS.items())
