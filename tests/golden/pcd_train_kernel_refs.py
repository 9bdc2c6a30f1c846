"""fp64 contracts of the passes of the 3D piece encoder's training path (include/diffassemble_hip.h, "Passes of the 3D
encoder's training path", da_pcd_train_pass) under the rule of tests/golden/encoder_kernel_refs.py (``evaluate``, ``e_acc``,
``judge`` are that module's: the rule is not restated here).  Used by tests/test_pcd_train_kernel_refs.py (host: the chained
contracts against torch autograd of tests/golden/pcd_train_torch.py, the rule's sensitivity) and
tests/test_gpu_pcd_train_kernels.py (the HIP kernels).

Every contract is a plain torch function of the STORED operands in the passes' own layouts (premap rows [A | Ad | U | Ud],
stat records [6][256], component-major gradient maps, ...), written from the maths of vnn/vn_layers.py:50-91,133-154 as
restated in pcd_train_torch.torch_layer: with n = |p| + 1e-6, xhat = (n - mean) rstd, y = gamma xhat + beta, q = p y / n,

    out = q - [q.d < 0] 0.8 (q.d) / (|d|^2 + 1e-6) d

and its derivative.  It runs in the dtype of its operands (ref: fp64, plain: fp32 on the CPU) and returns, with
``cond=True``, the condition term S of every output.

Condition terms.  Linear accumulations (the premap, sums over 20 edges, block sums, the gather, the weight-gradient
operands): the same expression on absolute values.  The vector activation and its backward subtract by construction; there
S is the sum of the absolute values of the TERMS of each expression, built from the S of its inputs: every intermediate
is a ``V`` (value, S) and S follows the operations to first order -- S(a + b) = S_a + S_b, S(a b) = S_a |b| + |a| S_b,
S(a / b) = S_a / |b| + |a / b| S_b / |b|, S(|p|) = sum |p_k| S_k / |p|; a stored operand or a constant enters with
S = |x|.  (Multiplying the factors' S instead, S_a S_b, compounds the two layers' cancellation ratios and reached 1e16
times the value on a conv1-conv2 stage: a bound that rejects nothing.)  1 / sqrt(var + eps) takes
S = rstd + rstd / (2 (var + eps)) S_var (the same propagation of the variance's S = E n^2 + mean^2).

Leaky-ReLU decisions.  Every backward pass decides q.d < 0, and the gradient jumps there.  The contracts return per decision
the margin |cos(q, d)|; decisions with margin < TAU are OPEN (``Open``).  A per-edge output that depends on an open decision
is left out (mask), a summed output gets as extra slack the sum over its open decisions of |contribution with the decision
flipped - contribution| (the contract is evaluated a second time in fp64 with the open decisions flipped).  A vector that
is exactly zero (a point at the origin with its self edge) has q.d = 0 in any arithmetic: not open.  ``OPEN_CAP``: no case
may have more than 1e-3 of its decisions open; asserted from the reference alone.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

import encoder_kernel_refs as R
from encoder_kernel_refs import F32, F64, evaluate, e_acc, judge  # noqa: F401  (the rule)

KNN, VC, ROW, V3 = 20, 21, 64, 63
CMAX, REC = 256, 6
R_MEAN, R_RSTD, R_GAMMA, R_BETA, R_MDY, R_MDYX = range(6)
GB_LD, H_LD, E_LD, DT_LD, XC_LD = 44, 24, 128, 84, 24
EPS = 1e-6
TAU, OPEN_CAP = 1e-4, 1e-3
# FACTOR of the rule per pass (default: encoder_kernel_refs.FACTOR = 16).  A wider entry is at most twice the measured
# e(HIP) / e_acc(plain) and needs the measured figures and the reason in the docstring of the test that uses it.
FACTOR = {}


R.FACTOR.update({"pcd_" + k: v for k, v in FACTOR.items()})


def g6_ld(feat):
    return (feat + 4) & ~3


def judge_pass(got, ref, S, plain, kernel="default", slack=None, mask=None):
    """encoder_kernel_refs.judge (this module's FACTOR entries are registered in its table as "pcd_<pass>"), with the
    open-decision slack of a summed output added to the bound and the elements of ``mask`` (per-edge outputs of open
    decisions) left out.  -> judge's dict + ``left_out``."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if mask is not None and bool(mask.any()):
        keep = ~mask
        got, ref, S, plain = got[keep], ref[keep], S[keep], plain[keep]
        slack = None if slack is None else slack[keep]
    if slack is not None:
        d = got - ref                                    # an absolute allowance on top of the rule's bound
        got = ref + torch.sign(d) * (d.abs() - slack).clamp_min(0)
    j = judge(got, ref, S, plain, F32, kernel="pcd_" + kernel)
    j["left_out"] = 0 if mask is None else int(mask.sum())
    return j


# ------------------------------------------------------------------------------------------------ layouts
def segs(T):
    """premap rows [pts][256] -> [pts, 4, 21, 3] (A, Ad, U, Ud)"""
    return T.view(-1, 4, ROW)[:, :, :V3].reshape(-1, 4, VC, 3)


def glob(idx, N):
    """cloud-local lists [pts][20] -> global point indices"""
    pts = idx.shape[0]
    return (torch.arange(pts) // N * N)[:, None] + idx.long()


def rec_bn(rec, C):
    return tuple(rec[r, :C] for r in (R_MEAN, R_RSTD, R_GAMMA, R_BETA))


def wb_maps(wb):
    """conv_b blob -> map_to_feat, map_to_dir [21][21] (rows zero-padded to 22 in the blob)"""
    return wb[:VC * 22].view(VC, 22)[:, :VC], wb[VC * 22:2 * VC * 22].view(VC, 22)[:, :VC]


def w6_maps(w6, feat):
    return w6[:feat * V3].view(feat, V3), w6[feat * V3:feat * V3 + V3].view(1, V3)


def cmajor(dX):
    """component-major gradient map [pts][3][64] -> [pts, 21, 3]"""
    return dX.view(-1, 3, ROW)[:, :, :VC].transpose(1, 2)


def to_cmajor(v, width=ROW):
    """[pts, C, 3] -> rows (point, k) [pts * 3, width], zero-padded"""
    r = v.transpose(1, 2).reshape(-1, v.shape[1])
    return F.pad(r, (0, width - v.shape[1]))


def _blocks(v):
    """v [pts, K, C] -> [nblk, C]: sums over a block's 256 points and K; contiguous last dimension (torch adds pairwise there,
    see encoder_kernel_refs._psum)"""
    pts, K, C = v.shape
    nb = (pts + 255) // 256
    v = F.pad(v, (0, 0, 0, 0, 0, nb * 256 - pts))
    return v.reshape(nb, 256 * K, C).transpose(1, 2).contiguous().sum(-1)


# ------------------------------------------------------------------------------------------------ values with their S
class V:
    """a value and its condition term, propagated to first order: S(a + b) = S_a + S_b, S(a b) = S_a |b| + |a| S_b,
    S(a / b) = S_a / |b| + |a / b| S_b / |b|.  A stored operand (a tensor) or a constant enters with S = |x|."""
    __slots__ = ("v", "S")

    def __init__(self, v, S=None):
        self.v, self.S = v, (v.abs() if S is None else S)

    @staticmethod
    def _vs(o):
        if isinstance(o, V):
            return o.v, o.S
        return (o, o.abs()) if torch.is_tensor(o) else (o, abs(o))

    def __add__(self, o):
        v, S = V._vs(o)
        return V(self.v + v, self.S + S)

    def __sub__(self, o):
        v, S = V._vs(o)
        return V(self.v - v, self.S + S)

    def __neg__(self):
        return V(-self.v, self.S)

    def __mul__(self, o):
        v, S = V._vs(o)
        av = v.abs() if torch.is_tensor(v) else abs(v)
        return V(self.v * v, self.S * av + self.v.abs() * S)

    def __truediv__(self, o):
        v, S = V._vs(o)
        av = v.abs() if torch.is_tensor(v) else abs(v)
        r = self.v / v
        return V(r, self.S / av + r.abs() * S / av)

    def sum(self, dim):
        return V(self.v.sum(dim), self.S.sum(dim))

    def un(self):
        return V(self.v[..., None], self.S[..., None])

    def where(self, m):
        z = torch.zeros_like(self.v)
        return V(torch.where(m, self.v, z), torch.where(m, self.S, z))

    def expand_as(self, o):
        return V(self.v.expand_as(o.v), self.S.expand_as(o.v))

    def map(self, f):
        return V(f(self.v), f(self.S))


def norm3(p):
    """|p| over the last dimension: S = sum |p_k| S_k / |p| (a zero vector: the norm of the S)"""
    n = (p.v * p.v).sum(-1).sqrt()
    ok = n > 0
    S = torch.where(ok, (p.v.abs() * p.S).sum(-1) / torch.where(ok, n, torch.ones_like(n)), (p.S * p.S).sum(-1).sqrt())
    return V(n, S)


def lin(w, x):
    """channel map w [o][c] over x [..., c, 3]; the stored weights are exact"""
    return V(torch.einsum("oc,...ck->...ok", w, x.v), torch.einsum("oc,...ck->...ok", w.abs(), x.S))


def lin_t(w, x):
    return V(torch.einsum("oc,...ok->...ck", w, x.v), torch.einsum("oc,...ok->...ck", w.abs(), x.S))


# ------------------------------------------------------------------------------------------------ the vector activation
def _act(p, d, bn, flip=None):
    """VNBatchNorm on the norm + the vector leaky ReLU.  p, d: V [..., C, 3]; bn = (mean, rstd, gamma, beta) [C]."""
    mu, rstd, gam, bet = bn
    n = norm3(p) + EPS
    xh = (n - mu) * rstd
    y = xh * gam + bet
    s = y / n
    q = p * s.un()
    dot, dsq = (q * d).sum(-1), (d * d).sum(-1) + EPS
    zero = ((p.v == 0).all(-1) | (d.v == 0).all(-1))
    margin = torch.where(zero, torch.full_like(dot.v, math.inf),
                         dot.v.abs() / ((q.v * q.v).sum(-1).sqrt() * (d.v * d.v).sum(-1).sqrt() + 1e-300))
    neg = dot.v < 0
    if flip is not None:
        neg = neg ^ flip
    c = (dot / dsq * 0.8).where(neg)
    return NS(p=p, d=d, n=n, xh=xh, y=y, s=s, q=q, dot=dot, dsq=dsq, neg=neg, out=q - d * c.un(), margin=margin, bn=bn)


def _act_local(A, g, defect=()):
    """backward of _act down to the BatchNorm output: with k = 0.8 (g.d) / |d|^2 and c = 0.8 (q.d) / |d|^2 on the projected
    branch, dq = g - k d, dd = -c g - k q + 2 k (q.d) / |d|^2 d; dy = dq.p / n"""
    k8 = 0.79 if "c079" in defect else 0.8
    kk = ((g * A.d).sum(-1) / A.dsq * k8).where(A.neg)
    cb = (A.dot / A.dsq * k8).where(A.neg)
    dq = g - A.d * kk.un()
    dd = -(g * cb.un()) - A.q * kk.un()
    if "no_ddsq2" not in defect:
        dd = dd + A.d * (kk * A.dot / A.dsq * 2.0).un()
    return NS(dq=dq, dd=dd, dy=(dq * A.p).sum(-1) / A.n)


def _act_finish(A, L, mdy, mdyx, defect=()):
    """dp from the local part and the channel's batch means of dy, dy xhat: the norm receives
    dn = gamma rstd (dy - mean dy - xhat mean(dy xhat)) - dy y / n, and dp = (y / n) dq + dn p / |p|"""
    mu, rstd, gam, bet = A.bn
    dn = (L.dy - mdy - A.xh * mdyx) * (gam * rstd)
    if "no_dyy" not in defect:
        dn = dn - L.dy * A.y / A.n
    pn = A.n.v - EPS
    ok = pn > 0
    f = (dn / V(torch.where(ok, pn, torch.ones_like(pn)), A.n.S)).where(ok)
    return L.dq * A.s.un() + A.p * f.un()


class Open:
    """the open decisions of a case, collected from the fp64 evaluation"""

    def __init__(self, *masks):
        self.total = sum(m.numel() for m in masks)
        self.n_open = sum(int(m.sum()) for m in masks)

    @property
    def share(self):
        return self.n_open / max(self.total, 1)

    def assert_cap(self, tag=""):
        assert self.share <= OPEN_CAP, f"{tag}: {self.n_open} of {self.total} decisions open (cap {OPEN_CAP})"


def _ret(out, S, cond):
    return (out, S) if cond else out


def _split(d):
    """dict name -> V  ->  (values, S)"""
    return {k: x.v for k, x in d.items()}, {k: x.S for k, x in d.items()}


# ------------------------------------------------------------------------------------------------ premap
def premap(X, Wm, C=1, cond=False):
    """PREMAP: T[p][m] = Wm[m] x_p for the four maps, 21 x 3 values + one zero per 64-float segment.  X [pts][ldx] rows."""
    def run(X, Wm):
        x = X[:, :3 * C].reshape(-1, C, 3)
        t = torch.einsum("moc,pck->pmok", Wm.view(4, VC, C), x).reshape(-1, 4, V3)
        return F.pad(t, (0, 1)).reshape(-1, 4 * ROW)
    return _ret({"T": run(X, Wm)}, {"T": run(X.abs(), Wm.abs())}, cond)


# ------------------------------------------------------------------------------------------------ the edge passes
def edge_inputs(T, idx, N):
    """first-layer inputs of every edge: p = A_j + U_i, d = Ad_j + Ud_i, V [pts, 20, 21, 3]"""
    s, j = segs(T), glob(idx, N)
    return V(s[j, 0]) + V(s[:, None, 2]), V(s[j, 1]) + V(s[:, None, 3])


def _sums(u, w):
    """the two block sums of a pass -> V [nblk][2][C]"""
    return V(torch.stack([_blocks(u.v), _blocks(w.v)], 1), torch.stack([_blocks(u.S), _blocks(w.S)], 1))


def _norm_sums(p, zero_last=False):
    n = norm3(p) + EPS
    if zero_last:
        n = V(n.v.clone(), n.S)
        n.v[..., -1] = 0
    return _sums(n, n * n)


def edge_stat_a(T, idx, N, cond=False):
    """EDGE_STAT_A: per block of 256 points the sums over its edges of n = |A_j + U_i| + eps and n^2 -> [nblk][2][21]"""
    p, _ = edge_inputs(T, idx, N)
    out, S = _split({"partial": _norm_sums(p)})
    return _ret(out, S, cond)


def edge_stat_b(T, idx, N, recA, wb, cond=False, zero_last=False):
    """EDGE_STAT_B: the same sums for layer b's feature vector Wf_b h, h = act_a(A_j + U_i).  ``zero_last`` plants a defect."""
    p, d = edge_inputs(T, idx, N)
    A = _act(p, d, rec_bn(recA, VC))
    out, S = _split({"partial": _norm_sums(lin(wb_maps(wb)[0], A.out), zero_last)})
    return _ret(out, S, cond)


def edge_pool(T, idx, N, recA, recB=None, wb=None, cond=False):
    """the forward's pooling pass (the eval kernel on the batch statistics): X[p] = mean over the 20 edges of the stage's
    output -> rows [pts][64], 63 used"""
    p, d = edge_inputs(T, idx, N)
    A = _act(p, d, rec_bn(recA, VC))
    if wb is not None:
        wf, wd = wb_maps(wb)
        A = _act(lin(wf, A.out), lin(wd, A.out), rec_bn(recB, VC))
    out, S = _split({"X": A.out.map(lambda v: F.pad(v.mean(1).reshape(-1, V3), (0, 1)))})
    return _ret(out, S, cond)


def edge_bwd(mode, T, idx, N, recA, recB, wb, dX, cond=False, flip=False, defect=()):
    """EDGE_BWD1 / 2 / 3 (mode 1, 2, 3).  dX: gradient of the pooled output, component-major; every edge receives g = dX / 20.
    recA / recB: the layers' records (recB, wb None: a single-layer stage).  ``flip``: evaluate with the open decisions
    flipped (for the slack of summed outputs).
      1: partial = block sums of dy, dy xhat of the LAST layer;
      2: Gb = [dp_b | dd_b] rows (edge, k), Hb = h rows, partial = block sums of layer a;
      3: E = [dp_a (63) | 0 | dd_a (63) | 0] per edge.
    Key "_open": the open decisions (layer a, layer b) [pts, 20, 21], not a kernel output."""
    has_b = wb is not None
    p, d = edge_inputs(T, idx, N)
    g = V(cmajor(dX)[:, None]) / float(KNN)
    A = _act(p, d, rec_bn(recA, VC))
    oa = A.margin < TAU
    if flip:
        A = _act(p, d, rec_bn(recA, VC), flip=oa)
    res = {}
    ob = torch.zeros_like(oa)
    g = g.expand_as(p)
    if has_b:
        wf, wd = wb_maps(wb)
        pb, db = lin(wf, A.out), lin(wd, A.out)
        B = _act(pb, db, rec_bn(recB, VC))
        ob = B.margin < TAU
        if flip:
            B = _act(pb, db, rec_bn(recB, VC), flip=ob)
        LB = _act_local(B, g, defect)
        if mode == 1:
            res["partial"] = _sums(LB.dy, LB.dy * B.xh)
        else:
            dpb = _act_finish(B, LB, recB[R_MDY, :VC], recB[R_MDYX, :VC], defect)
            if mode == 2:
                res["Gb"] = V(torch.cat([dpb.v, LB.dd.v], -2), torch.cat([dpb.S, LB.dd.S], -2)).map(lambda v: v.transpose(-1, -2).reshape(-1, 2 * VC))
                res["Hb"] = A.out.map(lambda v: v.transpose(-1, -2).reshape(-1, VC))
            g = lin_t(wf, dpb) + lin_t(wd, LB.dd)
    if not has_b or mode >= 2:
        LA = _act_local(A, g, defect)
        if mode < 3:
            res["partial"] = _sums(LA.dy, LA.dy * A.xh)
        else:
            dpa = _act_finish(A, LA, recA[R_MDY, :VC], recA[R_MDYX, :VC], defect)
            res["E"] = V(torch.stack([dpa.v, LA.dd.v], 2), torch.stack([dpa.S, LA.dd.S], 2)).map(lambda v: F.pad(v.reshape(-1, 2, V3), (0, 1)).reshape(-1, E_LD))
    out, S = _split(res)
    out["_open"] = S["_open"] = (oa, ob)
    return _ret(out, S, cond)


def edge_open_masks(mode, oa, ob, has_b):
    """per-edge outputs that depend on an open decision -> boolean masks in the outputs' layouts.  Gb: the two columns of an
    open layer-b decision; E: the whole edge when a layer-b decision of it is open (dh jumps), else the channel's entries."""
    m = {}
    if mode == 2:
        col = ob[..., None, :].expand(*ob.shape[:2], 3, VC).reshape(-1, VC)
        m["Gb"] = torch.cat([col, col], 1)
    if mode == 3:
        ch = (oa | ob.any(-1, keepdim=True)) if has_b else oa
        e = F.pad(ch[..., None].expand(*ch.shape, 3).reshape(-1, V3), (0, 1))
        m["E"] = torch.cat([e, e], 1)
    return m


def edge_case(mode, T, idx, N, recA, recB, wb, dX):
    """evaluate one backward edge pass for a test: -> (ref, S, plain, slack, masks, Open); asserts the open cap."""
    ops = (T, idx, N, recA, recB, wb, dX)
    ref, S, plain = evaluate(lambda *o, cond=False: edge_bwd(mode, *o, cond=cond), *ops)
    oa, ob = ref.pop("_open")
    S.pop("_open"), plain.pop("_open")
    has_b = wb is not None
    op = Open(oa, ob) if has_b else Open(oa)
    op.assert_cap(f"edge pass {mode}")
    slack = {}
    if op.n_open and "partial" in ref:
        # per block and channel |sums with the open decisions flipped - sums| (>= the issue's sum of per-decision differences
        # only while a block holds one open decision per channel; the cases' seeds are chosen to have none or few)
        fl = edge_bwd(mode, *R._cast(ops, F64), flip=True)
        slack["partial"] = (fl["partial"] - ref["partial"]).abs()
    return ref, S, plain, slack, edge_open_masks(mode, oa, ob, has_b), op


# ------------------------------------------------------------------------------------------------ conv6
def _c6(X1, X2, X3, w6, feat):
    f = V(torch.cat([X[:, :V3].reshape(-1, VC, 3) for X in (X1, X2, X3)], 1))                # [pts, 63, 3]
    wf, wd = w6_maps(w6, feat)
    return f, lin(wf, f), lin(wd, f)


def c6_stat(X1, X2, X3, w6, feat, cond=False):
    """C6_STAT: block sums over the points of n = |W6 cat(x1, x2, x3)| + eps and n^2 -> [nblk][2][feat]"""
    _, p, _ = _c6(X1, X2, X3, w6, feat)
    out, S = _split({"partial": _norm_sums(p.map(lambda v: v[:, None]))})
    return _ret(out, S, cond)


def c6_bwd(mode, X1, X2, X3, w6, feat, N, rec, dm, cond=False, flip=False, defect=()):
    """C6_BWD1 (mode 1): block sums of dy, dy xhat; C6_BWD2 (mode 2): G6 rows (point, k) = [dp6 (feat) | sum_o dd6],
    F rows = cat(x1, x2, x3) component-major.  dm [P][feat][3]: gradient of the mean over the cloud's N points."""
    f, p, d = _c6(X1, X2, X3, w6, feat)
    d = d.expand_as(p)
    pts = p.v.shape[0]
    g = V(dm.view(-1, feat, 3)[torch.arange(pts) // N]) / float(N)
    bn = rec_bn(rec, feat)
    A = _act(p, d, bn)
    o6 = A.margin < TAU
    if flip:
        A = _act(p, d, bn, flip=o6)
    L = _act_local(A, g, defect)
    un = lambda x: x.map(lambda v: v[:, None])                             # noqa: E731
    if mode == 1:
        res = {"partial": _sums(un(L.dy), un(L.dy * A.xh))}
    else:
        dp = _act_finish(A, L, rec[R_MDY, :feat], rec[R_MDYX, :feat], defect)
        dd6 = L.dd.sum(1)
        res = {"G6": V(torch.cat([dp.v, dd6.v[:, None]], 1), torch.cat([dp.S, dd6.S[:, None]], 1)).map(lambda v: v.transpose(1, 2).reshape(-1, feat + 1)),
               "F": f.map(to_cmajor)}
    out, S = _split(res)
    out["_open"] = S["_open"] = o6
    return _ret(out, S, cond)


def c6_case(mode, X1, X2, X3, w6, feat, N, rec, dm):
    ops = (X1, X2, X3, w6, feat, N, rec, dm)
    ref, S, plain = evaluate(lambda *o, cond=False: c6_bwd(mode, *o, cond=cond), *ops)
    o6 = ref.pop("_open")
    S.pop("_open"), plain.pop("_open")
    op = Open(o6)
    op.assert_cap(f"conv6 pass {mode}")
    slack, masks = {}, {}
    if op.n_open:
        fl = c6_bwd(mode, *R._cast(ops, F64), flip=True)
        if mode == 1:
            slack["partial"] = (fl["partial"] - ref["partial"]).abs()
        else:
            col = o6[:, None, :].expand(-1, 3, -1).reshape(-1, feat)
            masks["G6"] = torch.cat([col, torch.zeros(col.shape[0], 1, dtype=torch.bool)], 1)
            slack["G6"] = torch.zeros_like(ref["G6"])
            slack["G6"][:, feat] = (fl["G6"] - ref["G6"])[:, feat].abs()       # dd6 sums over the point's channels
    return ref, S, plain, slack, masks, op


def c6_dx(G6, w6, feat, cond=False):
    """C6_DX: row r of d cat(x1, x2, x3) = W6^T dp6 + w_dir^T dd6 -> three maps, 21 columns each + a zero"""
    def run(G6, w6):
        acc = G6[:, :feat + 1] @ w6[:(feat + 1) * V3].view(feat + 1, V3)
        return {f"dX{i + 1}": F.pad(acc[:, VC * i:VC * i + VC], (0, 1)) for i in range(3)}
    return _ret(run(G6, w6), run(G6.abs(), w6.abs()), cond)


# ------------------------------------------------------------------------------------------------ finalisers
def bn_fin_fwd(partial, count, gamma, beta, mom, eps, rm, rv, cond=False, biased=False):
    """BN_FIN_FWD: partial [nblk][2][C] (sums of n, n^2) -> mean, rstd = 1 / sqrt(max(E n^2 - mean^2, 0) + eps), the scale /
    shift slots gamma rstd, beta - mean gamma rstd, and torch's running statistics (momentum blend; the running variance
    takes the UNBIASED batch variance).  ``biased`` plants a defect (host module only)."""
    a, b = partial[:, 0].t().contiguous().sum(1), partial[:, 1].t().contiguous().sum(1)
    mean = a / count
    var = (b / count - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    sc = gamma * rstd
    unb = 1.0 if biased else count / (count - 1)
    out = {"mean": mean, "rstd": rstd, "scale": sc, "shift": beta - mean * sc,
           "run_mean": (1 - mom) * rm + mom * mean, "run_var": (1 - mom) * rv + mom * var * unb}
    if not cond:
        return out
    Sm = partial[:, 0].abs().t().contiguous().sum(1) / count
    Sv = partial[:, 1].abs().t().contiguous().sum(1) / count + mean * mean
    Sr = rstd + rstd / (2 * (var + eps)) * Sv
    Ssc = gamma.abs() * Sr
    return out, {"mean": Sm, "rstd": Sr, "scale": Ssc, "shift": beta.abs() + Sm * sc.abs() + mean.abs() * Ssc,
                 "run_mean": (1 - mom) * rm.abs() + mom * Sm, "run_var": (1 - mom) * rv.abs() + mom * Sv * count / (count - 1)}


def bn_fin_bwd(partial, count, dgamma0, dbeta0, cond=False, count_minus_one=False):
    """BN_FIN_BWD: partial (sums of dy, dy xhat) -> mean dy, mean dy xhat; dgamma = dgamma0 + sum dy xhat, dbeta = dbeta0 + sum dy"""
    def run(partial, g0, b0):
        a, b = partial[:, 0].t().contiguous().sum(1), partial[:, 1].t().contiguous().sum(1)
        return {"mdy": a / count, "mdyx": b / (count - 1 if count_minus_one else count), "dgamma": g0 + b, "dbeta": b0 + a}
    return _ret(run(partial, dgamma0, dbeta0), run(partial.abs(), dgamma0.abs(), dbeta0.abs()), cond)


# ------------------------------------------------------------------------------------------------ reverse adjacency, gather
def rev_adj(idx, N):
    """REV_ADJ by a numpy counting sort: for every point the edges (source point * 20 + rank) that end in it, ascending.
    -> cnt, ptr [pts], rev [pts * 20] (int32); exact."""
    idx = np.asarray(idx, dtype=np.int64)
    pts = idx.shape[0]
    dst = (np.arange(pts)[:, None] // N * N + idx).reshape(-1)
    cnt = np.bincount(dst, minlength=pts)
    ptr = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rev = np.argsort(dst, kind="stable")
    return cnt.astype(np.int32), ptr.astype(np.int32), rev.astype(np.int32)


def gather(E, cnt, rev, Wm, X, C, dXp0, cond=False, drop_edge=None):
    """GATHER: dT_j = [sum over the edges INTO j of dp_a | of dd_a | sum over j's own 20 edges of dp_a | of dd_a];
    dTc = dT component-major [pts * 3][84]; Xc = x component-major; dXp = dXp0 + Wm^T dT ([pts][3] for C = 1, else a
    component-major map, 21 columns used).  cnt / rev: the reverse adjacency (rev position t belongs to the point whose
    [ptr, ptr + cnt) holds t: the lists are contiguous and in point order).  ``drop_edge``: planted defect, position in rev."""
    pts = cnt.shape[0]
    owner = torch.repeat_interleave(torch.arange(pts), cnt.long())
    r = rev.long()
    if drop_edge is not None:
        keep = torch.ones_like(r, dtype=torch.bool)
        keep[drop_edge] = False
        owner, r = owner[keep], r[keep]

    def run(E, Wm, X, dXp0):
        e = E.view(-1, 2, ROW)[:, :, :V3]
        into = torch.zeros(pts, 2, V3, dtype=E.dtype).index_add_(0, owner, e[r])
        own = e.view(pts, KNN, 2, V3).sum(1)
        dT = torch.cat([into, own], 1).view(pts, 4, VC, 3)
        dTc = dT.permute(0, 3, 1, 2).reshape(pts * 3, 4 * VC)
        dx = torch.einsum("moc,pmok->pck", Wm.view(4, VC, C), dT)
        x = X[:, :3 * C].reshape(pts, C, 3)
        if C == 1:
            dXp = dXp0.view(pts, 3) + dx[:, 0]
        else:
            dXp = dXp0.clone().view(pts * 3, ROW)
            dXp[:, :VC] += dx.transpose(1, 2).reshape(pts * 3, VC)
        return {"dTc": dTc, "Xc": x.transpose(1, 2).reshape(pts * 3, C), "dXp": dXp}
    return _ret(run(E, Wm, X, dXp0), run(E.abs(), Wm.abs(), X.abs(), dXp0.abs()), cond)


def premap_wgrad(dWm, C, dwf0, dwd0, cond=False, keep_u=False):
    """PREMAP_WGRAD: W[:, :C] feeds A (x_j - x_i share) and U = (W[:, C:] - W[:, :C]) x_i, so dW[:, :C] = dWm_A - dWm_U and
    dW[:, C:] = dWm_U, for the feature map (blocks 0, 2) and the direction map (1, 3); added to dwf0 / dwd0 [21][2C].
    ``keep_u`` plants a defect: the U share not subtracted."""
    m = dWm.view(4, VC, C)

    def run(m, f0, d0, sub):
        return {"dwf": f0.view(VC, 2 * C) + torch.cat([m[0] - sub * m[2], m[2]], 1), "dwd": d0.view(VC, 2 * C) + torch.cat([m[1] - sub * m[3], m[3]], 1)}
    return _ret(run(m, dwf0, dwd0, 0.0 if keep_u else 1.0), run(m.abs(), dwf0.abs(), dwd0.abs(), -1.0), cond)


# ------------------------------------------------------------------------------------------------ head
def head_bwd(G, inv, feat, lin0=None, cond=False):
    """HEAD_BWD: the output is the pooled map m [feat][3] twice (inv = 0): dm = g[:3 feat] + g[3 feat:]; or linear0 of the mean
    over the 2 feat channels of [m, m] (inv = 1): dm[c][k] = sum_o g[o] W0[o][k] / feat."""
    def run(G, lin0):
        if not inv:
            return {"dm": G[:, :3 * feat] + G[:, 3 * feat:6 * feat]}
        s = G[:, :2 * feat] @ lin0[:6 * feat].view(2 * feat, 3) / feat
        return {"dm": s[:, None, :].expand(-1, feat, 3).reshape(-1, 3 * feat)}
    return _ret(run(G, lin0), run(G.abs(), None if lin0 is None else lin0.abs()), cond)


def lin0_grad(G, M, feat, dW0, db0, cond=False):
    """LIN0_GRAD: dW0[o][k] += sum_p G[p][o] xbar_p[k], db0[o] += sum_p G[p][o]; xbar_p = mean over the feat channels of m_p"""
    def run(G, M, dW0, db0):
        xbar = M[:, :3 * feat].reshape(-1, feat, 3).transpose(1, 2).contiguous().sum(-1) / feat
        g = G[:, :2 * feat]
        return {"dW0": dW0.view(2 * feat, 3) + g.t() @ xbar, "db0": db0 + g.t().contiguous().sum(1)}
    return _ret(run(G, M, dW0, db0), run(G.abs(), M.abs(), dW0.abs(), db0.abs()), cond)


# ------------------------------------------------------------------------------------------------ VnInv
def vn_lin(X, Wf, Wd, cin, cond=False):
    """VN_LIN: rows x [P][cin][3] -> P = Wf x, D = Wd x [P][cout][3]"""
    def run(X, Wf, Wd):
        x = X[:, :3 * cin].reshape(-1, cin, 3)
        return {"vP": torch.einsum("oc,pck->pok", Wf, x), "vD": torch.einsum("oc,pck->pok", Wd, x)}
    return _ret(run(X, Wf, Wd), run(X.abs(), Wf.abs(), Wd.abs()), cond)


def vn_stat(vP, cond=False):
    """VN_STAT: sums over the P fragments of n = |P| + eps and n^2 -> [1][2][cout]"""
    n = (vP * vP).sum(-1).sqrt() + EPS
    out = {"partial": torch.stack([n.t().contiguous().sum(1), (n * n).t().contiguous().sum(1)])[None]}
    return _ret(out, {"partial": out["partial"].clone()}, cond)


def vn_apply(vP, vD, rec, cond=False):
    """VN_APPLY: the vector activation on the record's batch statistics"""
    A = _act(V(vP), V(vD), rec_bn(rec, vP.shape[1]))
    return _ret({"vY": A.out.v}, {"vY": A.out.S}, cond)


gemm_tn = R.gemm_tn


# ------------------------------------------------------------------------------------------------ records, operands
def make_rec(mean=None, rstd=None, gamma=None, beta=None, mdy=None, mdyx=None, dtype=F32):
    rec = torch.zeros(REC, CMAX, dtype=dtype)
    for r, v in enumerate((mean, rstd, gamma, beta, mdy, mdyx)):
        if v is not None:
            rec[r, :v.numel()] = v.to(dtype)
    return rec


def knn_lists(x, N):
    """real kNN lists of rows x [pts][F] (fp64 scores as pcd_train_torch.torch_graph) -> [pts][20] int32, cloud-local"""
    f = x.double().view(-1, N, x.shape[1])
    sc = -(f * f).sum(-1)[:, :, None] + 2 * f @ f.transpose(1, 2) - (f * f).sum(-1)[:, None, :]
    return sc.topk(KNN, dim=-1)[1].reshape(-1, KNN).to(torch.int32)


def hub_lists(P, N, seed):
    """synthetic lists: point 0 of every cloud is in EVERY list (cnt = N), point N - 1 in none (cnt = 0); the rest random"""
    assert N >= KNN + 1
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(P * N, KNN, dtype=torch.int32)
    for r in range(P * N):
        out[r, 0] = 0
        out[r, 1:] = (torch.randperm(N - 2, generator=g)[:KNN - 1] + 1).to(torch.int32)
    return out


def perm_lists(P, N, seed):
    """N == 20: every list is a permutation of the cloud"""
    assert N == KNN
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(N, generator=g) for _ in range(P * N)]).to(torch.int32)


# ------------------------------------------------------------------------------------------------ packing, composition
def pack_premap(wf, wd, C):
    """map_to_feat / map_to_dir [21][2C] of a stage's first layer -> the premap blob [4][21][C] (diffassemble_amd/pcd_encoder.py)"""
    return torch.cat([t.reshape(-1) for t in (wf[:, :C], wd[:, :C], wf[:, C:] - wf[:, :C], wd[:, C:] - wd[:, :C])])


def pack_wb(wf, wd):
    return torch.cat([F.pad(wf, (0, 1)).reshape(-1), F.pad(wd, (0, 1)).reshape(-1), wf.new_zeros(2 * VC)])


def pack_w6(wf, wd):
    return torch.cat([wf.reshape(-1), wd.reshape(-1), wf.new_zeros(2 * wf.shape[0])])


def fin_to_rec(fin, gamma, beta):
    return make_rec(fin["mean"], fin["rstd"], gamma, beta, dtype=gamma.dtype)


def stage_chain(X, C, N, idx, Wm, bn_a, wb, bn_b, G, dt, flip=False):
    """One stage of the training path as the chain of this module's contracts in dtype ``dt``: premap -> STAT_A -> fin
    [-> STAT_B -> fin] -> pool, then with the gradient G [pts][21][3] of the pooled output BWD1 -> fin [-> BWD2 (+ the two
    weight GEMMs) -> fin] -> BWD3 -> reverse adjacency -> gather (+ the premap GEMM) -> premap_wgrad.  bn_a / bn_b: dicts
    gamma, beta, rm, rv, mom, eps (bn_b, wb None: a single-layer stage).  -> (out, S, open): S of the FINAL passes' outputs
    (their own condition terms on this chain's operands)."""
    c = lambda t: None if t is None else t.to(dt)                          # noqa: E731
    X, Wm, wb, G = c(X), c(Wm), c(wb), c(G)
    bn_a = {k: (c(v) if torch.is_tensor(v) else v) for k, v in bn_a.items()}
    bn_b = None if bn_b is None else {k: (c(v) if torch.is_tensor(v) else v) for k, v in bn_b.items()}
    pts = X.shape[0]
    count = float(pts * KNN)
    out, S = {}, {}
    T = premap(X, Wm, C)["T"]

    def fin(part, bn, tag):
        f = bn_fin_fwd(part, count, bn["gamma"], bn["beta"], bn["mom"], bn["eps"], bn["rm"], bn["rv"])
        out[f"run_mean_{tag}"], out[f"run_var_{tag}"] = f["run_mean"], f["run_var"]
        return fin_to_rec(f, bn["gamma"], bn["beta"])

    recA = fin(edge_stat_a(T, idx, N)["partial"], bn_a, "a")
    recB = None
    if wb is not None:
        recB = fin(edge_stat_b(T, idx, N, recA, wb)["partial"], bn_b, "b")
    out["X"] = edge_pool(T, idx, N, recA, recB, wb)["X"]
    dX = to_cmajor(G).reshape(-1)
    zero = lambda n: torch.zeros(n, dtype=dt)                             # noqa: E731

    def fin_b(part, rec, tag):
        f, s = bn_fin_bwd(part, count, zero(VC), zero(VC), cond=True)
        rec[R_MDY, :VC], rec[R_MDYX, :VC] = f["mdy"], f["mdyx"]
        out[f"dgamma_{tag}"], out[f"dbeta_{tag}"] = f["dgamma"], f["dbeta"]
        S[f"dgamma_{tag}"], S[f"dbeta_{tag}"] = s["dgamma"], s["dbeta"]

    kw = dict(flip=flip)
    last = "b" if wb is not None else "a"
    fin_b(edge_bwd(1, T, idx, N, recA, recB, wb, dX, **kw)["partial"], recB if wb is not None else recA, last)
    if wb is not None:
        b2 = edge_bwd(2, T, idx, N, recA, recB, wb, dX, **kw)
        for k, a in (("dwf_b", b2["Gb"][:, :VC]), ("dwd_b", b2["Gb"][:, VC:])):
            o, s = gemm_tn(a, b2["Hb"], torch.zeros(VC, VC, dtype=dt), cond=True)
            out[k], S[k] = o["C"], s["C"]
        fin_b(b2["partial"], recA, "a")
    b3 = edge_bwd(3, T, idx, N, recA, recB, wb, dX, **kw)
    oa, ob = b3["_open"]
    cnt, ptr, rev = (torch.from_numpy(v) for v in rev_adj(idx.numpy(), N))
    dXp0 = torch.zeros(pts * 3 if C == 1 else pts * 3 * ROW, dtype=dt)
    ga, gs = gather(b3["E"], cnt, rev, Wm, X, C, dXp0, cond=True)
    out["dXp"], S["dXp"] = ga["dXp"], gs["dXp"]
    o, s = gemm_tn(ga["dTc"], ga["Xc"], torch.zeros(4 * VC, C, dtype=dt), cond=True)
    w, ws = premap_wgrad(o["C"].reshape(-1), C, zero(VC * 2 * C), zero(VC * 2 * C), cond=True)
    _, ws = premap_wgrad(s["C"].reshape(-1), C, zero(VC * 2 * C), zero(VC * 2 * C), cond=True)
    out["dwf_a"], out["dwd_a"], S["dwf_a"], S["dwd_a"] = w["dwf"], w["dwd"], ws["dwf"], ws["dwd"]
    return out, S, (Open(oa, ob) if wb is not None else Open(oa))
