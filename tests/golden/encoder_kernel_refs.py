"""fp64 contracts of the piece encoder's training primitives (include/diffassemble_hip.h, "Training path of the 2D piece
encoder") and the rule that judges a kernel against them.  Used by tests/test_encoder_kernel_refs.py (host: pins the
contracts against torch's own operators / autograd and shows that the rule tells a right evaluation from a subtly wrong
one) and tests/test_gpu_encoder_kernels.py (the HIP kernels).

Every contract is a plain torch function of the STORED operands (for bf16 maps: the bf16 values, widened) in the zero-haloed
NHWC layout [B][H+2][H+2][C4]; it runs in the dtype of its operands, so the same code gives

    ref    the contract in fp64,
    S      its condition term: the same expression on absolute values (sum |x||w| + |bias| + |res| for a convolution,
           sum |y| / n for a mean, ...), returned with ``cond=True``,
    plain  the contract in fp32 (torch on the CPU), before any rounding to the stored type.

The rule (``judge``), for every element i of every output:

    |got_i - ref_i| <= u_out |ref_i| + FACTOR e_acc(plain) S_i,      e_acc(plain) = max_i |plain_i - ref_i| / S_i

u_out = unit roundoff of the stored type (one rounding to nearest of the final value: 2^-8 for bf16, 2^-24 for fp32; a store
that truncates errs by up to twice that and must fail); e_acc(plain) is the reference arithmetic's own accumulation error,
computed per case and never from the code under test; FACTOR = 16 is the allowance this project already gives a kernel that
sums in another order than torch (tests/test_gpu_pcd_train.py).  Accumulation error is judged per element against S_i, not
against the tensor's maximum: a wrong border pixel or a wrong small channel counts as much as a wrong large one.  Where
S_i = 0 (halo cells, zero-stuffed cells) the bound is zero: the value must be exact.
"""
import torch
import torch.nn.functional as F

from oracle.encoder import p4_filter_bank

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -8}
# FACTOR of the rule per kernel; one table, read by the host module and the GPU module alike.  A wider entry needs the
# measured e(HIP), e_acc(plain) and the reason in the docstring of the test that uses it.
FACTOR = {"default": 16.0}
BN_EPS = float(torch.tensor(1e-5, dtype=F32))                       # the kernels' fp32 literal 1e-5f
MEAN3 = torch.tensor([0.4850, 0.4560, 0.4060], dtype=F32)           # the kernels' fp32 literals (efficient_gat.py:109-112)
SD3 = torch.tensor([0.2290, 0.2240, 0.2250], dtype=F32)


def factor(kernel="default"):
    return FACTOR.get(kernel, FACTOR["default"])


# ------------------------------------------------------------------------------------------------ layout / packing
def halo(x):
    """[B, C, H, W] -> zero-haloed NHWC [B, H+2, W+2, C]"""
    return F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).contiguous()


def unhalo(x):
    return x[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)


def with_halo(y):
    """interior NHWC [B, H, H, C] -> [B, H+2, H+2, C] with a zero halo"""
    return F.pad(y, (0, 0, 1, 1, 1, 1)).contiguous()


def halo_is_zero(m):
    return all(float(t.float().abs().max()) == 0.0 for t in (m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1]))


def pack_fwd(bank):                       # [O4, I4, k, k] -> [O4, k*k*I4]  (tap-major, channel-minor)
    return bank.permute(0, 2, 3, 1).reshape(bank.shape[0], -1).contiguous()


def pack_dgrad(bank):                     # -> [I4, k*k*O4], taps flipped: conv(dY, .) is the input gradient
    return bank.flip(2, 3).permute(1, 2, 3, 0).reshape(bank.shape[1], -1).contiguous()


def stored(t, dt):
    """the values a kernel reads when ``t`` is kept in the storage type ``dt`` (round to nearest even), as fp64"""
    return t.to(dt).double()


def _cast(ops, dt):
    return [o.to(dt) if torch.is_tensor(o) and o.is_floating_point() else o for o in ops]


def evaluate(contract, *ops, **kw):
    """-> (ref, S, plain): dicts name -> tensor of the contract in fp64, its condition term, and the contract in fp32"""
    ref, S = contract(*_cast(ops, F64), cond=True, **kw)
    plain = contract(*_cast(ops, F32), cond=False, **kw)
    return ref, S, plain


# ------------------------------------------------------------------------------------------------ the rule
def e_acc(plain, ref, S):
    d = (plain.double() - ref).abs()
    assert bool((d[S == 0] == 0).all()), "the plain evaluation differs from the reference where the condition term is zero"
    m = S > 0
    return float((d[m] / S[m]).max()) if bool(m.any()) else 0.0


def judge(got, ref, S, plain, out_dtype, kernel="default"):
    """The rule of the module docstring.  -> dict(ok, e_hip, e_acc, bad, n, worst): e_hip = max_i (|got_i - ref_i| -
    u_out |ref_i|)+ / S_i is the figure to hold against FACTOR e_acc; bad = number of elements over the bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ea = e_acc(plain, ref, S)
    err = (got - ref).abs()
    slack = U_OUT[out_dtype] * ref.abs()
    bad = (err > slack + factor(kernel) * ea * S) | ~torch.isfinite(got)
    over = (err - slack).clamp_min(0)
    m = S > 0
    eh = float((over[m] / S[m]).max()) if bool(m.any()) else 0.0
    if bool((over[~m] > 0).any()):
        eh = float("inf")
    nbad = int(bad.sum())
    worst = None
    if nbad:
        i = int(torch.where(bad.flatten(), err.flatten(), torch.zeros(()).double()).argmax())
        worst = (tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)), float(got.flatten()[i]), float(ref.flatten()[i]),
                 float(S.flatten()[i]))
    return {"ok": nbad == 0, "e_hip": eh, "e_acc": ea, "bad": nbad, "n": ref.numel(), "worst": worst}


def rel_max(got, ref):
    """the project's older bound for fp32 primitives: max-abs error / max-abs reference (tests/test_gpu_encoder_train.py)"""
    return float((got.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------ contracts
def conv(X, Wp, bias, res, relu=0, k=3, stride=1, cond=False):
    """da_enc_conv: Y = conv(X, W) + bias [+ res] [ReLU].  X [B][Hi+2][Hi+2][Cin] as stored INCLUDING its halo (the kernel
    reads it; it must be zero for the result to be a padded convolution), Wp [Cout][k*k*Cin] tap-major, res / Y
    [B][Ho+2][Ho+2][Cout]; a 1x1 filter reads the pixel itself.  The halo of Y is zero (never written)."""
    Hi, Cin, Cout = X.shape[1] - 2, X.shape[3], Wp.shape[0]
    w = Wp.view(Cout, k, k, Cin).permute(0, 3, 1, 2)
    x = X.permute(0, 3, 1, 2)
    if k == 1:
        x = x[:, :, 1:Hi + 1, 1:Hi + 1]

    def run(x, w, b, r):
        y = F.conv2d(x, w, b, stride=stride).permute(0, 2, 3, 1)
        return y if r is None else y + r[:, 1:-1, 1:-1]
    y = run(x, w, bias, res)
    out = {"Y": with_halo(F.relu(y) if relu else y)}
    if not cond:
        return out
    return out, {"Y": with_halo(run(x.abs(), w.abs(), bias.abs(), None if res is None else res.abs()))}


def upsample2(S, cond=False):
    """da_enc_upsample2: Up (interior 2H x 2H) = S(i, j) at interior (2i, 2j), zero elsewhere."""
    B, Hp, _, C = S.shape
    H = Hp - 2
    up = S.new_zeros(B, 2 * H + 2, 2 * H + 2, C)
    up[:, 1:2 * H + 1:2, 1:2 * H + 1:2] = S[:, 1:-1, 1:-1]
    return ({"Up": up}, {"Up": up.abs()}) if cond else {"Up": up}


def dgrad(dY, bank, res, k=3, stride=1, cond=False):
    """The engine's input gradient of a unit: da_enc_conv on dY (zero-stuffed first for a stride-2 unit) with the
    flipped / transposed bank, ``res`` accumulating the other gradient paths."""
    if stride == 2:
        dY = upsample2(dY)["Up"]
    zero = dY.new_zeros(bank.shape[1])
    return conv(dY, pack_dgrad(bank), zero, res, 0, k, 1, cond=cond)


def _normalised(P):
    m, s = MEAN3.to(P.dtype).view(1, 3, 1, 1), SD3.to(P.dtype).view(1, 3, 1, 1)
    return (P - m) / s, (P.abs() + m) / s


def stem(P, w, bias, relu=0, cond=False):
    """da_enc_stem: normalise, 3x3 convolution (zero padding of the NORMALISED image) with w [128][c*9 + ky*3 + kx] + bias
    [ReLU] -> [B][34][34][128]."""
    xn, xa = _normalised(P)
    y = F.conv2d(xn, w.view(128, 3, 3, 3), bias, padding=1).permute(0, 2, 3, 1)
    out = {"Y": with_halo(F.relu(y) if relu else y)}
    if not cond:
        return out
    return out, {"Y": with_halo(F.conv2d(xa, w.abs().view(128, 3, 3, 3), bias.abs(), padding=1).permute(0, 2, 3, 1))}


def stem_im2col(P, cond=False):
    """da_enc_stem_im2col: cols [B][34][34][32], channel t = c*9 + ky*3 + kx < 27 = the normalised crop at (y+ky-1, x+kx-1)
    (zero outside the crop), channels 27..31 and the halo zero."""
    B = P.shape[0]
    xn, xa = _normalised(P)

    def cols(x):
        u = F.unfold(x, 3, padding=1).view(B, 27, 32, 32).permute(0, 2, 3, 1)
        return F.pad(u, (0, 5, 1, 1, 1, 1)).contiguous()
    return ({"cols": cols(xn)}, {"cols": cols(xa)}) if cond else {"cols": cols(xn)}


def _planes(M):
    """haloed map -> interior values [pixels, planes, 4]"""
    C4 = M.shape[3]
    return M[:, 1:-1, 1:-1].reshape(-1, C4 // 4, 4)


def _psum(t):
    """[pixels, planes, 4] -> per-plane sums.  Over a contiguous last dimension, where torch adds pairwise: summed along the
    strided pixel dimension its fp32 result is a running sum per plane (e_acc 2e-6 at 4 000 pixels instead of 1e-7), and a
    plain evaluation that poor would make the rule lax."""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1).sum(1)


def bn_stats(Y, cond=False):
    """da_enc_bn_stats: mean and biased variance per plane over (B, 4, H, W).  The variance's condition term is the
    variance itself: sum |y - m|^2 / n has no cancellation, whatever the plane's mean."""
    y = _planes(Y)
    n = y.shape[0] * 4
    mean = _psum(y) / n
    var = _psum((y - mean.view(1, -1, 1)) ** 2) / n
    out = {"mean": mean, "var": var}
    return (out, {"mean": _psum(y.abs()) / n, "var": var.clone()}) if cond else out


def _per_channel(v):
    return v.repeat_interleave(4).view(1, 1, 1, -1)


def bn_apply(Y, mean, var, gamma, beta, res, relu=0, cond=False):
    """da_enc_bn_apply: Z = (Y - mean) * (rsqrt(var + 1e-5) * gamma) + beta [+ res] [ReLU] on the interior."""
    sc = _per_channel(torch.rsqrt(var + BN_EPS) * gamma)
    y, r = Y[:, 1:-1, 1:-1], (None if res is None else res[:, 1:-1, 1:-1])
    z = (y - _per_channel(mean)) * sc + _per_channel(beta)
    if r is not None:
        z = z + r
    out = {"Z": with_halo(F.relu(z) if relu else z)}
    if not cond:
        return out
    s = (y.abs() + _per_channel(mean.abs())) * sc.abs() + _per_channel(beta.abs())
    return out, {"Z": with_halo(s if r is None else s + r.abs())}


def bn_backward(dZ, Z, Y, mean, var, gamma, dgamma0, dbeta0, relu=0, want_dres=True, drop_xhat_term=False, cond=False):
    """da_enc_bn_backward: g = dZ [where Z > 0, on the Z passed in]; dgamma = dgamma0 + sum g xhat; dbeta = dbeta0 + sum g;
    dY = gamma rstd (g - mean(g) - xhat mean(g xhat)); dRes = g.  ``drop_xhat_term`` plants a defect (host module only)."""
    shape = dZ[:, 1:-1, 1:-1].shape
    g, y = _planes(dZ), _planes(Y)
    if relu:
        g = torch.where(_planes(Z) > 0, g, torch.zeros_like(g))
    n = g.shape[0] * 4
    rstd = torch.rsqrt(var + BN_EPS).view(1, -1, 1)
    mu = mean.view(1, -1, 1)
    xh = (y - mu) * rstd
    s1, s2 = _psum(g), _psum(g * xh)
    k = (gamma.view(1, -1, 1) * rstd)
    dY = k * (g - (s1 / n).view(1, -1, 1) - (0 if drop_xhat_term else xh * (s2 / n).view(1, -1, 1)))
    out = {"dgamma": dgamma0 + s2, "dbeta": dbeta0 + s1, "dY": with_halo(dY.reshape(shape))}
    if want_dres:
        out["dRes"] = with_halo(g.reshape(shape))
    if not cond:
        return out
    xa = (y.abs() + mu.abs()) * rstd
    a1, a2 = _psum(g.abs()), _psum(g.abs() * xa)
    S = {"dgamma": dgamma0.abs() + a2, "dbeta": dbeta0.abs() + a1,
         "dY": with_halo((k.abs() * (g.abs() + (a1 / n).view(1, -1, 1) + xa * (a2 / n).view(1, -1, 1))).reshape(shape))}
    if want_dres:
        S["dRes"] = with_halo(g.abs().reshape(shape))
    return out, S


def gemm_tn(A, B, C0, cond=False):
    """da_gemm_tn_f32 / da_gemm_tn_bf16: C = C0 + A^T B over the rows.  A [M, N], B [M, K] (the used columns)."""
    out = {"C": C0 + A.t() @ B}
    return (out, {"C": C0.abs() + A.abs().t() @ B.abs()}) if cond else out


def colsum(A, out0, cond=False):
    """da_colsum_f32: out = out0 + sum_m A[m]"""
    out = {"out": out0 + A.t().contiguous().sum(1)}                     # (contiguous: torch adds pairwise, see _psum)
    return (out, {"out": out0.abs() + A.abs().t().contiguous().sum(1)}) if cond else out


def bank_grad(dbank, dW0, table, cond=False):
    """da_enc_bank_grad: dW[i] = dW0[i] + sum_{r<4} dbank[table[i][r]]"""
    t = table.long()
    out = {"dW": dW0 + dbank.reshape(-1)[t].sum(1)}
    return (out, {"dW": dW0.abs() + dbank.abs().reshape(-1)[t].sum(1)}) if cond else out


def _gather_bank(dbank4, wshape):
    """backward of oracle.encoder.p4_filter_bank (an index gather): the sum of the bank entries every parameter feeds"""
    w = torch.zeros(wshape, dtype=dbank4.dtype, requires_grad=True)
    (p4_filter_bank(w) * dbank4).sum().backward()
    return w.grad


def wgrad(dY, X, dW0, k=3, stride=1, transpose_taps=False, cond=False):
    """EncoderTrainEngine._wgrad: the parameter gradient of one group convolution from the haloed maps as they lie in
    memory.  dY [B][Ho+2][Ho+2][O4] (zero-stuffed to the input resolution first for stride 2), X [B][H+2][H+2][I4];
    dBank[o][tap][c] = sum_q dY[q][o] X[q + offset(tap)][c] over the haloed positions q, then the 4-way gather-sum into
    dW0 [O, I, 4, k, k].  ``transpose_taps`` plants a defect (host module only)."""
    if stride == 2:
        dY = upsample2(dY)["Up"]
    Wp, O4, I4 = X.shape[1], dY.shape[3], X.shape[3]
    assert dY.shape[:3] == X.shape[:3]
    a, x = dY.reshape(-1, O4), X.reshape(-1, I4)
    rows = a.shape[0] - 2 * (Wp + 1)

    def run(a, x, dW0):
        a = a[Wp + 1:Wp + 1 + rows]
        taps = []
        for tap in range(k * k):
            ky, kx = (tap // 3, tap % 3) if k == 3 else (1, 1)
            if transpose_taps:
                ky, kx = kx, ky
            off = (Wp + 1) + (ky - 1) * Wp + (kx - 1)
            taps.append(a.t() @ x[off:off + rows])                      # [O4, I4]
        dbank4 = torch.stack(taps, 2).view(O4, I4, k, k)
        return dW0 + _gather_bank(dbank4, dW0.shape)
    out = {"dW": run(a, x, dW0)}
    return (out, {"dW": run(a.abs(), x.abs(), dW0.abs())}) if cond else out


def stem_wgrad(dY, P, dW0, cond=False):
    """The stem's parameter gradient as the engine forms it: dBank [128][27] = dY^T im2col(P) over the haloed rows, then
    the gather-sum into dW0 [32, 3, 1, 3, 3]."""
    def run(a, cols, dW0):
        return dW0 + _gather_bank((a.reshape(-1, 128).t() @ cols.reshape(-1, 32)[:, :27]).view(128, 3, 3, 3), dW0.shape)
    if cond:
        c, ca = stem_im2col(P, cond=True)
        return {"dW": run(dY, c["cols"], dW0)}, {"dW": run(dY.abs(), ca["cols"], dW0.abs())}
    return {"dW": run(dY, stem_im2col(P)["cols"], dW0)}
