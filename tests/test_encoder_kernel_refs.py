"""Host tests of tests/golden/encoder_kernel_refs.py, the references the GPU kernel tests of the piece encoder's training
primitives (tests/test_gpu_encoder_kernels.py) are judged against.  No GPU.

1. Every fp64 contract equals torch's own operator or autograd in fp64 to 1e-12.
2. The comparator is sensitive: a plain torch evaluation of a contract (fp32; fp32 with ONE round-to-nearest-even to bf16 at
   the store; fp32 summed in another order) passes the rule, the same evaluation with one planted defect fails it.  The
   defects are planted in the CPU evaluation only.
"""
import pytest
import torch
import torch.nn.functional as F

import encoder_kernel_refs as R
from oracle import encoder as OE

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def rn_bf16(t):
    return t.float().to(BF16)


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (round towards zero)"""
    return (t.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def passes(got, ref, S, plain, out_dtype):
    return all(R.judge(got[k], ref[k], S[k], plain[k], out_dtype)["ok"] for k in ref)


def rnd(*shape, seed=0, dtype=F64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ 1. the contracts
def test_table_and_packing_match_the_engine():
    """one FACTOR table, default 16; the helper's packers are the engine's"""
    assert R.factor() == 16.0 and all(v >= 16.0 for v in R.FACTOR.values())
    assert R.U_OUT[BF16] == 2.0 ** -8 and R.U_OUT[F32] == 2.0 ** -24
    from diffassemble_amd.encoder_train import EncoderTrainEngine as E
    bank = rnd(8, 12, 3, 3)
    assert torch.equal(R.pack_fwd(bank), E._pack_fwd(bank)) and torch.equal(R.pack_dgrad(bank), E._pack_dgrad(bank))


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2), (1, 1)])
def test_conv_dgrad_wgrad_contracts_vs_autograd(k, stride):
    B, cin, cout, H = 3, 3, 5, 8
    Ho = H // stride
    w = (rnd(cout, cin, 4, k, k, seed=1) * 0.3).requires_grad_(True)
    x = rnd(B, cin * 4, H, H, seed=2).requires_grad_(True)
    bias, res = rnd(cout * 4, seed=3), rnd(B, cout * 4, Ho, Ho, seed=4)
    bank = OE.p4_filter_bank(w)
    y = F.conv2d(x, bank, None, stride=stride, padding=k // 2)
    dy = rnd(*y.shape, seed=5)
    y.backward(dy)
    X, dY, bankd = R.halo(x.detach()), R.halo(dy), bank.detach()
    for relu in (0, 1):
        for r in (None, R.halo(res)):
            got, S = R.conv(X, R.pack_fwd(bankd), bias, r, relu, k, stride, cond=True)
            want = y.detach() + bias.view(1, -1, 1, 1) + (0 if r is None else res)
            want = F.relu(want) if relu else want
            assert close(R.unhalo(got["Y"]), want) and R.halo_is_zero(got["Y"])
            s_want = F.conv2d(x.detach().abs(), bankd.abs(), bias.abs(), stride=stride, padding=k // 2) + (0 if r is None else res.abs())
            assert close(R.unhalo(S["Y"]), s_want)
    prior = R.halo(rnd(*x.shape, seed=6))
    got = R.dgrad(dY, bankd, prior, k, stride)["Y"]
    assert close(R.unhalo(got), x.grad + R.unhalo(prior)) and R.halo_is_zero(got)
    dW0 = rnd(*w.shape, seed=7)
    got, S = R.wgrad(dY, X, dW0, k, stride, cond=True)
    assert close(got["dW"], dW0 + w.grad)
    assert bool((S["dW"] >= got["dW"].abs() - 1e-12).all())


def test_stem_contracts_vs_torch():
    B = 2
    P = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(0), dtype=F64)
    w = (rnd(32, 3, 1, 3, 3, seed=1) * 0.3).requires_grad_(True)
    bias = rnd(128, seed=2)
    xn = (P - R.MEAN3.double().view(1, 3, 1, 1)) / R.SD3.double().view(1, 3, 1, 1)
    y = F.conv2d(xn, OE.p4_filter_bank(w), None, padding=1)
    dy = rnd(*y.shape, seed=3)
    y.backward(dy)
    bank = OE.p4_filter_bank(w).detach().reshape(128, 27)
    for relu in (0, 1):
        want = y.detach() + bias.view(1, -1, 1, 1)
        got = R.stem(P, bank, bias, relu)["Y"]
        assert close(R.unhalo(got), F.relu(want) if relu else want) and R.halo_is_zero(got)
    cols = R.stem_im2col(P)["cols"]
    assert R.halo_is_zero(cols) and float(cols[..., 27:].abs().max()) == 0
    # the im2col IS the convolution's operand: cols . bank^T reproduces the stem
    assert close((cols[:, 1:-1, 1:-1, :27] @ bank.t()).permute(0, 3, 1, 2), y.detach())
    dW0 = rnd(*w.shape, seed=4)
    assert close(R.stem_wgrad(R.halo(dy), P, dW0)["dW"], dW0 + w.grad)
    # the kernels' constants are the oracle's
    assert torch.equal(R.MEAN3, OE.MEAN.flatten().float()) and torch.equal(R.SD3, OE.STD.flatten().float())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_contracts_vs_batch_norm_autograd(relu, with_res):
    B, planes, H = 3, 5, 4
    y = (rnd(B, planes, 4, H, H, seed=1) * 2 + 3).requires_grad_(True)
    gamma = (torch.rand(planes, dtype=F64) + 0.5).requires_grad_(True)
    beta = rnd(planes, seed=2).requires_grad_(True)
    res = rnd(B, planes, 4, H, H, seed=3).requires_grad_(True)
    z = F.batch_norm(y, None, None, gamma, beta, True, 0.1, R.BN_EPS)
    if with_res:
        z = z + res
    z = F.relu(z) if relu else z
    dz = rnd(*z.shape, seed=4)
    z.backward(dz)
    f = lambda t: R.halo(t.detach().reshape(B, planes * 4, H, H))  # noqa: E731
    Y = f(y)
    st, S = R.bn_stats(Y, cond=True)
    yd = y.detach()
    assert close(st["mean"], yd.mean((0, 2, 3, 4))) and close(st["var"], yd.var((0, 2, 3, 4), unbiased=False))
    assert close(S["mean"], yd.abs().mean((0, 2, 3, 4)))
    Z = R.bn_apply(Y, st["mean"], st["var"], gamma.detach(), beta.detach(), f(res) if with_res else None, relu)["Z"]
    assert close(Z, f(z)) and R.halo_is_zero(Z)
    dg0, db0 = rnd(planes, seed=5), rnd(planes, seed=6)
    bw, S = R.bn_backward(f(dz), Z, Y, st["mean"], st["var"], gamma.detach(), dg0, db0, relu, want_dres=with_res, cond=True)
    assert close(bw["dY"], f(y.grad)) and R.halo_is_zero(bw["dY"])
    assert close(bw["dgamma"], dg0 + gamma.grad) and close(bw["dbeta"], db0 + beta.grad)
    assert ("dRes" in bw) == with_res
    if with_res:
        assert close(bw["dRes"], f(res.grad))
    for k in bw:
        assert bool((S[k] >= bw[k].abs() * (1 - 1e-12)).all()), k


def test_small_contracts_vs_torch():
    s = rnd(2, 6, 6, 8, seed=1)
    s[:, 0] = 0; s[:, -1] = 0; s[:, :, 0] = 0; s[:, :, -1] = 0          # noqa: E702
    # zero-stuffing is the adjoint of sampling the even pixels (what a stride-2 convolution does after a stride-1 one)
    up = R.upsample2(s)["Up"]
    assert up.shape == (2, 10, 10, 8) and torch.equal(up[:, 1:-1:2, 1:-1:2], s[:, 1:-1, 1:-1]) and R.halo_is_zero(up)
    assert int((up != 0).sum()) == int((s != 0).sum())                    # nothing anywhere else
    A, B, C0 = rnd(70, 9, seed=2), rnd(70, 5, seed=3), rnd(9, 5, seed=4)
    assert close(R.gemm_tn(A, B, C0)["C"], C0 + torch.einsum("mn,mk->nk", A, B))
    assert close(R.colsum(A, C0[:, 0])["out"], C0[:, 0] + A.sum(0))
    w = torch.zeros(3, 2, 4, 3, 3, dtype=F64, requires_grad=True)
    bank = OE.p4_filter_bank(w)
    db = rnd(*bank.shape, seed=5)
    (bank * db).sum().backward()
    src = OE.p4_filter_bank(torch.arange(w.numel()).view(w.shape)).reshape(-1)
    table = torch.argsort(src, stable=True).to(torch.int32).view(w.numel(), 4)
    dW0 = rnd(w.numel(), seed=6)
    assert close(R.bank_grad(db, dW0, table)["dW"], dW0 + w.grad.reshape(-1))


# ------------------------------------------------------------------------------------------------ 2. the comparator
def _conv_case(k=3, stride=1, storage=F32, seed=0):
    B, Cin, Cout, H = 2, 128, 128, 8
    X = R.halo(R.stored(rnd(B, Cin, H, H, seed=seed), storage))
    Wp = R.stored(rnd(Cout, k * k * Cin, seed=seed + 1) * 0.05, storage)
    bias = rnd(Cout, seed=seed + 2).float().double()
    res = R.halo(R.stored(rnd(B, Cout, H // stride, H // stride, seed=seed + 3), storage))
    return X, Wp, bias, res


@pytest.mark.parametrize("storage", [F32, BF16], ids=["fp32", "bf16"])
def test_rule_passes_plain_conv_and_fails_planted_defects(storage):
    X, Wp, bias, res = _conv_case(storage=storage)
    ref, S, plain = R.evaluate(R.conv, X, Wp, bias, res, relu=1)
    store = (lambda t: t.to(storage))
    assert passes({"Y": store(plain["Y"])}, ref, S, plain, storage)
    # another summation order: tap by tap, the residual first
    Cin = X.shape[3]
    acc = res.float()[:, 1:-1, 1:-1] + bias.float()
    for tap in range(9):
        wt = torch.zeros_like(Wp)
        wt[:, tap * Cin:(tap + 1) * Cin] = Wp[:, tap * Cin:(tap + 1) * Cin]
        acc = acc + R.conv(X.float(), wt.float(), torch.zeros(128), None)["Y"][:, 1:-1, 1:-1]
    assert passes({"Y": store(R.with_halo(F.relu(acc)))}, ref, S, plain, storage)
    # one tap dropped from the 3x3 filter
    wd = Wp.clone()
    wd[:, 4 * Cin:5 * Cin] = 0
    assert not passes({"Y": store(R.conv(X.float(), wd.float(), bias.float(), res.float(), 1)["Y"])}, ref, S, plain, storage)
    # ONE channel of one tap dropped: a small error in every pixel
    wd = Wp.clone()
    wd[:, 7 * Cin + 5] = 0
    assert not passes({"Y": store(R.conv(X.float(), wd.float(), bias.float(), res.float(), 1)["Y"])}, ref, S, plain, storage)
    # one halo row of X holds stale values
    Xs = X.clone()
    Xs[1, 0] = X[0, 3]
    assert not passes({"Y": store(R.conv(Xs.float(), Wp.float(), bias.float(), res.float(), 1)["Y"])}, ref, S, plain, storage)
    # the residual overwritten instead of added to (the in-place form accumulates gradient paths)
    assert not passes({"Y": store(R.conv(X.float(), Wp.float(), bias.float(), None, 1)["Y"])}, ref, S, plain, storage)
    # a written halo cell
    bad = plain["Y"].clone()
    bad[0, 0, 3, 7] = 1e-30
    assert not passes({"Y": store(bad)}, ref, S, plain, F32)


def test_rule_fails_truncated_bf16_store_and_passes_rounded():
    X, Wp, bias, res = _conv_case(storage=BF16, seed=10)
    for relu, r in ((0, None), (1, res)):
        ref, S, plain = R.evaluate(R.conv, X, Wp, bias, r, relu=relu)
        assert passes({"Y": rn_bf16(plain["Y"])}, ref, S, plain, BF16)
        j = R.judge(trunc_bf16(plain["Y"]), ref["Y"], S["Y"], plain["Y"], BF16)
        assert not j["ok"] and j["bad"] > 0.1 * (X.shape[0] * 8 * 8 * 128), j
    # BatchNorm output, bf16 maps
    Y = R.halo(R.stored(rnd(4, 128, 8, 8, seed=11) + 4.0, BF16))
    st = R.bn_stats(Y)
    g, b = torch.rand(32, dtype=F64) + 0.5, rnd(32, seed=12)
    ref, S, plain = R.evaluate(R.bn_apply, Y, st["mean"].float(), st["var"].float(), g.float(), b.float(), None, relu=0)
    assert passes({"Z": rn_bf16(plain["Z"])}, ref, S, plain, BF16)
    assert not passes({"Z": trunc_bf16(plain["Z"])}, ref, S, plain, BF16)


@pytest.mark.parametrize("storage", [F32, BF16], ids=["fp32", "bf16"])
def test_rule_on_wgrad_and_gemm_defects(storage):
    B, C, H = 3, 128, 8
    dY = R.halo(R.stored(rnd(B, C, H, H, seed=20), storage))
    X = R.halo(R.stored(rnd(B, C, H, H, seed=21), storage))
    dW0 = rnd(32, 32, 4, 3, 3, seed=22).float().double()
    ref, S, plain = R.evaluate(R.wgrad, dY, X, dW0)
    assert passes(plain, ref, S, plain, F32)
    # taps transposed (ky <-> kx)
    assert not passes(R.wgrad(dY.float(), X.float(), dW0.float(), transpose_taps=True), ref, S, plain, F32)
    # dW overwritten instead of added to
    assert not passes(R.wgrad(dY.float(), X.float(), torch.zeros_like(dW0).float()), ref, S, plain, F32)
    # TN GEMM: the last row chunk left out; C overwritten
    M, N, K = 1000, 128, 96
    A, Bm, C0 = R.stored(rnd(M, N, seed=23), storage), R.stored(rnd(M, K, seed=24), storage), rnd(N, K, seed=25).float().double()
    ref, S, plain = R.evaluate(R.gemm_tn, A, Bm, C0)
    assert passes(plain, ref, S, plain, F32)
    # another order: 32-row chunks in four row splits, summed in sequence
    parts = [sum((A[i:i + 32].float().t() @ Bm[i:i + 32].float() for i in range(s, min(M, s + 256), 32)), torch.zeros(N, K)) for s in range(0, M, 256)]
    assert passes({"C": C0.float() + sum(parts, torch.zeros(N, K))}, ref, S, plain, F32)
    assert not passes(R.gemm_tn(A[:M - 8].float(), Bm[:M - 8].float(), C0.float()), ref, S, plain, F32)
    assert not passes(R.gemm_tn(A[:M - 1].float(), Bm[:M - 1].float(), C0.float()), ref, S, plain, F32)
    assert not passes(R.gemm_tn(A.float(), Bm.float(), torch.zeros_like(C0).float()), ref, S, plain, F32)
    # column sum: += and the last row
    ref, S, plain = R.evaluate(R.colsum, A, C0[:, 0])
    assert passes(plain, ref, S, plain, F32)
    assert not passes(R.colsum(A.float(), torch.zeros(N)), ref, S, plain, F32)
    assert not passes(R.colsum(A[:-1].float(), C0[:, 0].float()), ref, S, plain, F32)


@pytest.mark.parametrize("storage", [F32, BF16], ids=["fp32", "bf16"])
def test_rule_on_batchnorm_and_upsample_defects(storage):
    B, C4, H = 4, 128, 8
    planes = C4 // 4
    Y = R.halo(R.stored(rnd(B, C4, H, H, seed=30) + 4.0, storage))                    # |mean| / std = 4
    dZ = R.halo(R.stored(rnd(B, C4, H, H, seed=31), storage))
    gamma, beta = (torch.rand(planes) + 0.5).double(), rnd(planes, seed=32).float().double()
    ref, S, plain = R.evaluate(R.bn_stats, Y)
    assert passes(plain, ref, S, plain, F32)
    # the variance of a shifted plane as E[y^2] - m^2 in fp32 loses what the rule asks for
    y = Y.float()[:, 1:-1, 1:-1].reshape(-1, planes, 4)
    naive = (y * y).mean((0, 2)) - y.mean((0, 2)) ** 2
    assert not passes({"mean": plain["mean"], "var": naive}, ref, S, plain, F32)
    mean, var = ref["mean"].float().double(), ref["var"].float().double()
    Z = R.stored(R.bn_apply(Y, mean, var, gamma, beta, None, relu=1)["Z"], storage)
    dg0, db0 = rnd(planes, seed=33).float().double(), rnd(planes, seed=34).float().double()
    ops = (dZ, Z, Y, mean, var, gamma, dg0, db0)
    ref, S, plain = R.evaluate(R.bn_backward, *ops, relu=1)
    st = lambda d: {k: (v.to(storage) if v.dim() == 4 else v) for k, v in d.items()}  # noqa: E731
    assert passes(st(plain), {k: ref[k] for k in ("dY", "dRes")}, S, plain, storage)
    assert passes(plain, {k: ref[k] for k in ("dgamma", "dbeta")}, S, plain, F32)
    f32 = R._cast(ops, F32)
    # without the xhat * mean(g xhat) term
    assert not passes(st(R.bn_backward(*f32, relu=1, drop_xhat_term=True)), {"dY": ref["dY"]}, S, plain, storage)
    # dgamma / dbeta overwritten instead of added to
    z32 = R.bn_backward(*f32[:6], torch.zeros(planes), torch.zeros(planes), relu=1)
    assert not passes(z32, {"dgamma": ref["dgamma"]}, S, plain, F32) and not passes(z32, {"dbeta": ref["dbeta"]}, S, plain, F32)
    # the ReLU mask ignored
    assert not passes(st(R.bn_backward(*f32, relu=0)), {"dRes": ref["dRes"]}, S, plain, storage)
    # upsample2 writing S(i, j) at (2i + 1, 2j + 1)
    ref, S, plain = R.evaluate(R.upsample2, dZ)
    assert torch.equal(plain["Up"].double(), ref["Up"]) and passes(st(plain), ref, S, plain, storage)
    shifted = torch.zeros_like(plain["Up"])
    shifted[:, 2:-1, 2:-1] = plain["Up"][:, 1:-2, 1:-2]
    assert not passes(st({"Up": shifted}), ref, S, plain, storage)
