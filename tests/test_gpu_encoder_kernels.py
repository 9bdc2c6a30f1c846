"""Kernel-level parity tests of the piece encoder's training primitives (da_enc_*, da_gemm_tn_*, da_colsum_f32 through the
C ABI, and the compositions of diffassemble_amd/encoder_train.py), fp32 and bf16 storage, at the network's real shapes.

Every primitive is a deterministic function of its operands (include/diffassemble_hip.h, "Training path of the 2D piece
encoder"), so unlike the end-to-end tests of tests/test_gpu_encoder_train.py nothing here differentiates through a ReLU
decision: each kernel is held against its contract in fp64 on the STORED operands (tests/golden/encoder_kernel_refs.py,
pinned by tests/test_encoder_kernel_refs.py) under the rule

    |got_i - ref_i| <= u_out |ref_i| + 16 e_acc(plain) S_i          for every element i of every output,

u_out = 2^-8 (bf16 maps) / 2^-24 (fp32), S_i the contract's condition term, e_acc(plain) the accumulation error of the same
contract evaluated by torch in fp32 on the CPU, computed per case.  No element is left out; halo cells have S_i = 0 and
must be exactly zero; kernels that only move values are compared exactly.  fp32 outputs also keep the older bound max-abs
error / max-abs reference < 1e-5.  Every case prints e(HIP) and e_acc(plain) (run with -s).
"""
import math

import pytest
import torch

import encoder_kernel_refs as R
from diffassemble_amd import encoder_train as ET
from oracle import encoder as OE
from oracle import weights as W

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PRECS = ["fp32", "bf16"]
STORAGE = {"fp32": F32, "bf16": BF16}
UNITS = ET._units()
CONV_UNITS = UNITS[1:]
UNIT_IDS = [u[0] for u in CONV_UNITS]
BN_SHAPES = [(32, 128), (16, 256), (8, 256), (4, 512)]
# pieces per output resolution: M = B Ho^2 is not a multiple of 128 where the shape allows (Ho = 4: B % 8 != 0, Ho = 8: B odd)
# and the number of 128-pixel tiles is not a multiple of 8 (Ho = 32 has 8 B tiles whatever B)
B_FOR = {32: 2, 16: 3, 8: 5, 4: 9}
RES_MODES = ("none", "separate", "inplace")


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


@pytest.fixture(scope="module")
def engines(dev):
    """One EncoderTrainEngine per precision on the synthetic weights: its tables, packers, _conv and _wgrad are the code under test."""
    from diffassemble_amd.model.backbones.resnet_equivariant import ResNet18
    out = {}
    for prec in PRECS:
        net = ResNet18(precision=prec)
        net.load_state_dict(W.make_encoder_state(3))
        out[prec] = ET.EncoderTrainEngine(net.to(dev).train(), dev, precision=prec)
    return out


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def prec_id(lib, prec):
    return lib.PREC_BF16 if prec == "bf16" else lib.PREC_F32


def filled_map(dev, storage, B, H, C, value=7.0):
    """a destination map: interior pre-filled (a kernel that skips a pixel shows), zero halo"""
    m = torch.zeros(B, H + 2, H + 2, C, dtype=storage, device=dev)
    m[:, 1:-1, 1:-1] = value
    return m


def check(tag, got, ref, S, plain, outs):
    """Judge the outputs named in ``outs`` (name -> stored dtype) by the rule; print the figures; assert at the end."""
    fails = []
    for k, dt in outs.items():
        j = R.judge(got[k], ref[k], S[k], plain[k], dt)
        line = f"[enc-kernels] {tag} {k}: e(HIP) {j['e_hip']:.3e}  e_acc(plain) {j['e_acc']:.3e}  over the bound {j['bad']}/{j['n']}"
        if dt == F32:
            rm = R.rel_max(got[k], ref[k])
            line += f"  max-abs rel {rm:.2e}"
            if not rm < 1e-5:
                fails.append((k, "max-abs rel", rm))
        print(line)
        if not j["ok"]:
            fails.append((k, j))
        if ref[k].dim() == 4 and not R.halo_is_zero(got[k]):
            fails.append((k, "halo written"))
    assert not fails, (tag, fails)


# ------------------------------------------------------------------------------------------------ da_enc_conv
def conv_operands(unit, storage, B, seed, dgrad=False):
    """stored operands of one unit on the CPU: forward X [B][H+2][H+2][Cin4] -> [B][Ho+2][Ho+2][Cout4]; for the dgrad the
    map that enters is dY at the output resolution."""
    _, _, cin, planes, k, stride, H = unit
    g = gen(seed)
    w = randn(g, planes, cin, 4, k, k) / math.sqrt(cin * 4 * k * k)
    bank = OE.p4_filter_bank(w).to(storage)
    Ho = H // stride
    if dgrad:
        src = R.halo(randn(g, B, planes * 4, Ho, Ho)).to(storage)
        res = R.halo(randn(g, B, cin * 4, H, H)).to(storage)
    else:
        src = R.halo(randn(g, B, cin * 4, H, H)).to(storage)
        res = R.halo(randn(g, B, planes * 4, Ho, Ho)).to(storage)
    bias = randn(g, planes * 4)
    return bank, src, res, bias


def run_conv(lib, dev, prec, X, Wp, bias, res_mode, res, cout4, k, stride, relu):
    """da_enc_conv on device copies; -> Y (a fresh pre-filled map, or the residual's own buffer for "inplace")"""
    L = lib.lib()
    B, Hi, cin4 = X.shape[0], X.shape[1] - 2, X.shape[3]
    Ho = Hi // stride
    if res_mode == "inplace":
        Y = res.clone()
        r = Y
    else:
        Y = filled_map(dev, X.dtype, B, Ho, cout4)
        r = res if res_mode == "separate" else None
    lib.check(L.da_enc_conv(prec_id(lib, prec), B, lib.ptr(X), cin4, Hi, lib.ptr(Wp), lib.ptr(bias), lib.ptr(r), lib.ptr(Y), cout4, k,
                            stride, relu, lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    return Y


def conv_forward_case(lib, dev, prec, unit, B, relu, res_mode, seed, tag):
    storage = STORAGE[prec]
    _, _, cin, planes, k, stride, H = unit
    bank, X, res, bias = conv_operands(unit, storage, B, seed)
    Wp = R.pack_fwd(bank)
    Y = run_conv(lib, dev, prec, X.to(dev), Wp.to(dev), bias.to(dev), res_mode, res.to(dev), planes * 4, k, stride, relu)
    ref, S, plain = R.evaluate(R.conv, X, Wp, bias, None if res_mode == "none" else res, relu=relu, k=k, stride=stride)
    check(f"{tag}[{prec}] relu={relu} res={res_mode} B={B}", {"Y": Y}, ref, S, plain, {"Y": storage})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ui", range(len(CONV_UNITS)), ids=UNIT_IDS)
def test_conv_forward(dev, lib, ui, prec):
    """da_enc_conv with the forward packing at every conv unit's shape, bias != 0; relu = ui % 2 and the residual form
    (NULL / a separate map / res == Y) = ui % 3 run through all six combinations over the 19 units.
    Measured: e(HIP) <= 1.1 e_acc(plain) in both precisions.  The bf16 cases with a residual caught the tile being staged in
    bf16 before the residual was added (two roundings: e(HIP) 3e-4 .. 1e-3 against e_acc 1.5e-7, 5 - 15 % of the elements over
    the bound); k_conv_mfma<bf16> now stages such a tile in fp32 and rounds once."""
    unit = CONV_UNITS[ui]
    Ho = unit[6] // unit[5]
    B = B_FOR[Ho]
    nrt = -(-B * Ho * Ho // 128)
    assert Ho == 32 or nrt % 8 != 0
    assert Ho >= 16 or (B * Ho * Ho) % 128 != 0
    conv_forward_case(lib, dev, prec, unit, B, ui % 2, RES_MODES[ui % 3], 100 + ui, f"conv-fwd {unit[0]}")


@pytest.mark.parametrize("prec", PRECS)
def test_conv_single_tile(dev, lib, prec):
    """M = 16 output pixels: one ragged tile, 112 of its 128 rows clamped"""
    unit = next(u for u in CONV_UNITS if u[0] == "layer4.1.conv1")
    for relu, mode in ((1, "separate"), (0, "none")):
        conv_forward_case(lib, dev, prec, unit, 1, relu, mode, 50, "conv-single-tile")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ui", range(len(CONV_UNITS)), ids=UNIT_IDS)
def test_conv_dgrad(dev, lib, ui, prec):
    """The input gradient as the engine forms it: da_enc_conv on dY with _pack_dgrad's bank (a stride-2 unit through
    da_enc_upsample2 first), zero bias, no ReLU; the residual form (accumulation of other gradient paths) = ui % 3."""
    storage = STORAGE[prec]
    L = lib.lib()
    _, _, cin, planes, k, stride, H = unit = CONV_UNITS[ui]
    B, mode = B_FOR[H], RES_MODES[ui % 3]
    bank, dY, res, _ = conv_operands(unit, storage, B, 200 + ui, dgrad=True)
    src = dY.to(dev)
    if stride == 2:
        up = filled_map(dev, storage, B, H, planes * 4)
        lib.check(L.da_enc_upsample2(prec_id(lib, prec), B, H // 2, planes * 4, lib.ptr(src), lib.ptr(up), lib.stream_ptr(dev)))
        src = up
    zero = torch.zeros(512, device=dev)
    dX = run_conv(lib, dev, prec, src, R.pack_dgrad(bank).to(dev), zero, mode, res.to(dev), cin * 4, k, 1, 0)
    ref, S, plain = R.evaluate(R.dgrad, dY, bank, None if mode == "none" else res, k=k, stride=stride)
    check(f"conv-dgrad {unit[0]}[{prec}] res={mode} B={B}", {"Y": dX}, ref, S, plain, {"Y": storage})


def xcd_sample(B, HH):
    """first and last piece, and the pieces on either side of each XCD's tile-range boundary (pixel tile k * nrt8)"""
    M = B * HH
    nrt8 = (-(-M // 128) + 7) // 8
    s = {0, B - 1}
    for k in range(1, 8):
        p = k * nrt8 * 128
        if p < M:
            s |= {(p - 1) // HH, p // HH}
    return sorted(s)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,B,relu,mode,chunk", [("layer1.0.conv1", 130, 1, "separate", 7), ("layer2.0.conv2", 259, 0, "inplace", 9),
                                                     ("layer4.0.conv2", 2051, 1, "none", 67)],
                         ids=["cout128-h32-B130", "cout256-h16-B259", "cout512-h4-B2051"])
def test_conv_persistent_walk(dev, lib, name, B, relu, mode, chunk, prec):
    """Workgroups that walk at least three virtual tiles (nvirt > 2 grid; the grid is capped at 512) for each channel-tile
    count nct = Cout4 / 128 in {1, 2, 4}: the fp64 rule on a fixed sample of pieces (first, last, both sides of every XCD's
    tile-range boundary) and bit-equality of ALL pieces with runs of the same pieces in small batches (pieces are independent)."""
    storage = STORAGE[prec]
    _, _, cin, planes, k, stride, H = unit = next(u for u in CONV_UNITS if u[0] == name)
    assert stride == 1
    nct = planes * 4 // 128
    nrt8 = (-(-B * H * H // 128) + 7) // 8
    grid = max(512 // (8 * nct) * (8 * nct), 8 * nct)
    assert 8 * nrt8 * nct > 2 * grid, "workgroups must get a third tile"
    g = torch.Generator(device=dev).manual_seed(B)
    w = randn(gen(B), planes, cin, 4, k, k) / math.sqrt(cin * 4 * k * k)
    bank = OE.p4_filter_bank(w).to(storage)
    Wp, bias = R.pack_fwd(bank), randn(gen(B + 1), planes * 4)

    def rand_map(C):
        m = torch.zeros(B, H + 2, H + 2, C, dtype=storage, device=dev)
        m[:, 1:-1, 1:-1] = torch.randn(B, H, H, C, generator=g, device=dev).to(storage)
        return m
    X, res = rand_map(cin * 4), rand_map(planes * 4)
    Wd, bd = Wp.to(dev), bias.to(dev)
    Y = run_conv(lib, dev, prec, X, Wd, bd, mode, res, planes * 4, k, 1, relu)
    assert R.halo_is_zero(Y)
    pieces = xcd_sample(B, H * H)
    idx = torch.tensor(pieces, device=dev)
    r_cpu = None if mode == "none" else res[idx].cpu()
    ref, S, plain = R.evaluate(R.conv, X[idx].cpu(), Wp, bias, r_cpu, relu=relu, k=k, stride=1)
    check(f"conv-persistent {name}[{prec}] relu={relu} res={mode} B={B} pieces={pieces}", {"Y": Y[idx]}, ref, S, plain, {"Y": storage})
    for i in range(0, B, chunk):
        j = min(B, i + chunk)
        Ys = run_conv(lib, dev, prec, X[i:j].contiguous(), Wd, bd, mode, res[i:j].contiguous(), planes * 4, k, 1, relu)
        assert torch.equal(Ys, Y[i:j]), f"pieces {i}..{j} differ from their small-batch run"


def test_engine_conv_slicing(dev, lib, engines):
    """EncoderTrainEngine._conv keeps a map below the kernel's 4 GB limit by slicing the batch: fp32, H = 32, C4 = 128 takes
    7 256 pieces per slice, so B = 7 258 runs two slices.  No error, and the pieces at the seam are bit-equal to a B = 4 run."""
    eng = engines["fp32"]
    B, H, C = 7258, 32, 128
    per = 4 * (H + 2) * (H + 2) * C
    assert ((1 << 32) - 1) // per == 7256
    X = torch.empty(B, H + 2, H + 2, C, device=dev)
    X.normal_(generator=torch.Generator(device=dev).manual_seed(5))
    X[:, 0] = 0; X[:, -1] = 0; X[:, :, 0] = 0; X[:, :, -1] = 0          # noqa: E702
    Y = torch.zeros_like(X)
    Wp = (torch.randn(C, 9 * C, generator=torch.Generator(device=dev).manual_seed(6), device=dev) / 34.0).contiguous()
    eng._conv(X, C, H, Wp, Y, C, 3, 1)
    torch.cuda.synchronize()
    idx = torch.tensor([0, 7255, 7256, 7257], device=dev)
    X4, Y4 = X[idx].contiguous(), torch.zeros(4, H + 2, H + 2, C, device=dev)
    eng._conv(X4, C, H, Wp, Y4, C, 3, 1)
    torch.cuda.synchronize()
    assert torch.equal(Y[idx], Y4) and float(Y4.abs().max()) > 0 and R.halo_is_zero(Y4)
    del X, Y


# ------------------------------------------------------------------------------------------------ stem
def patches(g, B):
    p = torch.rand(B, 3, 32, 32, generator=g, dtype=F32)
    p[:, :, 0, :5] = 0.0                                 # exact 0 and 1, at the crop's border and inside
    p[:, :, 31, 27:] = 1.0
    p[:, 1, 10:12, 10:12] = 0.0
    p[:, 2, 20:22, 5:7] = 1.0
    return p


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 5, 130])
def test_stem_and_im2col(dev, lib, B, prec):
    storage, L, st = STORAGE[prec], lib.lib(), lib.stream_ptr(dev)
    g = gen(B)
    P, w, bias = patches(g, B), randn(g, 128, 27) * 0.2, randn(g, 128)
    Pd, wd, bd = P.to(dev), w.to(dev), bias.to(dev)
    for relu in (0, 1):
        Y = filled_map(dev, storage, B, 32, 128)
        lib.check(L.da_enc_stem(prec_id(lib, prec), B, lib.ptr(Pd), lib.ptr(wd), lib.ptr(bd), lib.ptr(Y), relu, st))
        ref, S, plain = R.evaluate(R.stem, P, w, bias, relu=relu)
        check(f"stem[{prec}] relu={relu} B={B}", {"Y": Y}, ref, S, plain, {"Y": storage})
    cols = torch.full((B, 34, 34, 32), 3.0, dtype=storage, device=dev)          # the kernel writes every cell, halo included
    lib.check(L.da_enc_stem_im2col(prec_id(lib, prec), B, lib.ptr(Pd), lib.ptr(cols), st))
    ref, S, plain = R.evaluate(R.stem_im2col, P)
    assert R.halo_is_zero(cols) and float(cols[..., 27:].float().abs().max()) == 0
    if prec == "fp32":
        assert torch.equal(cols.cpu(), plain["cols"]), "fp32 im2col only moves normalised values: exact"
    check(f"stem-im2col[{prec}] B={B}", {"cols": cols}, ref, S, plain, {"cols": storage})


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_batches(H):
    """B with nblk = 1 (one piece; several pieces), 2 and >= 5 with a ragged last block of BN_PIX = 4096 pixels"""
    per = H * H
    one, two, five = max(3, 3072 // per // 2 * 2 + 1), 4096 // per + 1, 4 * 4096 // per + 5
    out = [1, one, two, five]
    nblk = [-(-b * per // 4096) for b in out]
    assert nblk[:3] == [1, 1, 2] and nblk[3] >= 5 and (out[3] * per) % 4096 != 0, (out, nblk)
    return out


BN_CASES = [(H, C4, B) for H, C4 in BN_SHAPES for B in bn_batches(H)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,C4,B", BN_CASES, ids=[f"h{h}-c{c}-B{b}" for h, c, b in BN_CASES])
def test_batchnorm_kernels(dev, lib, H, C4, B, prec):
    """da_enc_bn_stats / _apply / _backward on the operands each receives (the apply and the backward take the mean and
    variance the statistics kernel produced; the backward takes the Z the apply stored, so no ReLU decision can flip).
    Data: every plane offset by 4 standard deviations (|mean| / std = 4: the next power of two above the largest ratio, 2.44,
    over the 20 BatchNorm inputs of the fp64 oracle's training forward on the fixtures' inputs), all four (relu, res)
    combinations; and zero-mean data once.  dgamma / dbeta are pre-filled: the contract is +=.
    Measured: e(HIP) <= 10 e_acc(plain) (dgamma, whose plain sum is pairwise: e_acc 5e-10).  The offset planes caught the
    variance, E[y^2] - m^2 over fp32 per-thread sums: off by up to 3.2e-5 of the variance (39 e_acc, and over the 1e-5 bound in
    17 of these 32 cases); k_enc_bn_stats now keeps its per-thread sums in double and is exact to the output's rounding."""
    storage, L, st, P = STORAGE[prec], lib.lib(), lib.stream_ptr(dev), prec_id(lib, prec)
    planes = C4 // 4
    g = gen(1000 * H + B)
    sigma = (torch.rand(planes, generator=g) * 1.5 + 0.5).repeat_interleave(4).view(1, -1, 1, 1)
    sign = (torch.randint(0, 2, (planes,), generator=g) * 2.0 - 1.0).repeat_interleave(4).view(1, -1, 1, 1)
    noise = randn(g, B, C4, H, H)
    gamma, beta = torch.rand(planes, generator=g) + 0.5, randn(g, planes)
    res, dZ = R.halo(randn(g, B, C4, H, H)).to(storage), R.halo(randn(g, B, C4, H, H)).to(storage)
    scratch = torch.empty(L.da_enc_train_scratch_bytes(B), dtype=torch.uint8, device=dev)
    gd, bd, rd, dZd = gamma.to(dev), beta.to(dev), res.to(dev), dZ.to(dev)
    for offset, relu, with_res in ((4.0, 0, 0), (4.0, 0, 1), (4.0, 1, 0), (4.0, 1, 1), (0.0, 1, 1)):
        tag = f"[{prec}] h{H} c{C4} B={B} offset={offset:g} relu={relu} res={with_res}"
        Y = R.halo(noise * sigma + offset * sigma * sign).to(storage)
        Yd = Y.to(dev)
        mean, var = torch.full((planes,), 9.0, device=dev), torch.full((planes,), 9.0, device=dev)
        lib.check(L.da_enc_bn_stats(P, B, H, C4, lib.ptr(Yd), lib.ptr(mean), lib.ptr(var), lib.ptr(scratch), st))
        ref, S, plain = R.evaluate(R.bn_stats, Y)
        check("bn-stats" + tag, {"mean": mean, "var": var}, ref, S, plain, {"mean": F32, "var": F32})
        Z = filled_map(dev, storage, B, H, C4)
        lib.check(L.da_enc_bn_apply(P, B, H, C4, lib.ptr(Yd), lib.ptr(mean), lib.ptr(var), lib.ptr(gd), lib.ptr(bd),
                                    lib.ptr(rd if with_res else None), relu, lib.ptr(Z), st))
        mc, vc = mean.cpu(), var.cpu()
        ref, S, plain = R.evaluate(R.bn_apply, Y, mc, vc, gamma, beta, res if with_res else None, relu=relu)
        check("bn-apply" + tag, {"Z": Z}, ref, S, plain, {"Z": storage})
        dg0, db0 = randn(g, planes), randn(g, planes)
        dg, db = dg0.to(dev), db0.to(dev)
        dY = filled_map(dev, storage, B, H, C4)
        dR = filled_map(dev, storage, B, H, C4) if with_res else None
        lib.check(L.da_enc_bn_backward(P, B, H, C4, lib.ptr(dZd), lib.ptr(Z), lib.ptr(Yd), lib.ptr(mean), lib.ptr(var), lib.ptr(gd), relu,
                                       lib.ptr(dg), lib.ptr(db), lib.ptr(dY), lib.ptr(dR), lib.ptr(scratch), st))
        ref, S, plain = R.evaluate(R.bn_backward, dZ, Z.cpu(), Y, mc, vc, gamma, dg0, db0, relu=relu, want_dres=bool(with_res))
        outs = {"dgamma": F32, "dbeta": F32, "dY": storage}
        got = {"dgamma": dg, "dbeta": db, "dY": dY}
        if with_res:
            outs["dRes"], got["dRes"] = storage, dR
            assert torch.equal(dR.cpu().double(), ref["dRes"]), "dRes only moves (masked) values: exact"
        check("bn-backward" + tag, got, ref, S, plain, outs)


# ------------------------------------------------------------------------------------------------ da_enc_upsample2
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,C4", [(16, 256), (8, 256), (4, 512)], ids=["h16-c256", "h8-c256", "h4-c512"])
def test_upsample2(dev, lib, H, C4, prec):
    """the three (H, C4) of the engine's zero-stuffed maps; destination interior pre-filled, halo zero; exact"""
    storage, L = STORAGE[prec], lib.lib()
    for B in (1, 5):
        s = R.halo(randn(gen(H + B), B, C4, H, H)).to(storage)
        up = filled_map(dev, storage, B, 2 * H, C4)
        lib.check(L.da_enc_upsample2(prec_id(lib, prec), B, H, C4, lib.ptr(s.to(dev)), lib.ptr(up), lib.stream_ptr(dev)))
        ref = R.upsample2(s)["Up"]
        assert torch.equal(up.cpu(), ref), (H, C4, B)
        assert R.halo_is_zero(up) and int((up != 0).sum()) == int((s != 0).sum())


# ------------------------------------------------------------------------------------------------ TN GEMMs
PART_CAP = 16 << 20


def tn_splits(kind, M, N, K):
    """the row-split count of launch_gemm_tn / launch_gemm_tn_bf16 (da_train_gemm.hip) and what set it"""
    tile, rows, chunk = (64, 256, 16) if kind == "f32" else (128, 512, 32)
    cands = {"tiles": 2048 // (-(-N // tile) * -(-K // tile)), "rows": -(-M // rows), "cap": PART_CAP // (N * K)}
    regime = min(cands, key=lambda r: (cands[r], r))
    splits = max(1, cands[regime])
    Mc = -(-(-(-M // splits)) // chunk) * chunk
    splits = -(-M // Mc)
    return splits, ("one" if splits == 1 else regime), Mc


# (name, M, N, K, lda, ldb, ldc, regime of da_gemm_tn_f32, regime of da_gemm_tn_bf16).  The fp32 kernel's split count is never
# set by the scratch cap (2048 / (tn tk) <= 8 M / (N K) < 16 M / (N K) floats); the bf16 kernel's is set by 2048 / (tn tk)
# only for ragged tiles (for full 128 x 128 tiles the cap is half of it), hence the 160 x 136 case.
TN_CASES = [
    ("one-split-256x128", 200, 256, 128, 264, 136, 131, "one", "one"),
    ("rows-128x128", 5003, 128, 128, 136, 136, 131, "rows", "rows"),
    ("rows-256x256", 2318, 256, 256, 264, 264, 259, "rows", "rows"),
    ("rows-512x256", 1301, 512, 256, 520, 264, 259, "rows", "rows"),
    ("tiles-512x512", 9001, 512, 512, 520, 520, 515, "tiles", "rows"),
    ("cap-512x512", 40003, 512, 512, 512, 512, 512, "tiles", "cap"),
    ("stem-128x27", 2305, 128, 27, 128, 32, 27, "rows", "rows"),
    ("head1-544x25600", 37, 544, 25600, 1152, 25600, 25600, "one", "one"),
    ("head2-544x18432", 37, 544, 18432, 1152, 18432, 18432, "one", "one"),
    ("tiles-160x136", 270001, 160, 136, 168, 136, 139, "tiles", "tiles"),
    ("haloed-512-pieces-128x128", 512 * 34 * 34 - 70, 128, 128, 128, 128, 128, "tiles", "cap"),
]


@pytest.mark.parametrize("case", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_gemm_tn(dev, lib, case):
    """da_gemm_tn_f32 and da_gemm_tn_bf16, C pre-filled (the contract is +=) and the cells of C beyond K untouched, in every
    regime of the row split; M is never a multiple of the 16- (fp32) / 32-row (bf16) chunk rounding.  The two largest cases
    give both kernels the same bf16-representable operands, so one CPU reference serves both."""
    name, M, N, K, lda, ldb, ldc, reg32, reg16 = case
    L, st = lib.lib(), lib.stream_ptr(dev)
    assert M % 16 != 0
    scratch = torch.empty(PART_CAP, device=dev)
    g = torch.Generator(device=dev).manual_seed(M)
    shared = M > 100000
    A32 = torch.randn(M, lda, generator=g, device=dev)
    B32 = torch.randn(M, ldb, generator=g, device=dev)
    C0 = torch.randn(N, ldc, generator=g, device=dev)
    A16, B16 = A32.to(BF16), B32.to(BF16)
    if shared:
        A32, B32 = A16.float(), B16.float()
    evals = {}
    for kind, fn, A, B, want in (("f32", L.da_gemm_tn_f32, A32, B32, reg32), ("bf16", L.da_gemm_tn_bf16, A16, B16, reg16)):
        splits, regime, Mc = tn_splits(kind, M, N, K)
        assert regime == want and M % Mc != 0, (kind, splits, regime, Mc)
        C = C0.clone()
        lib.check(fn(M, N, K, lib.ptr(A), lda, lib.ptr(B), ldb, lib.ptr(C), ldc, lib.ptr(scratch), st))
        torch.cuda.synchronize()
        key = "shared" if shared else kind
        if key not in evals:
            evals[key] = R.evaluate(R.gemm_tn, A[:, :N].cpu(), B[:, :K].cpu(), C0[:, :K].cpu())
        ref, S, plain = evals[key]
        assert torch.equal(C[:, K:], C0[:, K:]), "cells of C beyond K were written"
        check(f"gemm-tn-{kind} {name} M={M} splits={splits} ({regime})", {"C": C[:, :K]}, ref, S, plain, {"C": F32})


# ------------------------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("M", [1, 127, 128, 129, 1000])
def test_colsum(dev, lib, M):
    L, N, lda = lib.lib(), 544, 1088
    g = gen(M)
    A, out0 = randn(g, M, lda), randn(g, N)
    out = out0.to(dev)
    scratch = torch.empty(-(-M // 128) * N + 64, device=dev)
    lib.check(L.da_colsum_f32(M, N, lib.ptr(A.to(dev)), lda, lib.ptr(out), lib.ptr(scratch), lib.stream_ptr(dev)))
    ref, S, plain = R.evaluate(R.colsum, A[:, :N], out0)
    check(f"colsum M={M}", {"out": out}, ref, S, plain, {"out": F32})


@pytest.mark.parametrize("name", ["layer1.0.conv1", "layer2.0.shortcut.0", "conv1"])
def test_bank_grad(dev, lib, engines, name):
    """da_enc_bank_grad with the engine's own tables (a 3x3 unit, a 1x1 shortcut, the stem), dW pre-filled; the table itself
    is held against autograd through the oracle's filter bank."""
    eng, L = engines["fp32"], lib.lib()
    _, _, cin, planes, k, _, _ = next(u for u in UNITS if u[0] == name)
    w = eng.params[name + ".weight"]
    table = eng._tables[name]
    g = gen(len(name))
    I4 = 3 if cin is None else cin * 4
    dbank = randn(g, planes * 4, k * k * I4)
    dW0 = randn(g, w.numel())
    dW = dW0.to(dev)
    lib.check(L.da_enc_bank_grad(w.numel(), lib.ptr(table), lib.ptr(dbank.to(dev)), lib.ptr(dW), lib.stream_ptr(dev)))
    ref, S, plain = R.evaluate(R.bank_grad, dbank, dW0, table=table.cpu())
    check(f"bank-grad {name}", {"dW": dW}, ref, S, plain, {"dW": F32})
    d4 = dbank.double().view(planes * 4, 3, 3, 3) if cin is None else dbank.double().view(planes * 4, k, k, I4).permute(0, 3, 1, 2)
    gathered = dW0.double() + R._gather_bank(d4, w.shape).reshape(-1)
    assert float((ref["dW"] - gathered).abs().max()) <= 1e-12 * float(gathered.abs().max())


# ------------------------------------------------------------------------------------------------ engine compositions
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ui", range(len(CONV_UNITS)), ids=UNIT_IDS)
def test_engine_wgrad(dev, lib, engines, ui, prec):
    """EncoderTrainEngine._wgrad (nine shifted TN GEMMs over the haloed maps + the bank gather; a stride-2 unit on the
    zero-stuffed dY) at every unit's real channel counts, the parameter's gradient pre-filled, against the fp64 contract
    (= autograd of F.conv2d(x, p4_filter_bank(w)) on the stored operands, tests/test_encoder_kernel_refs.py)."""
    storage, L, eng = STORAGE[prec], lib.lib(), engines[prec]
    name, _, cin, planes, k, stride, H = unit = CONV_UNITS[ui]
    B = B_FOR[H]
    g = gen(300 + ui)
    X = R.halo(randn(g, B, cin * 4, H, H)).to(storage)
    dY = R.halo(randn(g, B, planes * 4, H // stride, H // stride)).to(storage)
    dW0 = randn(g, planes, cin, 4, k, k)
    src = dY.to(dev)
    if stride == 2:
        up = filled_map(dev, storage, B, H, planes * 4)
        lib.check(L.da_enc_upsample2(prec_id(lib, prec), B, H // 2, planes * 4, lib.ptr(src), lib.ptr(up), lib.stream_ptr(dev)))
        src = up
    eng._n = B
    grad = eng._grad(name + ".weight")
    grad.copy_(dW0.to(dev))
    eng._wgrad(name, src, X.to(dev), cin * 4, planes * 4, k, H)
    torch.cuda.synchronize()
    ref, S, plain = R.evaluate(R.wgrad, dY, X, dW0, k=k, stride=stride)
    check(f"engine-wgrad {name}[{prec}] B={B}", {"dW": grad}, ref, S, plain, {"dW": F32})
    assert eng.params[name + ".weight"].grad.data_ptr() == grad.data_ptr()


@pytest.mark.parametrize("prec", PRECS)
def test_stem_wgrad(dev, lib, engines, prec):
    """The stem's parameter gradient as EncoderTrainEngine.backward forms it: im2col of the crops, one TN GEMM over the
    haloed rows (K = 27, ldb = 32), the bank gather with the stem's table."""
    storage, L, eng, st = STORAGE[prec], lib.lib(), engines[prec], lib.stream_ptr(dev)
    B = 3
    g = gen(77)
    P, dY, dW0 = patches(g, B), R.halo(randn(g, B, 128, 32, 32)).to(storage), randn(g, 32, 3, 1, 3, 3)
    cols = torch.zeros(B, 34, 34, 32, dtype=storage, device=dev)
    lib.check(L.da_enc_stem_im2col(prec_id(lib, prec), B, lib.ptr(P.to(dev)), lib.ptr(cols), st))
    dbank = torch.zeros(128, 27, device=dev)
    eng._gemm_tn(B * 34 * 34, 128, 27, dY.to(dev), 128, cols, 32, dbank, 27)
    dW = dW0.to(dev)
    lib.check(L.da_enc_bank_grad(dW.numel(), lib.ptr(eng._tables["conv1"]), lib.ptr(dbank), lib.ptr(dW), st))
    # the contract on the operands the GEMM read: the stored im2col values
    c = cols.cpu()

    def contract(dY, c, dW0, cond=False):
        run = lambda a, c, d: d + R._gather_bank((a.reshape(-1, 128).t() @ c.reshape(-1, 32)[:, :27]).view(128, 3, 3, 3), d.shape)  # noqa: E731
        out = {"dW": run(dY, c, dW0)}
        return (out, {"dW": run(dY.abs(), c.abs(), dW0.abs())}) if cond else out
    ref, S, plain = R.evaluate(contract, dY, c, dW0)
    check(f"stem-wgrad[{prec}] B={B}", {"dW": dW}, ref, S, plain, {"dW": F32})
    if prec == "fp32":                                   # and from the crops themselves
        full = R.stem_wgrad(dY.double(), P.double(), dW0.double())["dW"]
        assert R.rel_max(dW, full) < 1e-5
