"""Contract of the EfficientNet-B0 piece encoder (include/diffassemble_hip.h, "EfficientNet-B0 piece encoder";
diffassemble_amd/csrc/da_efficientnet.hip): the eval feature forward of timm's ``efficientnet_b0`` under ``features_only=True`` on a
timm-keyed state dict, restated with plain ``torch.nn.functional`` calls in NCHW and in the dtype of its operands (the tests pass
fp64) -- stem, blocks.0 .. blocks.4, the eleven block outputs and the row [map 2 | map 3] that ``Eff_GAT.visual_features`` keeps.
The table of widths, kernels, strides and squeeze widths is written from timm's published architecture; neither timm nor a checkpoint
of it is available to hold this file against.  tests/test_efficientnet_host.py holds the module's keys and the host packing against
it, tests/test_gpu_efficientnet.py the HIP kernels.

Also here: the generators of weights and crops (numpy ``default_rng`` seeds; tests/golden/efficientnet_v1.npz stores SHA-256 digests
of what they must produce, not the 3.6 M weights), and a small NHWC evaluator of the PACKED weights (the arithmetic of the kernels,
in fp64) for the host test of fold, padding, flatten order and the quarter-turn index map."""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
WEIGHT_SEED = 20260
F32 = np.float32
MEAN, STD = (0.4850, 0.4560, 0.4060), (0.2290, 0.2240, 0.2250)      # the ``mean`` / ``std`` buffers of Eff_GAT (fp32 values)
# timm's efficientnet_b0: (blocks, depthwise kernel, stride, expansion, out channels) per stage; squeeze width = block input / 4
STAGES = ((1, 3, 1, 1, 16), (2, 3, 2, 6, 24), (2, 5, 2, 6, 40), (3, 3, 2, 6, 80), (3, 5, 1, 6, 112), (4, 5, 2, 6, 192), (1, 3, 1, 6, 320))
LIVE_STAGES = 5                                                      # blocks.0 .. blocks.4 are read
MAP2, MAP3 = "blocks.2.1", "blocks.4.2"
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def blocks():
    """[(prefix, in, mid, out, kernel, stride, squeeze width, depthwise-separable)] of all 16 blocks in timm's order."""
    out, cin = [], 32
    for s, (n, k, stride, e, cout) in enumerate(STAGES):
        for b in range(n):
            out.append((f"blocks.{s}.{b}", cin, cin * e, cout, k, stride if b == 0 else 1, cin // 4, e == 1))
            cin = cout
    return out


def live_blocks():
    return [b for b in blocks() if int(b[0].split(".")[1]) < LIVE_STAGES]


def key_shapes():
    """[(key, shape)] of the state dict in timm's registration order."""
    out = [("conv_stem.weight", (32, 3, 3, 3))]

    def bn(name, c):
        out.extend((f"{name}.{k}", () if k == "num_batches_tracked" else (c,)) for k in BN_KEYS)

    def se(p, c, r):
        out.extend([(f"{p}.se.conv_reduce.weight", (r, c, 1, 1)), (f"{p}.se.conv_reduce.bias", (r,)),
                    (f"{p}.se.conv_expand.weight", (c, r, 1, 1)), (f"{p}.se.conv_expand.bias", (c,))])

    bn("bn1", 32)
    for p, cin, mid, cout, k, s, r, ds in blocks():
        if ds:
            out.append((f"{p}.conv_dw.weight", (cin, 1, k, k)))
            bn(f"{p}.bn1", cin)
            se(p, cin, r)
            out.append((f"{p}.conv_pw.weight", (cout, cin, 1, 1)))
            bn(f"{p}.bn2", cout)
        else:
            out.append((f"{p}.conv_pw.weight", (mid, cin, 1, 1)))
            bn(f"{p}.bn1", mid)
            out.append((f"{p}.conv_dw.weight", (mid, 1, k, k)))
            bn(f"{p}.bn2", mid)
            se(p, mid, r)
            out.append((f"{p}.conv_pwl.weight", (cout, mid, 1, 1)))
            bn(f"{p}.bn3", cout)
    return out


# ------------------------------------------------------------------------------------------------------ generators
def make_weights(seed=WEIGHT_SEED):
    """The state dict as numpy arrays in key order: He-scaled Gaussian convolutions (std sqrt(2 / fan_in), fan_in = k k in /
    groups, which keeps the activations' scale through the SiLU layers; the linear projections sqrt(1 / fan_in)), BatchNorm
    statistics and affine parameters that leave nothing trivial (running mean 0.3 randn, running var in [0.25, 1.75], |gamma| in
    [0.5, 1.5] with about a quarter negative, beta 0.3 randn), squeeze-excite biases 0.3 randn."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in key_shapes():
        leaf = key.rsplit(".", 1)[1]
        if key.endswith("num_batches_tracked"):
            sd[key] = np.array(0, dtype=np.int64)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            linear = key.endswith(("conv_pwl.weight", "blocks.0.0.conv_pw.weight"))
            sd[key] = (np.sqrt((1.0 if linear else 2.0) / fan_in) * rng.standard_normal(shape)).astype(F32)
        elif ".se." in key:
            sd[key] = (0.3 * rng.standard_normal(shape)).astype(F32)
        elif leaf == "weight":
            sign = np.where(rng.random(shape) < 0.25, -1.0, 1.0)
            sd[key] = (sign * (0.5 + rng.random(shape))).astype(F32)
        elif leaf == "running_var":
            sd[key] = (0.25 + 1.5 * rng.random(shape)).astype(F32)
        else:
            sd[key] = (0.3 * rng.standard_normal(shape)).astype(F32)
    return sd


def state(dtype=torch.float32, seed=WEIGHT_SEED):
    return {k: torch.from_numpy(v).to(dtype if v.dtype.kind == "f" else torch.int64) for k, v in make_weights(seed).items()}


def make_crops(N, seed):
    """[N, 3, 32, 32] float32 with values k / 255.  The LAST three crops (as many as fit) are all zeros, all ones and a single bright
    corner pixel; the others are smooth colour ramps plus noise, so neighbouring pixels correlate as in a picture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    out = np.zeros((N, 3, 32, 32), dtype=np.int64)
    for n in range(N):
        a = rng.uniform(-4, 4, (3, 2))
        base = rng.integers(0, 256, (3, 1, 1))
        ramp = base + a[:, :1, None] * yy + a[:, 1:, None] * xx + rng.integers(-40, 41, (3, 32, 32))
        out[n] = np.clip(np.rint(ramp), 0, 255)
    special = [np.zeros((3, 32, 32), np.int64), np.full((3, 32, 32), 255, np.int64), np.zeros((3, 32, 32), np.int64)]
    special[2][:, 0, 31] = 255
    for j, s in enumerate(special[:max(0, min(3, N - 1))]):
        out[N - 1 - j] = s
    return (out.astype(F32) / F32(255.0)).astype(F32)


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------ the contract
def _bn(x, sd, name):
    return F.batch_norm(x, sd[f"{name}.running_mean"], sd[f"{name}.running_var"], sd[f"{name}.weight"], sd[f"{name}.bias"], False, 0.0, EPS)


def _se(x, sd, p):
    s = x.mean((2, 3), keepdim=True)
    s = F.silu(F.conv2d(s, sd[f"{p}.se.conv_reduce.weight"], sd[f"{p}.se.conv_reduce.bias"]))
    return x * torch.sigmoid(F.conv2d(s, sd[f"{p}.se.conv_expand.weight"], sd[f"{p}.se.conv_expand.bias"]))


def forward(sd, crops, quarter_turns=0):
    """crops [N, 3, 32, 32] in [0, 1] -> (taps: the eleven block outputs NCHW, row [N, 1088]).  ``quarter_turns`` r: the crops
    turned clockwise by r quarter turns first."""
    dt = sd["conv_stem.weight"].dtype
    x = torch.rot90(crops.to(dt), -int(quarter_turns), (2, 3))
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dt).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).to(dt).view(1, 3, 1, 1)
    x = (x - mean) / std
    x = F.silu(_bn(F.conv2d(x, sd["conv_stem.weight"], None, 2, 1), sd, "bn1"))
    taps, maps = [], {}
    for p, cin, mid, cout, k, s, r, ds in live_blocks():
        y = x
        if ds:
            y = F.silu(_bn(F.conv2d(y, sd[f"{p}.conv_dw.weight"], None, s, k // 2, 1, cin), sd, f"{p}.bn1"))
            y = _se(y, sd, p)
            y = _bn(F.conv2d(y, sd[f"{p}.conv_pw.weight"]), sd, f"{p}.bn2")
        else:
            y = F.silu(_bn(F.conv2d(y, sd[f"{p}.conv_pw.weight"]), sd, f"{p}.bn1"))
            y = F.silu(_bn(F.conv2d(y, sd[f"{p}.conv_dw.weight"], None, s, k // 2, 1, mid), sd, f"{p}.bn2"))
            y = _se(y, sd, p)
            y = _bn(F.conv2d(y, sd[f"{p}.conv_pwl.weight"]), sd, f"{p}.bn3")
        x = y + x if (s == 1 and cin == cout) else y
        taps.append(x)
        maps[p] = x
    n = crops.shape[0]
    return taps, torch.cat([maps[MAP2].reshape(n, -1), maps[MAP3].reshape(n, -1)], -1)


# ------------------------------------------------------------------------------------------------------ evaluator of the packing
def forward_packed(packed, block_table, turn_source, crops, quarter_turns=0):
    """The kernels' arithmetic on ``efficientnet_encoder.pack``'s output, in its dtype: NHWC maps with padded channel counts, the
    stem gathering the turned crop through ``turn_source``, 1x1 convolutions as row products, depthwise taps with zero padding, the
    gate applied to the projection's operand -> (taps NCHW unpadded, row [N, 1088])."""
    dt = packed["stem_w"].dtype
    n = crops.shape[0]
    si, sj = turn_source(quarter_turns)
    x = crops.to(dt)[:, :, si, sj]
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dt).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).to(dt).view(1, 3, 1, 1)
    x = F.pad((x - mean) / std, (1, 1, 1, 1))
    cols = torch.stack([x[:, c, ky:ky + 32:2, kx:kx + 32:2] for c in range(3) for ky in range(3) for kx in range(3)], -1)   # [n, 16, 16, 27]
    x = F.silu(cols @ packed["stem_w"].t() + packed["stem_b"])                                                                # [n, 16, 16, 32]
    taps, rows = [], {}
    for b, (p, cin, mid, cout, k, s, r, h, skip) in enumerate(block_table):
        y = x
        if packed["exp_w"][b] is not None:
            y = F.silu(y @ packed["exp_w"][b].t() + packed["exp_b"][b])
        ho, pad = h // s, k // 2
        yp = F.pad(y, (0, 0, pad, pad, pad, pad))
        acc = torch.zeros(n, ho, ho, y.shape[-1], dtype=dt)
        for ky in range(k):
            for kx in range(k):
                acc = acc + yp[:, ky:ky + s * ho:s, kx:kx + s * ho:s, :] * packed["dw_w"][b][ky * k + kx]
        y = F.silu(acc + packed["dw_b"][b])
        sq = F.silu(y.mean((1, 2)) @ packed["se_rw"][b].t() + packed["se_rb"][b])
        gate = torch.sigmoid(sq @ packed["se_ew"][b] + packed["se_eb"][b])
        y = (y * gate[:, None, None, :]) @ packed["prj_w"][b].t() + packed["prj_b"][b]
        x = y + x if skip else y
        assert float(x[..., cout:].abs().max() if x.shape[-1] > cout else 0.0) == 0.0, (p, "padding channels must stay zero")
        taps.append(x[..., :cout].permute(0, 3, 1, 2))
        rows[b] = taps[-1].reshape(n, -1)
    return taps, rows
