"""Host side of the EfficientNet-B0 piece encoder (``model="efficientnet_b0"``, the default 2D backbone; what the reference's
puzzle_diff/model/backbones/efficient_gat.py:149-189 keeps of timm's ``efficientnet_b0`` under ``features_only=True``): packs a
timm-keyed state dict into the fp32 tensors ``da_effnet_forward`` reads (include/diffassemble_hip.h) -- every eval BatchNorm folded
into the convolution in front of it in fp64, the 1x1 convolutions as row-major [out][in] matrices with both widths zero-padded to a
multiple of 16 (the kernels' NHWC channel stride), the depthwise filters tap-major, ``se.conv_expand`` transposed.  ``pack`` is a pure
host function (fp64 in, fp64 out); the engine rounds its result to fp32 on the device.  No torch arithmetic on the data path, no CPU
fallback."""
import ctypes as C

import torch

from . import _lib

OUT_DIM = _lib.EFFNET_OUT
BN_EPS = 1e-5
STEM = 32
# (state-dict prefix, in, expansion, out, depthwise kernel, stride, squeeze width, input size, skip) of the live blocks
BLOCKS = (
    ("blocks.0.0", 32, 32, 16, 3, 1, 8, 16, False),           # depthwise-separable: no expansion, conv_dw reads the stem's 32 maps
    ("blocks.1.0", 16, 96, 24, 3, 2, 4, 16, False), ("blocks.1.1", 24, 144, 24, 3, 1, 6, 8, True),
    ("blocks.2.0", 24, 144, 40, 5, 2, 6, 8, False), ("blocks.2.1", 40, 240, 40, 5, 1, 10, 4, True),
    ("blocks.3.0", 40, 240, 80, 3, 2, 10, 4, False), ("blocks.3.1", 80, 480, 80, 3, 1, 20, 2, True),
    ("blocks.3.2", 80, 480, 80, 3, 1, 20, 2, True),
    ("blocks.4.0", 80, 480, 112, 5, 1, 20, 2, False), ("blocks.4.1", 112, 672, 112, 5, 1, 28, 2, True),
    ("blocks.4.2", 112, 672, 112, 5, 1, 28, 2, True),
)
MAP2, MAP3 = 4, 10                                           # the blocks whose outputs make the row: [map 2 (640) | map 3 (448)]
STAGES = {"stem": 1, **{name: 2 << b for b, (name, *_) in enumerate(BLOCKS)}, "out": 1 << 12}
ALL_STAGES = (1 << 13) - 1
_FIELDS = ("exp_w", "exp_b", "dw_w", "dw_b", "se_rw", "se_rb", "se_ew", "se_eb", "prj_w", "prj_b")


def p16(c):
    """A channel count in the kernels' NHWC layout: rounded up to a multiple of 16 (24 -> 32, 40 -> 48), the padding zero."""
    return (c + 15) // 16 * 16


def tap_shape(b):
    """(channels, H, W) of block ``b``'s output."""
    _, _, _, cout, _, s, _, h, _ = BLOCKS[b]
    return cout, h // s, h // s


def turn_source(quarter_turns):
    """(si, sj) int64 [32, 32]: pixel (i, j) of a crop turned CLOCKWISE by ``quarter_turns`` quarter turns is pixel (si, sj) of the
    crop -- ``torch.rot90(x, -quarter_turns, (2, 3))[..., i, j] == x[..., si[i, j], sj[i, j]]``; the stem kernel's index map."""
    i, j = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    r = int(quarter_turns)
    if r not in (0, 1, 2, 3):
        raise ValueError(f"quarter_turns {quarter_turns!r}: 0 .. 3")
    return ((i, j), (31 - j, i), (31 - i, 31 - j), (j, 31 - i))[r]


def _fold(w, sd, bn, eps):
    """eval BatchNorm folded into the bias-free convolution before it (fp64): W' = diag(s) W, b' = beta - mean s,
    s = gamma / sqrt(var + eps)."""
    s = sd[f"{bn}.weight"].double() / torch.sqrt(sd[f"{bn}.running_var"].double() + eps)
    w = w.double()
    return w * s.view(-1, *([1] * (w.dim() - 1))), sd[f"{bn}.bias"].double() - sd[f"{bn}.running_mean"].double() * s


def _pad(t, *shape):
    out = torch.zeros(*shape, dtype=t.dtype, device=t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def pack(sd, eps=BN_EPS):
    """timm-keyed state dict -> {"stem_w" [32, 27], "stem_b" [32], and per field of ``da_effnet_weights`` a list over the eleven
    blocks} of fp64 tensors in the kernels' layouts (``exp_w[0]`` / ``exp_b[0]`` are None)."""
    w, b = _fold(sd["conv_stem.weight"], sd, "bn1", eps)
    assert tuple(w.shape) == (STEM, 3, 3, 3), tuple(w.shape)
    out = {"stem_w": w.reshape(STEM, 27), "stem_b": b, **{f: [] for f in _FIELDS}}
    for i, (p, cin, mid, cout, k, s, r, h, skip) in enumerate(BLOCKS):
        ds = i == 0                                           # conv_dw, bn1, se, conv_pw, bn2 instead of conv_pw, bn1, conv_dw, bn2, se, conv_pwl, bn3
        if ds:
            out["exp_w"].append(None)
            out["exp_b"].append(None)
        else:
            cw = sd[f"{p}.conv_pw.weight"]
            assert tuple(cw.shape) == (mid, cin, 1, 1), (p, tuple(cw.shape))
            w, b = _fold(cw.reshape(mid, cin), sd, f"{p}.bn1", eps)
            out["exp_w"].append(_pad(w, p16(mid), p16(cin)))
            out["exp_b"].append(_pad(b, p16(mid)))
        dw = sd[f"{p}.conv_dw.weight"]
        assert tuple(dw.shape) == (mid, 1, k, k), (p, tuple(dw.shape))
        w, b = _fold(dw.reshape(mid, k * k), sd, f"{p}.bn1" if ds else f"{p}.bn2", eps)
        out["dw_w"].append(_pad(w.t(), k * k, p16(mid)))
        out["dw_b"].append(_pad(b, p16(mid)))
        rw, ew = sd[f"{p}.se.conv_reduce.weight"], sd[f"{p}.se.conv_expand.weight"]
        assert tuple(rw.shape) == (r, mid, 1, 1) and tuple(ew.shape) == (mid, r, 1, 1), (p, tuple(rw.shape), tuple(ew.shape))
        out["se_rw"].append(_pad(rw.double().reshape(r, mid), r, p16(mid)))
        out["se_rb"].append(sd[f"{p}.se.conv_reduce.bias"].double())
        out["se_ew"].append(_pad(ew.double().reshape(mid, r).t(), r, p16(mid)))
        out["se_eb"].append(_pad(sd[f"{p}.se.conv_expand.bias"].double(), p16(mid)))
        pw = sd[f"{p}.conv_pw.weight" if ds else f"{p}.conv_pwl.weight"]
        assert tuple(pw.shape) == (cout, mid, 1, 1), (p, tuple(pw.shape))
        w, b = _fold(pw.reshape(cout, mid), sd, f"{p}.bn2" if ds else f"{p}.bn3", eps)
        out["prj_w"].append(_pad(w, p16(cout), p16(mid)))
        out["prj_b"].append(_pad(b, p16(cout)))
    return out


class EfficientNetEngine:
    """Packed, folded eval EfficientNet-B0 feature encoder.  ``sd``: state dict with timm's ``efficientnet_b0(features_only=True)``
    keys (``visual_backbone.*`` of an ``Eff_GAT`` checkpoint with the prefix stripped); blocks.5 / blocks.6 are not read."""

    FEATS = OUT_DIM

    def __init__(self, sd, *, eps=BN_EPS, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise _lib.DaError("EfficientNetEngine needs a ROCm device (no CPU path in diffassemble_amd)")
        self.lib = _lib.lib()
        self.chunk = int(self.lib.da_effnet_constant(_lib.EFFNET_CHUNK))          # crops per pass over the workspace
        self.pw_rows = int(self.lib.da_effnet_constant(_lib.EFFNET_PW_ROWS))      # rows (crops * H * W) of a 1x1 convolution's workgroup
        self.pw_cols = int(self.lib.da_effnet_constant(_lib.EFFNET_PW_COLS))
        live = {k: v.detach().to(self.device) for k, v in sd.items()
                if v.is_floating_point() and not k.startswith(("blocks.5.", "blocks.6."))}
        packed = pack(live, eps)
        self._keep = []
        w = _lib.DaEffnetWeights()
        w.stem_w, w.stem_b = self._put(packed["stem_w"]), self._put(packed["stem_b"])
        for f in _FIELDS:
            for b, t in enumerate(packed[f]):
                getattr(w, f)[b] = self._put(t)
        self.w = w
        self._ws = None

    def _put(self, t):
        if t is None:
            return None
        t = t.float().contiguous()
        self._keep.append(t)
        return t.data_ptr()

    def _call(self, crops, quarter_turns, out, taps, stages):
        if crops.device.type != "cuda":
            raise _lib.DaError("EfficientNetEngine.forward: the crops must live on the ROCm device")
        assert crops.dim() == 4 and tuple(crops.shape[1:]) == (3, 32, 32), tuple(crops.shape)
        if int(quarter_turns) not in (0, 1, 2, 3):
            raise ValueError(f"quarter_turns {quarter_turns!r}: 0 .. 3")
        x = crops.detach().to(torch.float32).contiguous()
        n = int(x.shape[0])
        if out is None:
            out = torch.empty(n, OUT_DIM, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.shape == (n, OUT_DIM) and (n == 0 or out.stride(1) == 1)
        st = _lib.stream_ptr(self.device)
        if n == 0:
            _lib.check(self.lib.da_effnet_forward(self.w, 0, None, int(quarter_turns), None, OUT_DIM, None, 0, st))
            return out
        need = self.lib.da_effnet_workspace_bytes(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        args = (self.w, n, _lib.ptr(x), int(quarter_turns), _lib.ptr(out), out.stride(0), _lib.ptr(self._ws), self._ws.numel())
        if taps is None and stages is None:
            _lib.check(self.lib.da_effnet_forward(*args, st))
        else:
            tp = None if taps is None else (C.c_void_p * _lib.EFFNET_BLOCKS)(*[t.data_ptr() for t in taps])
            _lib.check(self.lib.da_effnet_forward_taps(*args, tp, ALL_STAGES if stages is None else int(stages), st))
        return out

    def forward(self, crops, quarter_turns=0, out=None):
        """crops [N, 3, 32, 32] in [0, 1], NOT normalised (device; any float dtype or uint8-derived values, converted to fp32) ->
        [N, 1088] fp32 (``out``: any row stride, unit column stride).  ``quarter_turns`` r: the crops are read turned clockwise by r
        quarter turns, bit-equal to ``forward(torch.rot90(crops, -r, (2, 3)))``."""
        return self._call(crops, quarter_turns, out, None, None)

    def forward_blocks(self, crops, quarter_turns=0, out=None):
        """``forward`` that also returns the eleven block outputs as NCHW fp32 tensors: (taps, out)."""
        n = int(crops.shape[0])
        taps = [torch.empty(n, *tap_shape(b), dtype=torch.float32, device=self.device) for b in range(len(BLOCKS))]
        return taps, self._call(crops, quarter_turns, out, taps if n else None, None)

    def run_stages(self, crops, stages, quarter_turns=0, out=None):
        """Only the stages of the bit set (``STAGES``), on the workspace the last ``forward`` of the same shape left: for timing."""
        return self._call(crops, quarter_turns, out, None, stages)
