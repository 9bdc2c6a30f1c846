"""The numpy contract of the 2D renderer (diffassemble_amd/render2d.py, da_render2d): the rule by which the reference's
``create_image_from_patches`` (spatial_diffusion.py:1204-1234) composes a puzzle's picture, restated step by step the way PIL
carries it out -- make the RGBA tile, pad it, rotate it into a second tile, paste that with its alpha -- in integer arithmetic,
without PIL and without anything of the package under test.  tests/golden/render2d_v1.npz holds what the reference itself
produced for the cases below (tests/golden/make_render2d_golden.py); tests/test_render2d_host.py proves this file equal to
those frames, and the GPU test compares the kernel with this file.

Also here: the crops of the cases (random bytes / 255 from a recorded seed; they are not stored) and the loader of the fixture."""
import hashlib
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "render2d_v1.npz")
CASES = ("one", "rot2x3", "clip3x5", "stack4x5", "ragged", "many12", "pile30", "solved30")
HASH_ONLY = ("many12", "pile30", "solved30")


def make_crops(seed, n):
    """[n, 3, 32, 32] fp32 crops: bytes / 255, so that every colour of the picture is one of the 256 the bytes name."""
    rng = np.random.default_rng(int(seed))
    return (rng.integers(0, 256, size=(n, 3, 32, 32)) / 255).astype(np.float32)


def sha256(frame):
    return hashlib.sha256(np.ascontiguousarray(frame, dtype=np.uint8).tobytes()).hexdigest()


def load_cases():
    """{name: dict(seed, dims [G, 2], counts [G], pos [K, N, 2], rot [K, N, 2] or None, deg [K, N] or None, steps,
    frames {(k, g): uint8 [H, W, 4]} or sha {(k, g): hex})} from the fixture; k counts the selected steps."""
    z = np.load(FIXTURE)
    out = {}
    for name in CASES:
        c = dict(seed=int(z[f"{name}/seed"]), dims=z[f"{name}/dims"], counts=z[f"{name}/counts"], pos=z[f"{name}/pos"],
                 rot=z[f"{name}/rot"] if f"{name}/rot" in z else None, deg=z[f"{name}/deg"] if f"{name}/deg" in z else None,
                 steps=[int(s) for s in z[f"{name}/steps"]], frames={}, sha={})
        for k in range(len(c["steps"])):
            for g in range(len(c["dims"])):
                if f"{name}/frame_{k}_{g}" in z:
                    c["frames"][(k, g)] = z[f"{name}/frame_{k}_{g}"]
                else:
                    c["sha"][(k, g)] = str(z[f"{name}/sha_{k}_{g}"])
        out[name] = c
    return out


# ------------------------------------------------------------------ the rule
def tile_of(crop):
    """The padded 46 x 46 RGBA tile of one fp32 crop [3, 32, 32]."""
    tile = np.zeros((46, 46, 4), dtype=np.uint8)
    tile[7:39, 7:39, :3] = (crop.transpose(1, 2, 0) * np.float32(255)).astype(np.int32).astype(np.uint8)      # truncation
    tile[7:39, 7:39, 3] = 255
    return tile


def coefficients(deg):
    """What ``Image.rotate(-deg)`` hands to its nearest-neighbour affine loop for a 46 x 46 image, as the loop's six 16.16
    integers.  ``deg`` is the fp32 angle; ``-deg % 360.0`` is an fp32 remainder with the sign of the divisor."""
    angle = float(np.remainder(-np.float32(deg), np.float32(360.0)))
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x = y = -23.0
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += 23.0
    m[5] += 23.0

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate_tile(tile, deg):
    """``tile.rotate(-deg)`` of PIL with its defaults.  The quarter turns are written as the transposes PIL uses for them;
    every other angle walks the destination rows with running integer sums."""
    angle = float(np.remainder(-np.float32(deg), np.float32(360.0)))
    if angle == 0:
        return tile.copy()
    if angle == 180:
        return tile[::-1, ::-1].copy()
    if angle == 90:                                    # counter-clockwise quarter turn
        return np.ascontiguousarray(tile.transpose(1, 0, 2)[::-1])
    if angle == 270:
        return np.ascontiguousarray(tile.transpose(1, 0, 2)[:, ::-1])
    a0, a1, a2, a3, a4, a5 = coefficients(deg)
    out = np.zeros_like(tile)
    xs = np.arange(46, dtype=np.int64)
    for y in range(46):
        xin, yin = (a2 + a0 * xs) >> 16, (a5 + a3 * xs) >> 16          # the running sums xx += a0, yy += a3 in closed form
        ok = (xin >= 0) & (xin < 46) & (yin >= 0) & (yin < 46)
        out[y, ok] = tile[yin[ok], xin[ok]]
        a2 += a1
        a5 += a4
    return out


def position(pos, rows, cols):
    """(x_pos, y_pos) of a piece, or None when a coordinate is not finite.  fp32 throughout; the factors (1 - 1 / rows) and
    (1 - 1 / cols) are Python floats that meet an fp32 tensor, so they are rounded to fp32 once."""
    W, H = np.float32(32 * cols), np.float32(32 * rows)
    with np.errstate(all="ignore"):
        x = np.float32(pos[0]) * np.float32(1 - 1 / rows)
        y = np.float32(pos[1]) * np.float32(1 - 1 / cols)
        tx, ty = (x + np.float32(1)) * W / np.float32(2), (y + np.float32(1)) * H / np.float32(2)
    if not (math.isfinite(float(tx)) and math.isfinite(float(ty))) or abs(float(tx)) >= 1e9 or abs(float(ty)) >= 1e9:
        return None                                    # the reference raises here; the project does not draw the piece
    return int(tx) - 23, int(ty) - 23                  # int() truncates toward zero


def render(crops, pos, dims, deg=None):
    """The frame of one puzzle: ``crops`` [n, 3, 32, 32], ``pos`` [n, >= 2], ``dims`` (rows, cols), ``deg`` [n] fp32 or None."""
    rows, cols = int(dims[0]), int(dims[1])
    H, W = 32 * rows, 32 * cols
    canvas = np.zeros((H, W, 4), dtype=np.uint8)
    for p in range(len(crops)):
        tile = tile_of(crops[p])
        if deg is not None:
            tile = rotate_tile(tile, deg[p])
        at = position(pos[p], rows, cols)
        if at is None:
            continue
        x_pos, y_pos = at
        x0, x1, y0, y1 = max(x_pos, 0), min(x_pos + 46, W), max(y_pos, 0), min(y_pos + 46, H)
        if x0 >= x1 or y0 >= y1:
            continue
        src = tile[y0 - y_pos:y1 - y_pos, x0 - x_pos:x1 - x_pos]
        mask = src[..., 3] == 255                       # the alpha is 0 or 255: the blend is a choice
        canvas[y0:y1, x0:x1][mask] = src[mask]
    return canvas


def render_case(case, crops, deg=None):
    """{(k, g): frame} of a loaded case; ``deg`` [K_all, N] overrides the recorded angles (None: the recorded ones)."""
    deg = case["deg"] if deg is None else deg
    out = {}
    for k, s in enumerate(case["steps"]):
        lo = 0
        for g, n in enumerate(case["counts"]):
            out[(k, g)] = render(crops[lo:lo + n], case["pos"][s, lo:lo + n], case["dims"][g],
                                 None if case["rot"] is None else deg[s, lo:lo + n])
            lo += int(n)
    return out
