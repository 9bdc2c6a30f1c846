"""Host-side checks of the 2D renderer (diffassemble_amd/render2d.py ``batch_frames``, C entry point ``da_render2d``).  No GPU.

Three layers, each pinned to the one below:
  * tests/golden/render2d_v1.npz holds what the reference's ``create_image_from_patches`` (PIL) drew for the cases of
    tests/golden/render2d_refs.py (made by tests/golden/make_render2d_golden.py): frames up to 4 x 5 whole, SHA-256 beyond;
  * the numpy contract of render2d_refs.py reproduces every one of them exactly from the recorded angles;
  * the host route of ``batch_frames`` equals the contract exactly, given the angles the host layer computes, which equal the
    recorded ones to within one fp32 ulp (atan2 of a vector and of a scalar may differ in the last bit).
Everything compared is a byte or an integer: there is no tolerance.  The helpers are shared with tests/test_gpu_render2d.py."""
import functools
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render2d_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def cases():
    return R.load_cases()


@functools.lru_cache(maxsize=None)
def crops_of(name):
    c = cases()[name]
    return R.make_crops(c["seed"], int(c["counts"].sum()))            # shared: the tests only read it


def poses_of(name):
    """[K, N, 2 or 4] fp32 tensor of a case: x, y and, where the case has them, (cos, sin)."""
    c = cases()[name]
    cols = [torch.from_numpy(c["pos"])] + ([torch.from_numpy(c["rot"])] if c["rot"] is not None else [])
    return torch.cat(cols, -1)


def batch_of(name):
    c = cases()[name]
    return torch.repeat_interleave(torch.arange(len(c["counts"])), torch.from_numpy(c["counts"]))


def host_angles(name):
    """The angles the host layer computes for a case on this machine ([K, N] fp32), or None without rotations."""
    from diffassemble_amd.render2d import piece_angles
    return None if cases()[name]["rot"] is None else piece_angles(torch.from_numpy(cases()[name]["rot"])).numpy()


@functools.lru_cache(maxsize=None)
def contract_frames(name):
    """{(k, g): frame} of the contract on the host layer's angles; computed once and shared."""
    out = R.render_case(cases()[name], crops_of(name), deg=host_angles(name))
    for f in out.values():
        f.setflags(write=False)
    return out


def ulp_distance(a, b):
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ fixture and contract
def test_fixture_is_small_and_complete():
    assert os.path.getsize(R.FIXTURE) < 500 * 1000
    cs = cases()
    assert tuple(cs) == R.CASES
    for name, c in cs.items():
        want = len(c["steps"]) * len(c["dims"])
        assert (len(c["sha"]), len(c["frames"])) == ((want, 0) if name in R.HASH_ONLY else (0, want)), name
        assert int(c["counts"].sum()) == c["pos"].shape[1]
    assert cs["ragged"]["counts"].tolist() == [5, 6, 1] and cs["ragged"]["steps"] == [0, 2] and cs["ragged"]["pos"].shape[0] == 3
    assert cs["pile30"]["pos"].shape[1] == 900 and not cs["pile30"]["pos"].any()


@pytest.mark.parametrize("name", R.CASES)
def test_contract_reproduces_the_reference_frames(name):
    c = cases()[name]
    got = R.render_case(c, crops_of(name))
    for key, frame in c["frames"].items():
        assert got[key].shape == frame.shape and got[key].dtype == np.uint8
        assert np.array_equal(got[key], frame), (name, key, int((got[key] != frame).any(-1).sum()))
    for key, digest in c["sha"].items():
        assert R.sha256(got[key]) == digest, (name, key)


def test_cases_reach_what_they_are_for():
    cs = cases()
    assert R.position(cs["one"]["pos"][0, 0], 1, 1) == (-7, -7)                          # clipped on all four sides
    deg = cs["rot2x3"]["deg"][0]
    assert sorted(np.remainder(-deg[:4], np.float32(360)).tolist()) == [0.0, 90.0, 180.0, 270.0]      # the four transposes
    assert any(min(R.coefficients(d)[2], R.coefficients(d)[5]) < 0 for d in deg[4:])     # negative running sums
    p = cs["clip3x5"]["pos"][0]
    x = np.float32(p[3, 0]) * np.float32(1 - 1 / 3)
    t = float((x + np.float32(1)) * np.float32(160) / np.float32(2))
    assert t < 0 and int(t) != int(np.floor(t))                                          # truncation toward zero below -1
    assert R.position(p[7], 3, 5)[0] >= 160 and R.position(p[7], 3, 5)[1] >= 96          # wholly off the canvas
    assert np.float32(1 - 1 / 3) != np.float32(1) - np.float32(1) / np.float32(3)         # the scale is rounded once, from fp64
    # rows scale x: swapping the pairing moves pieces of the 2 x 3 case
    q = cs["rot2x3"]["pos"][0]
    assert any(R.position(q[i], 2, 3) != (int((np.float32(q[i, 0]) * np.float32(1 - 1 / 3) + 1) * 96 / 2) - 23,
                                          int((np.float32(q[i, 1]) * np.float32(1 - 1 / 2) + 1) * 64 / 2) - 23) for i in range(6))


def test_quarter_turns_equal_the_fixed_point_map():
    """PIL turns by 0 / 90 / 180 / 270 with transposes; the rounded coefficients are exact there and give the same tile."""
    tile = R.tile_of(crops_of("one")[0])
    for deg in (0.0, 90.0, 180.0, -90.0, -180.0, 270.0, 360.0, -270.0):
        a = list(R.coefficients(deg))
        out = np.zeros_like(tile)
        for y in range(46):
            for x in range(46):
                xin, yin = (a[2] + a[0] * x + a[1] * y) >> 16, (a[5] + a[3] * x + a[4] * y) >> 16
                if 0 <= xin < 46 and 0 <= yin < 46:
                    out[y, x] = tile[yin, xin]
        assert np.array_equal(out, R.rotate_tile(tile, np.float32(deg))), deg


def test_a_piece_with_a_non_finite_pose_is_not_drawn():
    from diffassemble_amd.render2d import batch_frames
    c = cases()["clip3x5"]
    crops, pos = crops_of("clip3x5"), c["pos"][0].copy()
    keep = [i for i in range(15) if i != 5]
    want = R.render(crops[keep], pos[keep], (3, 5))
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 1):
            q = pos.copy()
            q[5, col] = bad
            assert np.array_equal(R.render(crops, q, (3, 5)), want)
            got = batch_frames(torch.from_numpy(crops), torch.from_numpy(q), [[3, 5]])[0][0]
            assert np.array_equal(got.numpy(), want)
    assert not np.array_equal(want, R.render(crops, pos, (3, 5)))                       # piece 5 is visible when it is drawn


# ------------------------------------------------------------------------------------------------ the host layer
@pytest.mark.parametrize("name", [n for n in R.CASES if n != "one" and n != "clip3x5"])
def test_host_angles_are_the_recorded_ones_to_one_ulp(name):
    got, want = host_angles(name), cases()[name]["deg"]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert int(ulp_distance(got, want).max()) <= 1


def test_host_coefficients_equal_the_contract_rule():
    """The vectorised rounding to 15 decimals is Python's ``round`` on every value: the recorded angles, 20 000 random ones,
    the special ones and their fp32 neighbours."""
    from diffassemble_amd.render2d import rotation_coefficients
    rng = np.random.default_rng(11)
    special = np.array([0, 90, 180, 270, -90, -180, -270, 360, 45, -45, 30, 60, 1e-6, -1e-6, 1e-30, 179.99998, -179.99998], np.float32)
    deg = np.concatenate([c["deg"].reshape(-1) for c in cases().values() if c["deg"] is not None]
                         + [rng.uniform(-400, 400, 20000).astype(np.float32), special, np.nextafter(special, np.float32(1000)),
                            np.nextafter(special, np.float32(-1000))])
    got = rotation_coefficients(deg)
    assert got.dtype == np.int32 and got.shape == (deg.size, 6)
    want = np.array([R.coefficients(d) for d in deg], dtype=np.int64)
    assert np.array_equal(got, want)
    assert rotation_coefficients(deg[:15].reshape(5, 3)).shape == (5, 3, 6)


@pytest.mark.parametrize("name", R.CASES)
def test_batch_frames_on_host_tensors_equals_the_contract(name, monkeypatch):
    from diffassemble_amd import _lib, render2d
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("host tensors must not reach the library"))
    c = cases()[name]
    frames = render2d.batch_frames(torch.from_numpy(crops_of(name)), poses_of(name), c["dims"], batch=batch_of(name), steps=c["steps"])
    want = contract_frames(name)
    assert len(frames) == len(c["steps"]) and all(len(f) == len(c["dims"]) for f in frames)
    for (k, g), w in want.items():
        f = frames[k][g]
        assert f.dtype == torch.uint8 and tuple(f.shape) == w.shape and f.device.type == "cpu"
        assert np.array_equal(f.numpy(), w), (name, k, g)
    if np.array_equal(host_angles(name), c["deg"]) if c["deg"] is not None else True:   # equal angles: the reference's own bytes
        for key, digest in c["sha"].items():
            assert R.sha256(frames[key[0]][key[1]].numpy()) == digest
        for key, frame in c["frames"].items():
            assert np.array_equal(frames[key[0]][key[1]].numpy(), frame)


def test_batch_frames_accepts_a_list_one_step_and_no_rotation():
    from diffassemble_amd.render2d import batch_frames
    c = cases()["ragged"]
    crops, poses, batch = torch.from_numpy(crops_of("ragged")), poses_of("ragged"), batch_of("ragged")
    want = contract_frames("ragged")
    as_list = batch_frames(crops, list(poses.unbind(0)), c["dims"], batch=batch, steps=[0, 2])
    one = batch_frames(crops, poses[2], c["dims"], batch=batch)
    for g in range(3):
        assert np.array_equal(as_list[1][g].numpy(), want[(1, g)]) and np.array_equal(one[0][g].numpy(), want[(1, g)])
    base = as_list[0][0].untyped_storage().data_ptr()
    assert all(f.untyped_storage().data_ptr() == base for fr in as_list for f in fr)      # views of one buffer
    flat = batch_frames(crops, poses[0], c["dims"], batch=batch, rotation=False)           # the (cos, sin) columns ignored
    lo = 0
    for g, n in enumerate(c["counts"]):
        assert np.array_equal(flat[0][g].numpy(), R.render(crops_of("ragged")[lo:lo + n], c["pos"][0, lo:lo + n], c["dims"][g]))
        lo += int(n)


def test_batch_frames_refusals():
    from diffassemble_amd.render2d import batch_frames
    crops, pos = torch.zeros(6, 3, 32, 32), torch.zeros(6, 2)
    with pytest.raises(ValueError, match="all_equivariant"):
        batch_frames(torch.zeros(6, 4, 3, 32, 32), pos, [[2, 3]])
    with pytest.raises(ValueError, match=r"\[N, 3, 32, 32\]"):
        batch_frames(torch.zeros(6, 3, 16, 16), pos, [[2, 3]])
    with pytest.raises(ValueError, match="poses are"):
        batch_frames(crops, torch.zeros(5, 2), [[2, 3]])
    with pytest.raises(ValueError, match="rotation needs"):
        batch_frames(crops, pos, [[2, 3]], rotation=True)
    with pytest.raises(ValueError, match="sorted batch vector"):
        batch_frames(crops, pos, [[2, 3], [1, 1]])
    with pytest.raises(ValueError, match="patches_dim has 1 rows"):
        batch_frames(crops, pos, [[2, 3]], batch=torch.tensor([0, 0, 0, 1, 1, 1]))
    need = 3 * 2 * 3 * 32 * 32 * 4
    with pytest.raises(ValueError, match=rf"{need} bytes.*fewer steps"):
        batch_frames(crops, torch.zeros(3, 6, 2), [[2, 3]], max_bytes=need - 1)
    assert len(batch_frames(crops, torch.zeros(3, 6, 2), [[2, 3]], max_bytes=need)) == 3
    with pytest.raises(ValueError, match=r"11796480000 bytes"):                            # 100 steps x 32 puzzles of 30 x 30: the default cap
        batch_frames(torch.zeros(32, 3, 32, 32), torch.zeros(100, 32, 2), [[30, 30]] * 32, batch=torch.arange(32))


# ------------------------------------------------------------------------------------------------ ABI and module surface
def test_header_library_and_binding_carry_da_render2d():
    from diffassemble_amd import _lib
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_render2d(int n_steps, int n_puzzles, int n_pieces, int max_tiles, const float *patches, const float *poses, "
            "int ld_pose, long long step_stride, const int32_t *coef, const int32_t *puzzles, long long step_bytes, uint8_t *out, "
            "void *stream);") in text
    assert "long long da_render2d_frame_bytes(int rows, int cols);" in text
    assert "spatial_diffusion.py:1204-1234" in text.split("da_render2d_frame_bytes(int rows")[0][-3000:]
    h = _lib.lib()
    for name, n_args in (("da_render2d", 13), ("da_render2d_frame_bytes", 2)):
        assert getattr(h, name).argtypes == _lib.PROTOTYPES[name][1] and len(_lib.PROTOTYPES[name][1]) == n_args
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays
    assert h.da_render2d_frame_bytes(30, 30) == 960 * 960 * 4 and h.da_render2d_frame_bytes(2, 3) == 64 * 96 * 4
    assert h.da_render2d_frame_bytes(0, 3) == 0


def test_entry_point_checks_its_arguments_before_launching():
    import ctypes as C
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(1 << 20)                                                # never dereferenced: every call below is refused

    def call(K=1, G=1, N=1, tiles=1, ld=2, stride=0, step_bytes=4096, ptrs=(one,) * 5):
        patches, poses, coef, puzzles, out = ptrs
        return h.da_render2d(K, G, N, tiles, patches, poses, ld, stride, coef, puzzles, step_bytes, out, None)

    for missing in (0, 1, 3, 4):                                             # coef (2) may be NULL
        assert call(ptrs=tuple(None if k == missing else one for k in range(5))) == 1 and b"null argument" in h.da_last_error(), missing
    for kw in (dict(K=0), dict(G=0), dict(N=0), dict(tiles=0), dict(ld=1), dict(stride=-1), dict(step_bytes=0)):
        assert call(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    assert call(step_bytes=4100) == 1 and b"16-byte aligned" in h.da_last_error()
    assert call(ptrs=(one, one, one, one, C.c_void_p((1 << 20) + 4))) == 1 and b"16-byte aligned" in h.da_last_error()
    assert call(K=1 << 16, G=1 << 10, tiles=900) == 1 and b"pass fewer steps" in h.da_last_error()


def _module(**kw):
    from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
    return GNN_Diffusion(steps=10, sampling="DDIM", model_mean_type=ModelMeanType.START_X, visual_pretrained=False, **kw)


def test_create_image_from_patches_returns_the_reference_picture():
    pytest.importorskip("PIL")
    c = cases()["rot2x3"]
    m = _module(rotation=True)
    img = m.create_image_from_patches(torch.from_numpy(crops_of("rot2x3")), torch.from_numpy(c["pos"][0]), n_patches=(2, 3), i=0,
                                      rotations=torch.from_numpy(c["rot"][0]))
    assert img.mode == "RGBA" and img.size == (96, 64)
    assert np.array_equal(np.asarray(img), contract_frames("rot2x3")[(0, 0)])
    c = cases()["one"]
    img = m.create_image_from_patches(torch.from_numpy(crops_of("one")), torch.from_numpy(c["pos"][0]), n_patches=(1, 1))
    assert img.mode == "RGBA" and img.size == (32, 32) and np.array_equal(np.asarray(img), c["frames"][(0, 0)])


def test_create_image_from_patches_without_pil_names_the_other_call(monkeypatch):
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="render2d.batch_frames"):
        _module().create_image_from_patches(torch.zeros(1, 3, 32, 32), torch.zeros(1, 2), n_patches=(1, 1))


def test_eval_step_saves_every_step_in_chunks_on_host_tensors(tmp_path):
    """The branch of ``_eval_step`` on CPU poses (the loop and the scoring stubbed out): K frames per puzzle reach
    ``save_eval_frame`` under the Batch's ``ind_name``, rendered in chunks of steps that respect the byte budget."""
    from diffassemble_amd import render2d
    c = cases()["ragged"]
    m = _module(rotation=True)
    imgs = list(poses_of("ragged").unbind(0))
    batch = SimpleNamespace(x=imgs[-1], patches=torch.from_numpy(crops_of("ragged")), patches_dim=torch.from_numpy(c["dims"]),
                            batch=batch_of("ragged"), ind_name=torch.tensor([7, 8, 9]))
    want = render2d.batch_frames(batch.patches, imgs, c["dims"], batch=batch.batch)
    seen, calls = {}, []
    m.save_eval_frame = lambda frame, ind_name, step: seen.__setitem__((ind_name, step), frame.clone())
    inner = m.render_frames
    m.render_frames = lambda *a, **k: (calls.append(k["steps"]), inner(*a, **k))[1]
    per_step = sum(int(r) * int(s) * 4096 for r, s in c["dims"])
    for budget, chunks in ((1 << 30, [[0, 1, 2]]), (2 * per_step, [[0, 1], [2]]), (1, [[0], [1], [2]])):
        seen.clear(), calls.clear()
        m.eval_image_max_bytes = budget
        m._save_eval_frames(batch, imgs)
        assert calls == chunks and sorted(seen) == [(n, s) for n in (7, 8, 9) for s in range(3)]
        assert all(torch.equal(seen[(7 + g, s)], want[s][g]) for g in range(3) for s in range(3))
    assert m.eval_image_dir == "results/test" and m.save_eval_images is False


def test_default_save_eval_frame_writes_a_png(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    m = _module()
    m.eval_image_dir = str(tmp_path / "deep" / "er")
    frame = torch.from_numpy(contract_frames("rot2x3")[(0, 0)].copy())
    m.save_eval_frame(frame, 4, 17)
    assert os.listdir(m.eval_image_dir) == ["004_017.png"]
    with Image.open(os.path.join(m.eval_image_dir, "004_017.png")) as im:
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), frame.numpy())


def test_eval_step_without_save_eval_images_never_imports_render2d():
    """In a fresh interpreter: ``_eval_step`` with the default ``save_eval_images = False`` (loop and scoring stubbed) leaves
    ``diffassemble_amd.render2d`` unimported; switching it on imports it."""
    code = """
import sys, types, torch
sys.path.insert(0, %r)
from diffassemble_amd.model.spatial_diffusion import GNN_Diffusion, ModelMeanType
from diffassemble_amd import score2d
m = GNN_Diffusion(steps=10, sampling="DDIM", model_mean_type=ModelMeanType.START_X, visual_pretrained=False)
pose = torch.zeros(1, 2)
m.p_sample_loop = lambda *a, **k: ([pose, pose], None)
score2d.batch_scores = lambda *a, **k: (torch.ones(1, dtype=torch.bool), torch.ones(1, dtype=torch.bool), torch.tensor([[1, 1, 1]]))
batch = types.SimpleNamespace(x=pose, patches=torch.zeros(1, 3, 32, 32), edge_index=None, batch=torch.zeros(1, dtype=torch.long), patches_dim=torch.tensor([[1, 1]]))
assert m.save_eval_images is False
assert m.test_step(batch, 0) is pose and m.validation_step(batch, 0) is pose
assert "diffassemble_amd.render2d" not in sys.modules, "render2d imported with save_eval_images off"
got = []
m.save_eval_frame = lambda frame, ind_name, step: got.append((ind_name, step, tuple(frame.shape)))
m.save_eval_images = True
assert m.test_step(batch, 0) is pose
assert "diffassemble_amd.render2d" in sys.modules and got == [(0, 0, (32, 32, 4)), (0, 1, (32, 32, 4))], got
print("OK")
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_product_file_does_not_import_the_oracle_or_pil():
    src = open(os.path.join(ROOT, "diffassemble_amd", "render2d.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "import PIL" not in src and "from PIL" not in src
