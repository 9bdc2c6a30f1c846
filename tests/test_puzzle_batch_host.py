"""Host-side checks of the Batch builder (diffassemble_amd/puzzle_batch.py ``make_batch``, C entry points ``da_puzzle_batch`` and
``da_complete_edges``).  No GPU.

tests/golden/puzzle_batch_v1.npz holds what the reference's own dataset classes returned for four small puzzles in five modes
(made by tests/golden/make_puzzle_batch_golden.py).  The host route ``_loop_batch`` must equal it with ``torch.equal`` on every
attribute; tests/test_gpu_puzzle_batch.py then holds the kernel to the fixture and to ``_loop_batch``.  Everything compared is a
byte, an integer or an fp32 value copied from a table: there is no tolerance.  The helpers are shared with the GPU file."""
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "puzzle_batch_v1.npz")
MODES = {"plain": {}, "rot": dict(rotation=True), "roteq": dict(rotation=True, all_equivariant=True), "mp": {}, "rotmp": dict(rotation=True)}
ATTRS = ("x", "patches", "indexes", "rot", "rot_index", "edge_index", "batch", "ptr", "patches_dim", "ind_name")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        blob = {k: z[k] for k in z.files}
    for v in blob.values():
        v.setflags(write=False)
    return blob


def puzzles():
    return [tuple(int(v) for v in d) for d in fixture()["puzzles"]]


def images():
    return [torch.from_numpy(fixture()[f"image/{g}"].copy()) for g in range(len(puzzles()))]


def unit():
    return torch.arange(256, dtype=torch.uint8).float() / 255


def ref(mode, g, name):
    """What the reference returned for puzzle g in a mode (None where it returns no such attribute); crops as fp32."""
    v = fixture().get(f"{mode}/{g}/{name}")
    if v is None:
        return None
    v = torch.from_numpy(v.copy())
    return unit()[v.long()] if name == "patches" else v


def fixture_draws(mode):
    """(rot_index, keep) arguments that repeat the reference's draws of a mode."""
    n_of = [r * c for r, c in puzzles()]
    rot_index = torch.cat([ref(mode, g, "rot_index") for g in range(4)]) if MODES[mode].get("rotation") else None
    keep = [ref(mode, g, "keep").tolist() for g in range(4)] if mode in ("mp", "rotmp") else None
    assert rot_index is None or rot_index.numel() == sum(n_of)
    return rot_index, keep


@functools.lru_cache(maxsize=None)
def expected(mode):
    """The Batch the fixture describes for a mode, collated as PyG does; with missing pieces rot / rot_index / indexes are
    gathered by the kept list (the one intended difference from the reference).  Computed once; the tests only read it."""
    out = {k: [] for k in ("x", "patches", "indexes", "rot", "rot_index", "edge_index", "batch")}
    ptr = [0]
    for g, (rows, cols) in enumerate(puzzles()):
        n = rows * cols
        keep = ref(mode, g, "keep")
        kept = torch.arange(n) if keep is None else keep
        out["x"].append(ref(mode, g, "x"))
        out["patches"].append(ref(mode, g, "patches"))
        idx = ref(mode, g, "indexes")
        assert idx is None or torch.equal(idx, torch.arange(n))
        out["indexes"].append(torch.arange(n)[kept])
        r = ref(mode, g, "rot_index")
        if r is None:
            r, rot = torch.zeros(n, dtype=torch.long), torch.tensor([[1, 0]]).repeat(n, 1)
        else:
            rot = ref(mode, g, "rot")
        out["rot"].append(rot[kept])
        out["rot_index"].append(r[kept])
        out["edge_index"].append(ref(mode, g, "edge_index") + ptr[-1])
        out["batch"].append(torch.full((len(kept),), g, dtype=torch.long))
        assert ref(mode, g, "ind_name").tolist() == [g] and ref(mode, g, "patches_dim").tolist() == [[rows, cols]]
        ptr.append(ptr[-1] + len(kept))
    res = {k: torch.cat(v, 1 if k == "edge_index" else 0) for k, v in out.items()}
    res["ptr"] = torch.tensor(ptr)
    res["patches_dim"] = torch.tensor(puzzles())
    res["ind_name"] = torch.arange(4)
    return res


def assert_batch_equal(got, want, where=""):
    """``torch.equal`` (values, shape) and dtype on every attribute of ``want`` (a dict or a PuzzleBatch)."""
    want = want if isinstance(want, dict) else want.__dict__
    for name in ATTRS:
        if name not in want:
            assert not hasattr(got, name), (where, name)
            continue
        g, w = getattr(got, name), want[name]
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (where, name, g.dtype, tuple(g.shape), w.dtype, tuple(w.shape))
        assert torch.equal(g.cpu(), w.cpu()), (where, name, int((g.cpu() != w.cpu()).sum()))
    assert got.num_graphs == len(want["ptr"]) - 1


def build(mode, **kw):
    from diffassemble_amd import make_batch
    rot_index, keep = fixture_draws(mode)
    missing = int(fixture()["missing_perc"]) if keep is not None else 0
    return make_batch(kw.pop("images", images()), puzzles(), rot_index=rot_index, keep=keep, missing_perc=missing, **MODES[mode], **kw)


def noise_images(dims, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (32 * r, 32 * c, 3), generator=g, dtype=torch.uint8) for r, c in dims]


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_small_and_says_what_it_is_for():
    assert os.path.getsize(FIXTURE) < 300 * 1000
    assert puzzles() == [(2, 3), (3, 2), (1, 4), (3, 3)]
    for g, (rows, cols) in enumerate(puzzles()):
        assert fixture()[f"image/{g}"].shape == (32 * rows, 32 * cols, 3) and fixture()[f"image/{g}"].dtype == np.uint8
        for mode in ("rot", "roteq"):
            assert sorted(set(ref(mode, g, "rot_index").tolist())) == [0, 1, 2, 3], (mode, g)     # every turn in every puzzle
        for mode in ("mp", "rotmp"):
            keep, n = ref(mode, g, "keep").tolist(), rows * cols
            assert len(keep) == n - int(np.ceil(n * 30 / 100)) and len(set(keep)) == len(keep), (mode, g, keep)
        assert ref("roteq", g, "patches").shape == (rows * cols, 4, 3, 32, 32)
        # the reference leaves these at full length under missing pieces: the difference make_batch removes on purpose
        assert ref("rotmp", g, "rot_index").shape == (rows * cols,) and ref("rotmp", g, "x").shape[0] < rows * cols
    assert any(ref(mode, g, "keep").tolist() != sorted(ref(mode, g, "keep").tolist()) for mode in ("mp", "rotmp") for g in range(4))
    assert np.array_equal(fixture()["unit"], unit().numpy())


def test_quarter_turns_of_the_fixture_are_rot90_and_every_byte_survives_the_round_trip():
    """The two facts the kernel rests on: PIL's quarter turn is np.rot90, and trunc(v / 255 * 255) == v for every byte."""
    for g, (rows, cols) in enumerate(puzzles()):
        img = fixture()[f"image/{g}"]
        r = ref("roteq", g, "rot_index").tolist()
        got = fixture()[f"roteq/{g}/patches"]
        for p in range(rows * cols):
            i, j = divmod(p, cols)
            tile = img[32 * i:32 * i + 32, 32 * j:32 * j + 32]
            for k in range(4):
                assert np.array_equal(got[p, k], np.rot90(tile, (r[p] + k) % 4).transpose(2, 0, 1)), (g, p, k)
    assert torch.equal((unit() * 255).long(), torch.arange(256))


# ------------------------------------------------------------------------------------------------ the host route
@pytest.mark.parametrize("mode", list(MODES))
def test_loop_batch_equals_the_reference(mode, monkeypatch):
    from diffassemble_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("host tensors must not reach the library"))
    got = build(mode)
    assert_batch_equal(got, expected(mode), mode)
    assert got.x.device.type == "cpu"
    if mode in ("mp", "rotmp"):                                  # x and patches equal the reference directly (checked above via cat)
        lo = 0
        for g in range(4):
            n = ref(mode, g, "x").shape[0]
            assert torch.equal(got.x[lo:lo + n], ref(mode, g, "x")) and torch.equal(got.patches[lo:lo + n], ref(mode, g, "patches"))
            lo += n


def test_padding_equals_zero_margin():
    from diffassemble_amd import make_batch
    got = make_batch(images()[:1], puzzles()[0], padding=3)
    assert torch.equal(got.patches, ref("pad3", 0, "patches")) and not torch.equal(got.patches, ref("plain", 0, "patches"))
    full = make_batch(images()[:1], puzzles()[0], padding=16)
    assert not full.patches.any()
    eq = make_batch(images()[:1], puzzles()[0], padding=3, rotation=True, all_equivariant=True, rot_index=ref("roteq", 0, "rot_index"))
    want = ref("roteq", 0, "patches").clone()
    want[..., :3, :] = 0
    want[..., -3:, :] = 0
    want[..., :, :3] = 0
    want[..., :, -3:] = 0
    assert torch.equal(eq.patches, want)


@pytest.mark.parametrize("side", [6, 7, 12, 30])
def test_positions_are_torch_linspace(side):
    from diffassemble_amd import make_batch
    other = 2
    for rows, cols in ((side, other), (other, side)):
        got = make_batch([torch.zeros(32 * rows, 32 * cols, 3, dtype=torch.uint8)], (rows, cols), edges=None)
        x, y = torch.linspace(-1, 1, cols), torch.linspace(-1, 1, rows)
        assert torch.equal(got.x, torch.stack(torch.meshgrid(x, y, indexing="xy"), -1).reshape(-1, 2))
        assert not hasattr(got, "edge_index")
    if side == 7:
        assert float(torch.linspace(-1, 1, 7)[3]) != 0.0          # what a home-made -1 + i * step would give


def test_tables_carry_torch_linspace_for_every_side():
    from diffassemble_amd import puzzle_batch as P
    dims = [(6, 7), (12, 30), (7, 7)]
    keeps = [list(range(r * c)) for r, c in dims]
    buf, where, N, E, n_lin = P._tables(dims, [[0] * len(k) for k in keeps], keeps, [0, 1, 2], True)
    a, b, dtype, shape = where["lin"]
    lin = torch.from_numpy(buf[a:b].view(np.float32).copy())
    assert n_lin == 6 + 7 + 12 + 30 and torch.equal(lin, torch.cat([torch.linspace(-1, 1, s) for s in (6, 7, 12, 30)]))
    a, b, dtype, shape = where["puzzles"]
    pz = buf[a:b].view(np.int32).reshape(shape)
    assert pz[:, 2:6].tolist() == [[6, 7, 0, 42], [12, 30, 42, 360], [7, 7, 402, 49]]
    assert pz[:, 6:].tolist() == [[6, 0], [25, 13], [6, 6]]      # x table = cols, y table = rows
    assert pz[:, 0].tolist() == [0, 42 * 3072, 402 * 3072] and all(where[k][0] % 16 == 0 for k in where)
    a, b, dtype, shape = where["unit"]
    assert torch.equal(torch.from_numpy(buf[a:b].view(np.float32).copy()), unit())
    assert (N, E) == (451, 42 * 42 + 360 * 360 + 49 * 49)


def test_a_2x3_and_a_3x2_puzzle_differ_in_x():
    from diffassemble_amd import make_batch
    a = make_batch([torch.zeros(64, 96, 3, dtype=torch.uint8)], (2, 3)).x
    b = make_batch([torch.zeros(96, 64, 3, dtype=torch.uint8)], (3, 2)).x
    assert a.shape == b.shape and not torch.equal(a, b)
    assert a[:, 0].tolist() == [-1, 0, 1, -1, 0, 1] and a[:, 1].tolist() == [-1, -1, -1, 1, 1, 1]
    assert b[:, 0].tolist() == [-1, 1, -1, 1, -1, 1] and b[:, 1].tolist() == [-1, -1, 0, 0, 1, 1]


def test_dtype_and_shape_of_every_attribute():
    got = build("rotmp")
    N = sum(len(ref("rotmp", g, "keep")) for g in range(4))
    E = sum(len(ref("rotmp", g, "keep")) ** 2 for g in range(4))
    want = dict(x=(torch.float32, (N, 4)), patches=(torch.float32, (N, 3, 32, 32)), indexes=(torch.int64, (N,)), rot=(torch.int64, (N, 2)),
                rot_index=(torch.int64, (N,)), edge_index=(torch.int64, (2, E)), batch=(torch.int64, (N,)), ptr=(torch.int64, (5,)),
                patches_dim=(torch.int64, (4, 2)), ind_name=(torch.int64, (4,)))
    assert sorted(want) == sorted(ATTRS)
    for name, (dtype, shape) in want.items():
        v = getattr(got, name)
        assert v.dtype == dtype and tuple(v.shape) == shape, name
    assert got.num_graphs == 4 and sorted(got.keys()) == sorted(ATTRS + ("num_graphs",))
    assert build("plain").x.shape == (25, 2) and build("roteq").patches.shape == (25, 4, 3, 32, 32)
    assert torch.equal(got.x[:, 2:], got.rot.float())
    assert build("plain", ind_name=[7, 5, 3, 1]).ind_name.tolist() == [7, 5, 3, 1]


def test_one_stacked_tensor_numpy_and_pil_inputs_agree():
    from diffassemble_amd import make_batch
    Image = pytest.importorskip("PIL.Image")
    imgs = noise_images([(2, 2)] * 3, 5)
    g = lambda: torch.Generator().manual_seed(9)
    want = make_batch(imgs, (2, 2), rotation=True, missing_perc=25, generator=g())
    assert want.x.shape[0] == 9 and want.ptr.tolist() == [0, 3, 6, 9]
    for other in (torch.stack(imgs), [i.numpy() for i in imgs], [Image.fromarray(i.numpy()) for i in imgs]):
        assert_batch_equal(make_batch(other, [(2, 2)] * 3, rotation=True, missing_perc=25, generator=g()), want)
    assert make_batch(imgs, (2, 2), keep=[[3], [0, 1, 2, 3], [2, 0]]).ptr.tolist() == [0, 1, 5, 7]      # keep alone decides


def test_every_refusal():
    from diffassemble_amd import make_batch
    from diffassemble_amd import puzzle_batch as P
    img = torch.zeros(64, 96, 3, dtype=torch.uint8)
    for bad, match in ((dict(images=[torch.zeros(64, 64, 3, dtype=torch.uint8)]), "resize it first"),
                       (dict(images=[torch.zeros(64, 96, 3)]), "uint8"),
                       (dict(images=[torch.zeros(64, 96, 4, dtype=torch.uint8)]), r"\[H, W, 3\]"),
                       (dict(images=torch.zeros(64, 96, 3, dtype=torch.uint8)), r"\[G, H, W, 3\]"),
                       (dict(images=[]), "no image"),
                       (dict(patch_per_dim=[(2, 3), (2, 3)]), "one pair per puzzle"),
                       (dict(patch_per_dim=(0, 3)), "positive"),
                       (dict(all_equivariant=True), "needs rotation=True"),
                       (dict(padding=17), "padding"), (dict(padding=-1), "padding"), (dict(padding=1.5), "padding"),
                       (dict(edges="ring"), "edges is"),
                       (dict(ind_name=[1, 2]), "ind_name"),
                       (dict(rot_index=[0] * 6), "needs rotation=True"),
                       (dict(rotation=True, rot_index=[0] * 5), "one entry per cell"),
                       (dict(rotation=True, rot_index=[0, 1, 2, 3, 4, 0]), "0 .. 3"),
                       (dict(rotation=True, rot_index=[0, 1, 2, 3, -1, 0]), "0 .. 3"),
                       (dict(rotation=True, rot_index=torch.zeros(6)), "integers"),
                       (dict(keep=[[0], [1]]), "one list of kept cells per puzzle"),
                       (dict(keep=[[0, 6]]), "names cells 0 .. 5"), (dict(keep=[[-1]]), "names cells 0 .. 5"),
                       (dict(keep=[[0, 2, 0]]), "repeats a cell"),
                       (dict(keep=[[]]), "leaves no piece"),
                       (dict(keep=[[0, 1]], missing_perc=30), "leaves 4 of 6"),
                       (dict(missing_perc=100), "leaves no piece"), (dict(missing_perc=-1), "percentage")):
        kw = dict(images=[img], patch_per_dim=(2, 3))
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            make_batch(kw.pop("images"), kw.pop("patch_per_dim"), **kw)
    pil = pytest.importorskip("PIL.Image")
    with pytest.raises(ValueError, match="convert it to 'RGB'"):
        make_batch([pil.new("L", (96, 64))], (2, 3))


def test_complete_edges_are_refused_above_the_cap(monkeypatch):
    from diffassemble_amd import make_batch
    from diffassemble_amd import puzzle_batch as P
    imgs = [torch.zeros(64, 96, 3, dtype=torch.uint8)] * 2
    monkeypatch.setattr(P, "MAX_EDGE_BYTES", 16 * 72 - 1)
    with pytest.raises(ValueError, match=r"72 edges = 1152 bytes.*edges=None"):
        make_batch(imgs, (2, 3))
    assert not hasattr(make_batch(imgs, (2, 3), edges=None), "edge_index")
    monkeypatch.setattr(P, "MAX_EDGE_BYTES", 16 * 72)
    assert make_batch(imgs, (2, 3)).edge_index.shape == (2, 72)
    monkeypatch.undo()
    assert 16 * 64 * 900 ** 2 > P.MAX_EDGE_BYTES >= 16 * 64 * 144 ** 2        # the headline Batch is refused, the training Batch is not


def test_image_to_pieces_to_image_on_the_host():
    """Rendering the ground-truth x of an unrotated, complete Batch gives the pictures back (square puzzles: the renderer scales
    x by the row count, the reference's pairing, so only they tile their canvas)."""
    from diffassemble_amd import make_batch
    from diffassemble_amd.render2d import batch_frames
    dims = [(4, 4), (2, 2), (1, 1)]
    imgs = noise_images(dims, 8)
    batch = make_batch(imgs, dims)
    frames = batch_frames(batch.patches, batch.x, batch.patches_dim, batch=batch.batch)[0]
    for g, img in enumerate(imgs):
        assert torch.equal(frames[g][..., :3], img) and bool((frames[g][..., 3] == 255).all()), g


# ------------------------------------------------------------------------------------------------ the kernel's LDS layout
def test_view_reads_of_the_padded_tile_are_conflict_free():
    """The bank rule for 4-byte LDS reads (two 32-lane halves, bank = dword address % 32) applied to the four reads of every
    view of k_puzzle_batch, tile row stride 97 floats: no two lanes of a half meet on a bank.  With stride 96 the column-wise
    views (t = 1, 3) are 8-way."""
    def worst(ld):
        out = {}
        for t in range(4):
            w = 0
            for half in range(8):
                lanes = range(32 * half, 32 * half + 32)
                for c in range(3):
                    for e in range(4):
                        banks = {}
                        for tid in lanes:
                            q4, y = (tid & 7) * 4, tid >> 3
                            base, step = ((y * ld + 3 * q4, 3), (q4 * ld + 3 * (31 - y), ld), ((31 - y) * ld + 3 * (31 - q4), -3),
                                          ((31 - q4) * ld + 3 * y, -ld))[t]
                            a = base + e * step + c
                            assert 0 <= a < 32 * ld
                            banks.setdefault(a % 32, set()).add(a)
                        w = max(w, max(len(v) for v in banks.values()))
            out[t] = w
        return out
    assert worst(97) == {0: 1, 1: 1, 2: 1, 3: 1}
    assert worst(96)[1] == 8 and worst(96)[3] == 8


# ------------------------------------------------------------------------------------------------ ABI and module surface
def test_header_library_and_binding_carry_the_two_entry_points():
    from diffassemble_amd import _lib
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_puzzle_batch(int n_puzzles, int n_pieces, const uint8_t *images, long long image_bytes, const int32_t *puzzles, "
            "const int32_t *pieces, const float *lin, int n_lin, const float *unit, int padding, int views, int x_cols, float *patches, "
            "float *x, long long *rot, long long *rot_index, long long *indexes, long long *batch, void *stream);") in text
    assert "int da_complete_edges(int n_puzzles, const long long *table, long long n_edges, long long *edge_index, void *stream);" in text
    doc = text.split("int da_puzzle_batch(")[0][-3500:]
    for line in ("dataset/puzzle_dataset.py", ":175-190", ":257-300", ":326-332", ":403-485", ":507-544", ":580-700"):
        assert line in doc, line
    h = _lib.lib()
    for name, n_args in (("da_puzzle_batch", 19), ("da_complete_edges", 5)):
        assert getattr(h, name).argtypes == _lib.PROTOTYPES[name][1] and len(_lib.PROTOTYPES[name][1]) == n_args
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays


def test_entry_points_check_their_arguments_before_launching():
    import ctypes as C
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(1 << 20)                                                # never dereferenced: every call below is refused

    def call(G=1, N=1, nbytes=3072, n_lin=2, padding=0, views=1, x_cols=2, ptrs=(one,) * 11):
        images, puzzles, pieces, lin, unit_, patches, x, rot, rot_index, indexes, batch = ptrs
        return h.da_puzzle_batch(G, N, images, nbytes, puzzles, pieces, lin, n_lin, unit_, padding, views, x_cols, patches, x, rot, rot_index,
                                 indexes, batch, None)

    for missing in range(11):
        assert call(ptrs=tuple(None if k == missing else one for k in range(11))) == 1 and b"null argument" in h.da_last_error(), missing
    for kw in (dict(G=0), dict(N=0), dict(N=-3), dict(nbytes=0), dict(n_lin=0)):
        assert call(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    for v in (0, 2, 3, 5):
        assert call(views=v) == 1 and b"views is 1 or 4" in h.da_last_error()
    for v in (1, 3):
        assert call(x_cols=v) == 1 and b"2 or 4 columns" in h.da_last_error()
    for v in (-1, 17):
        assert call(padding=v) == 1 and b"padding is 0 .. 16" in h.da_last_error()
    odd = C.c_void_p((1 << 20) + 4)
    for k in (0, 2, 5):
        assert call(ptrs=tuple(odd if i == k else one for i in range(11))) == 1 and b"16-byte aligned" in h.da_last_error(), k
    assert call(N=1 << 24) == 1 and b"in one launch" in h.da_last_error()
    assert h.da_complete_edges(1, None, 4, one, None) == 1 and b"null argument" in h.da_last_error()
    assert h.da_complete_edges(1, one, 4, None, None) == 1 and b"null argument" in h.da_last_error()
    for G, E in ((0, 4), (1, 0), (1, -1)):
        assert h.da_complete_edges(G, one, E, one, None) == 1 and b"bad sizes" in h.da_last_error()
    assert h.da_complete_edges(1, one, 1 << 32, one, None) == 1 and b"in one launch" in h.da_last_error()


def test_make_batch_is_exported_and_the_module_needs_neither_the_oracle_nor_pil_to_import():
    import diffassemble_amd
    from diffassemble_amd import puzzle_batch as P
    assert diffassemble_amd.make_batch is P.make_batch and "make_batch" in diffassemble_amd.__all__
    src = open(os.path.join(ROOT, "diffassemble_amd", "puzzle_batch.py")).read()
    assert "import oracle" not in src and "from oracle" not in src
    assert not re.search(r"^(import PIL|from PIL)", src, re.M)               # PIL is imported inside the host route only
    for words in ("all five follow the kept list", ":462-485"):
        assert words in P.__doc__
