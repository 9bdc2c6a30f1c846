"""Host-side checks of the 3D Batch builder (diffassemble_amd/fragment_batch.py ``make_batch3d``, C entry points
``da_mesh_cum_area`` and ``da_fragment_batch``).  No GPU.

The expectation is a literal per-part loop written here from the steps of the reference's dataset/breakingbad_dt.py (:113-149,
with the body of ``trimesh.sample.sample_surface`` spelled out: trimesh is not installed, so nothing is pinned to its outputs)
and dataset/objects_dataset.py (:174-225), with scipy's ``Rotation`` for the quaternion and the Euler matrix.  The host route
``_loop_batch3d`` must equal it bit for bit.  This module also holds the meshes and the fixed draws that
tests/test_gpu_fragment_batch.py runs through the kernels, and proves the margin condition on them: no pick lies close enough
to a boundary of the running area sum for a differently ordered fp64 sum to move it to another face."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_LIST = (1, 7, 256, 257, 1000)
COUNTS = (2, 5, 20)                               # parts per object of the shared case
SEED = 20


# ------------------------------------------------------------------------------------------------ meshes, made here
def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def cube(offset=1.0e3):
    """12 triangles, far from the origin: the centring cancels three digits."""
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]) * np.array([1.0, 0.7, 1.3]) + offset
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def icosphere(levels=1):
    g = (1 + math.sqrt(5)) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / math.sqrt(1 + g * g) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt((p * p).sum()))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


def strip(F, seed):
    """F triangles (i, i + 1, i + 2) over F + 2 random vertices: any face count, areas of every size."""
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, (F + 2, 3))
    i = np.arange(F)
    return v, np.stack([i, i + 1, i + 2], 1)


def with_zero_area_faces():
    """The first face, two in the middle and the last have area 0 (a repeated vertex, three collinear vertices)."""
    v, f = strip(9, 5)
    v = np.concatenate([v, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]]])
    f = np.concatenate([[[0, 0, 1]], f[:4], [[11, 12, 13], [3, 3, 3]], f[4:], [[12, 11, 13]]])
    return v, f


def one_huge_many_tiny():
    v, f = strip(60, 6)
    v = v * 1.0e-3
    v = np.concatenate([v, [[0.0, 0.0, 0.0], [1.0e3, 0.0, 0.0], [0.0, 1.0e3, 0.0]]])
    return v, np.concatenate([f[:30], [[62, 63, 64]], f[30:]])


def moved(mesh, seed):
    """The mesh scaled, turned a little and shifted: the plain parts of the case differ from one another."""
    rng = np.random.default_rng(seed)
    v, f = mesh
    a = rng.uniform(0, 2 * math.pi)
    rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return (v * rng.uniform(0.2, 3.0)) @ rz.T + rng.uniform(-2.0, 2.0, 3), f


def case_meshes():
    """Objects of 2, 5 and 20 parts.  Part numbers: 0 tetrahedron, 1 far cube | 2 icosphere, 3 one face, 4 zero-area faces, 5 huge
    and tiny, 6 F = 255 | 7 .. 9 F = 256, 257, 1300, the rest moved copies of the small meshes."""
    special = [tetrahedron(), cube(), icosphere(1), (np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 3.0, 1.0]]), np.array([[0, 1, 2]])),
               with_zero_area_faces(), one_huge_many_tiny(), strip(255, 1), strip(256, 2), strip(257, 3), strip(1300, 4)]
    plain = [tetrahedron(), cube(5.0), icosphere(0), icosphere(1)]
    parts = special + [moved(plain[k % 4], 100 + k) for k in range(sum(COUNTS) - len(special))]
    parts = [(np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)) for v, f in parts]
    out, lo = [], 0
    for n in COUNTS:
        out.append(parts[lo:lo + n])
        lo += n
    return out


_DRAWS = {}


def case_draws(N):
    """The fixed draws of the shared case at N points, made by the module under SEED (``u_face`` with exact zeros put in: the
    first pick of every part, and a whole row for part 4 whose first face has area 0)."""
    if N not in _DRAWS:
        from diffassemble_amd import fragment_batch as F
        u_face, u_len, rot_mats, point_perm, _, _ = F._draws(list(COUNTS), N, -1, False, 0, 0, torch.Generator().manual_seed(SEED + N))
        u_face = u_face.clone()
        u_face[:, 0] = 0.0
        u_face[4, ::2] = 0.0
        _DRAWS[N] = dict(u_face=u_face, u_len=u_len, rot_mats=rot_mats, point_perm=point_perm)
    return _DRAWS[N]


_HOST = {}


def host_batch(N):
    """The host route's Batch of the shared case (computed once per N, never modified)."""
    if N not in _HOST:
        from diffassemble_amd import make_batch3d
        _HOST[N] = make_batch3d(case_meshes(), num_points=N, category=["a", "b", "c"], data_id=[7, 8, 9], return_face_index=True,
                                **case_draws(N))
    return _HOST[N]


# non-finite vertices away from face 0: part -> (part, vertex, the first face that holds it).  Part 2 is the icosphere (F = 80),
# part 9 the strip of 1300 faces (vertex 700 lies in faces 698 .. 700: the third chunk of the scan), part 8 the strip of 257.
NONFINITE = {"mid": (2, 30, None), "late": (9, 700, 698), "inf": (8, 200, 198)}
_NONFINITE = {}


def nonfinite_meshes():
    meshes = case_meshes()
    flat = [p for obj in meshes for p in obj]
    for name, (s, vertex, _) in NONFINITE.items():
        flat[s][0][vertex, 1] = np.inf if name == "inf" else np.nan
    return meshes


def _first_face_with(s, vertex):
    f = [p for obj in case_meshes() for p in obj][s][1]
    return int(np.nonzero((f == vertex).any(1))[0][0])


NONFINITE["mid"] = (2, 30, _first_face_with(2, 30))
assert NONFINITE["mid"][2] > 0 and _first_face_with(9, 700) == 698 and _first_face_with(8, 200) == 198


def nonfinite_batch(N):
    """The host route's Batch of the shared case with the non-finite vertices put in."""
    if N not in _NONFINITE:
        from diffassemble_amd import make_batch3d
        with np.errstate(invalid="ignore"):                                 # numpy says that NaN went in
            _NONFINITE[N] = make_batch3d(nonfinite_meshes(), num_points=N, return_face_index=True, **case_draws(N))
    return _NONFINITE[N]


# ------------------------------------------------------------------------------------------------ the literal loop
def literal_sample_surface(vertices, faces, count, u_face, u_len):
    """The body of trimesh.sample.sample_surface with the two ``np.random.random`` calls replaced by the draws.  Face areas: half
    the norm of the cross product of the two edges from the first vertex."""
    tri = vertices[faces]
    crosses = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area_faces = np.sqrt((crosses ** 2).sum(axis=1)) / 2.0
    weight_cum = np.cumsum(area_faces)
    face_pick = u_face * weight_cum[-1]
    face_index = np.searchsorted(weight_cum, face_pick)
    face_index = np.minimum(face_index, len(faces) - 1)                       # a pick equal to the total (u = 1) stays inside
    tri_origins = vertices[faces[:, 0]]
    tri_vectors = vertices[faces[:, 1:]].copy()
    tri_vectors -= np.tile(tri_origins, (1, 2)).reshape((-1, 2, 3))
    tri_origins = tri_origins[face_index]
    tri_vectors = tri_vectors[face_index]
    random_lengths = u_len.reshape(count, 2, 1).copy()
    random_test = random_lengths.sum(axis=1).reshape(-1) > 1.0
    random_lengths[random_test] -= 1.0
    random_lengths = np.abs(random_lengths)
    sample_vector = (tri_vectors * random_lengths).sum(axis=1)
    return sample_vector + tri_origins, face_index


def literal_batch(meshes, N, max_num_part, u_face, u_len, rot_mats, point_perm, part_order=None, keep=None):
    """breakingbad_dt.__getitem__ and objects_dataset.get per object, then the collation; the draws by input part."""
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    xs, pcs, valids_all, edges, batch, lo, first = [], [], [], [], [], 0, 0
    for g, obj in enumerate(meshes):
        order = list(range(len(obj))) if part_order is None else list(part_order[g])
        cur_pts, cur_quat, cur_trans = [], [], []
        for k in order:
            s = lo + k
            pc, _ = literal_sample_surface(obj[k][0], obj[k][1], N, u_face[s], u_len[s])
            centroid = np.mean(pc, axis=0)                                   # _recenter_pc
            pc = pc - centroid[None]
            pc = (rot_mats[s] @ pc.T).T                                       # _rotate_pc
            quat_gt = Rotation.from_matrix(rot_mats[s].T).as_quat()[[3, 0, 1, 2]]
            cur_pts.append(pc[point_perm[s]])                                 # _shuffle_pc
            cur_quat.append(quat_gt)
            cur_trans.append(centroid)

        def pad(data):                                                        # _pad_data
            data = np.array(data)
            out = np.zeros((max_num_part,) + tuple(data.shape[1:]), dtype=np.float32)
            out[:data.shape[0]] = data
            return out

        part_pcs, part_quat, part_trans = pad(np.stack(cur_pts)), pad(np.stack(cur_quat)), pad(np.stack(cur_trans))
        valids = np.zeros(max_num_part, dtype=np.float32)
        valids[:len(obj)] = 1.0
        valids = torch.tensor(valids.astype(bool))                            # objects_dataset.get
        pcds = torch.tensor(part_pcs).permute(0, 2, 1)[valids].permute(0, 2, 1)
        target = torch.tensor(np.hstack((part_quat[valids], part_trans[valids])))
        if keep is not None:
            perm = list(keep[g])
            target, pcds = target[perm], pcds[perm]
            valids = torch.zeros(max_num_part, dtype=torch.bool)              # this project's choice: valids follows the kept parts
            valids[:len(perm)] = True
        n = target.shape[0]
        xs.append(target)
        pcs.append(pcds)
        valids_all.append(valids)
        edges.append(torch.ones(n, n).nonzero().t() + first)                  # dense_to_sparse(ones), shifted by the collation
        batch.append(torch.full((n,), g, dtype=torch.long))
        lo += len(obj)
        first += n
    return dict(x=torch.cat(xs), pcds=torch.cat(pcs), valids=torch.cat(valids_all), edge_index=torch.cat(edges, 1), batch=torch.cat(batch))


def np_draws(d):
    return {k: v.numpy() for k, v in d.items()}


@pytest.mark.parametrize("N", N_LIST)
def test_host_route_equals_the_literal_loop(N):
    got = host_batch(N)
    want = literal_batch(case_meshes(), N, 20, **np_draws(case_draws(N)))
    assert got.x.dtype == torch.float32 and got.x.shape == (27, 7) and got.pcds.dtype == torch.float32 and got.pcds.shape == (27, N, 3)
    assert torch.equal(got.x, want["x"]) and torch.equal(got.pcds, want["pcds"])                  # bit-equal
    assert got.valids.dtype == torch.bool and got.valids.shape == (60,) and torch.equal(got.valids, want["valids"])
    assert got.edge_index.dtype == torch.int64 and torch.equal(got.edge_index, want["edge_index"]) and got.edge_index.shape == (2, 4 + 25 + 400)
    assert got.batch.dtype == torch.int64 and torch.equal(got.batch, want["batch"])
    assert got.ptr.tolist() == [0, 2, 7, 27] and got.data_id.tolist() == [7, 8, 9] and got.data_id.dtype == torch.int64
    assert got.category == ["a", "b", "c"] and got.num_graphs == 3
    assert got.face_index.dtype == torch.int32 and got.face_index.shape == (27, N)
    assert bool(torch.isfinite(got.pcds).all()) and (N == 1 or float(got.pcds.abs().max()) > 0)         # one point: its own centroid
    if N >= 256:                                                               # the case reaches what it is there for
        fi = got.face_index
        assert int(fi[9].max()) > 1024 and int(fi[8].max()) >= 250 and set(fi[5].tolist()) == {0, 30}        # 0: the exact-zero pick
        assert fi[4, ::2].eq(0).all() and set(fi[4].tolist()).isdisjoint({5, 6, 12})              # faces of area 0 beyond the first: never


def test_host_route_with_shuffled_and_missing_parts_equals_the_literal_loop():
    from diffassemble_amd import make_batch3d
    N = 7
    order = [[1, 0], [4, 2, 0, 1, 3], list(range(19, -1, -1))]
    keep = [[1], [3, 0, 4], list(range(0, 20, 3))]
    got = make_batch3d(case_meshes(), num_points=N, part_order=order, keep=keep, **case_draws(N))
    want = literal_batch(case_meshes(), N, 20, part_order=order, keep=keep, **np_draws(case_draws(N)))
    for k in ("x", "pcds", "valids", "edge_index", "batch"):
        assert torch.equal(getattr(got, k), want[k]), k
    full = host_batch(N)
    assert torch.equal(got.pcds[0], full.pcds[0]) and torch.equal(got.pcds[1], full.pcds[2 + 1])  # part 0 of object 0; object 1: order[3] = 1
    assert got.ptr.tolist() == [0, 1, 4, 11] and got.valids.reshape(3, 20).sum(1).tolist() == [1, 3, 7]


def test_euler_turns_are_scipys_and_the_draw_order_is_the_documented_one():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    from diffassemble_amd import fragment_batch as F
    counts, N = [2, 3], 5
    u_face, u_len, rot_mats, point_perm, src, sel = F._draws(counts, N, 30.0, True, 40, 50, torch.Generator().manual_seed(3))
    gen = torch.Generator().manual_seed(3)
    assert torch.equal(u_face, torch.rand(5, N, dtype=torch.float64, generator=gen))
    assert torch.equal(u_len, torch.rand(5, N, 2, dtype=torch.float64, generator=gen))
    angles = (torch.rand(5, 3, dtype=torch.float64, generator=gen).numpy() - 0.5) * 2.0 * 30.0
    assert np.abs(angles).max() <= 30.0
    assert np.array_equal(rot_mats.numpy(), Rotation.from_euler("xyz", angles, degrees=True).as_matrix())
    assert torch.equal(point_perm, torch.rand(5, N, generator=gen).argsort(1))
    lo = 0
    for g, n in enumerate(counts):
        order = torch.randperm(n, generator=gen)
        kept = torch.randperm(n, generator=gen)[:n - math.ceil(n * 40 / 100)]
        assert src[g].tolist() == (lo + order[kept]).tolist()
        m = len(kept)
        assert sel[g].tolist() == torch.randperm(m * m, generator=gen)[:m * round(50 * (m - 1) / 100)].tolist()
        lo += n
    # without rot_range: the rotation of a normalised 4-vector of normals (uniform), as Rotation.random makes it
    _, _, rot_mats, _, _, _ = F._draws(counts, N, -1, False, 0, 0, torch.Generator().manual_seed(4))
    gen = torch.Generator().manual_seed(4)
    torch.rand(5, N, dtype=torch.float64, generator=gen), torch.rand(5, N, 2, dtype=torch.float64, generator=gen)
    q = torch.randn(5, 4, dtype=torch.float64, generator=gen).numpy()
    assert np.array_equal(rot_mats.numpy(), Rotation.from_quat(q).as_matrix())


# ------------------------------------------------------------------------------------------------ the quaternion routine
def test_matrix_to_quat_is_scipys_sign_included():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    from diffassemble_amd import fragment_batch as F
    rng = np.random.default_rng(11)
    mats = [Rotation.from_quat(rng.standard_normal((500, 4))).as_matrix()]
    axes = rng.standard_normal((40, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    mats.append(Rotation.from_rotvec(axes * math.pi).as_matrix())                                  # half turns about random axes
    mats.append(np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]))
    mats.append(Rotation.from_euler("xyz", [[90, 0, 0], [0, 90, 0], [0, 0, 90], [180, 90, 0], [120, 0, 0]], degrees=True).as_matrix())
    mats = np.concatenate(mats)
    got = F._matrix_to_quat(mats)
    want = Rotation.from_matrix(mats).as_quat()[:, [3, 0, 1, 2]]
    assert np.array_equal(np.signbit(got) & (got != 0), np.signbit(want) & (want != 0))
    assert np.array_equal(got, want)
    assert np.array_equal(got[540], [1.0, 0.0, 0.0, 0.0])                                           # the identity
    assert (want[:, 0] < 0).any()                                                                  # scipy does not canonicalise: neither do we


# ------------------------------------------------------------------------------------------------ missing, degree, valids
@pytest.mark.parametrize("missing", [0, 10, 30, 50])
def test_missing_counts_and_valids(missing):
    from diffassemble_amd import make_batch3d
    got = make_batch3d(case_meshes(), num_points=7, missing=missing, generator=torch.Generator().manual_seed(1))
    left = [n - math.ceil(n * missing / 100) for n in COUNTS]
    assert got.ptr.tolist() == [0] + np.cumsum(left).tolist() and got.x.shape[0] == got.pcds.shape[0] == sum(left)
    v = got.valids.reshape(3, 20)
    assert v.sum(1).tolist() == left and all(bool(v[g, :m].all()) for g, m in enumerate(left))
    assert got.edge_index.shape[1] == sum(m * m for m in left) and got.batch.tolist() == sum(([g] * m for g, m in enumerate(left)), [])


@pytest.mark.parametrize("degree", [10, 50, 100])
def test_degree_counts(degree):
    from diffassemble_amd import make_batch3d
    full = make_batch3d(case_meshes(), num_points=3, generator=torch.Generator().manual_seed(2))
    got = make_batch3d(case_meshes(), num_points=3, degree=degree, generator=torch.Generator().manual_seed(2))
    per = [n * round(degree * (n - 1) / 100) for n in COUNTS]
    assert got.edge_index.shape == (2, sum(per))
    lo = 0
    every = {tuple(e) for e in full.edge_index.t().tolist()}
    for g, m in enumerate(per):
        e = got.edge_index[:, lo:lo + m]
        assert bool((got.batch[e] == g).all())                                 # object g's edges, in its own block
        pairs = [tuple(p) for p in e.t().tolist()]
        assert len(set(pairs)) == m and set(pairs) <= every
        lo += m
    assert torch.equal(got.pcds, full.pcds) and torch.equal(got.x, full.x)      # the edge draw comes last: nothing else moves


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal():
    from diffassemble_amd import _lib, make_batch3d
    from diffassemble_amd import fragment_batch as F
    tet = (tetrahedron()[0], tetrahedron()[1])
    two = [[tet, tet]]

    def refused(match, meshes=two, **kw):
        kw.setdefault("num_points", 4)
        with pytest.raises(ValueError, match=match):
            make_batch3d(meshes, **kw)

    refused("outside", [[tet]])                                                # fewer than min_num_part
    refused("outside", [[tet] * 21])                                           # more than max_num_part
    refused("outside", [[tet] * 3], max_num_part=2)
    refused("outside its part", [[tet, (tet[0], np.array([[0, 1, 4]]))]])
    refused("outside its part", [[tet, (tet[0], np.array([[0, -1, 2]]))]])
    refused("fp64", [[tet, (tet[0].astype(np.float32), tet[1])]])
    refused("hold integers", [[tet, (tet[0], tet[1].astype(np.float64))]])
    refused(r"\[V, 3\]", [[tet, (tet[0][:, :2], tet[1])]])
    refused(r"\[F, 3\]", [[tet, (tet[0], tet[1][:, :2])]])
    refused("pair", [[tet, tet[0]]])
    refused("list of objects", "meshes")
    refused("no part", [])
    packed = dict(vertices=torch.from_numpy(np.concatenate([tet[0], tet[0]])), faces=torch.from_numpy(np.concatenate([tet[1], tet[1]])).int(),
                  vert_ptr=[0, 4, 8], face_ptr=[0, 4, 8], parts_per_object=[2])
    assert make_batch3d(packed, num_points=4).pcds.shape == (2, 4, 3)
    refused("int32", dict(packed, faces=packed["faces"].long()))
    refused("lacks", {k: v for k, v in packed.items() if k != "face_ptr"})
    refused("one entry per part", dict(packed, vert_ptr=[0, 8]))
    refused("at least one row", dict(packed, vert_ptr=[0, 8, 8]))
    refused("runs from 0", dict(packed, face_ptr=[0, 4, 7]))
    refused("outside its part", dict(packed, vert_ptr=[0, 5, 8]))              # part 1 has three vertices now
    refused("leaves no part", missing=100)
    refused("percentage", missing=-1)
    refused("percentage", degree=101)
    refused("above the kernel's limit", num_points=F.MAX_POINTS + 1)
    assert F.MAX_POINTS == 2048
    refused("positive integer", num_points=0)
    refused("positive integer", num_points=2.5)
    refused("positive integer", max_num_part=0)
    refused("'complete' or None", edges="ring")
    refused("needs edges", degree=50, edges=None)
    refused("one entry per object", category=["a", "b"])
    refused("one entry per object", data_id=[1, 2])
    refused(r"u_face is \[2, 4\]", u_face=torch.zeros(2, 5, dtype=torch.float64))
    refused("u_face is fp64", u_face=torch.zeros(2, 4))
    refused(r"u_len is \[2, 4, 2\]", u_len=torch.zeros(2, 4, dtype=torch.float64))
    refused(r"rot_mats is \[2, 3, 3\]", rot_mats=torch.zeros(2, 9, dtype=torch.float64))
    refused("point_perm holds integers", point_perm=torch.zeros(2, 4))
    refused("point_perm names points", point_perm=torch.tensor([[0, 1, 2, 4], [0, 1, 2, 3]]))
    refused("permutation", part_order=[[0, 0]])
    refused("one list per object", part_order=[[0, 1], [0, 1]])
    refused("repeats", keep=[[1, 1]])
    refused("names positions", keep=[[2]])
    refused("leaves no part", keep=[[]])
    refused("missing = 50 leaves 1", keep=[[0, 1]], missing=50)
    refused("edge_perm needs degree", edge_perm=[[0, 1, 2, 3]])
    refused("permutation", edge_perm=[[0, 1, 2, 2]], degree=100)
    with pytest.raises(_lib.DaError, match="ROCm device or the host"):
        make_batch3d(two, num_points=4, device="meta")


def test_documented_corner_cases_of_the_host_route():
    """A part of total area 0 samples face 0; non-finite vertices propagate into their part alone."""
    from diffassemble_amd import make_batch3d
    flat = (np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]), np.array([[0, 1, 2], [2, 1, 0]]))
    bad = (tetrahedron()[0].copy(), tetrahedron()[1])
    bad[0][2, 1] = np.nan
    got = make_batch3d([[flat, tetrahedron(), bad]], num_points=9, generator=torch.Generator().manual_seed(0), return_face_index=True)
    assert got.face_index[0].eq(0).all() and bool(torch.isfinite(got.pcds[:2]).all()) and bool(torch.isfinite(got.x[:2]).all())
    assert bool(torch.isnan(got.pcds[2]).any()) and bool(torch.isnan(got.x[2, 4:]).any()) and bool(torch.isfinite(got.x[2, :4]).all())
    want = nonfinite_batch(65)                                                 # NaN / Inf vertices away from face 0
    fi = want.face_index
    assert fi[NONFINITE["mid"][0]].eq(NONFINITE["mid"][2]).all() and fi[NONFINITE["late"][0]].eq(NONFINITE["late"][2]).all()
    for k in ("mid", "late"):
        s = NONFINITE[k][0]
        assert bool(torch.isnan(want.pcds[s]).all()) and bool(torch.isnan(want.x[s, 5]))       # the y of a vertex: the centroid's y
    s = NONFINITE["inf"][0]
    assert not bool(torch.isfinite(want.pcds[s]).any()) and int(fi[s].min()) >= NONFINITE["inf"][2]
    others = [k for k in range(27) if k not in {v[0] for v in NONFINITE.values()}]
    assert bool(torch.isfinite(want.pcds[others]).all()) and bool(torch.isfinite(want.x).all(1)[others].all())


# ------------------------------------------------------------------------------------------------ the margin condition
@pytest.mark.parametrize("N", N_LIST)
def test_no_pick_of_the_fixed_draws_lies_near_a_boundary(N):
    """Every pick lies at least 64 * F * 2^-53 * cum[-1] from every value of cum, except pick == 0 (exact on both sides).  Two
    fp64 sums of the same F non-negative areas in different orders differ by at most 2 (F - 1) 2^-53 cum[-1] in every prefix, and
    the pick itself moves by as much through cum[-1]: 64 F leaves a factor of 16.  So a face that differs on the GPU is a bug."""
    from diffassemble_amd import fragment_batch as F
    u_face = case_draws(N)["u_face"].numpy()
    parts = [p for obj in case_meshes() for p in obj]
    zeros = 0
    for s, (v, f) in enumerate(parts):
        cum = F._cum_area(v, f)
        assert cum[-1] > 0 and (np.diff(cum) >= 0).all()
        pick = u_face[s] * cum[-1]
        margin = 64 * len(f) * 2.0 ** -53 * cum[-1]
        gap = np.abs(pick[:, None] - cum[None, :]).min(1)
        assert (gap[pick != 0] >= margin).all(), (s, float(gap[pick != 0].min()), margin)
        zeros += int((pick == 0).sum())
    assert zeros >= len(parts)                                                 # the exact zeros are there


# ------------------------------------------------------------------------------------------------ ABI and module surface
def test_header_library_and_binding_carry_the_two_entry_points():
    from diffassemble_amd import _lib
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())
    assert ("int da_mesh_cum_area(int n_parts, const double *vertices, long long n_vertices, const int32_t *faces, long long n_faces, "
            "const long long *vert_ptr, const long long *face_ptr, double *cum, void *stream);") in text
    assert ("int da_fragment_batch(int n_out, int n_parts, int n_points, const double *vertices, long long n_vertices, const int32_t *faces, "
            "long long n_faces, const long long *vert_ptr, const long long *face_ptr, const double *cum, const int32_t *parts, "
            "const double *u_face, const double *u_len, const double *rot, const int32_t *perm, float *pcds, float *x, "
            "long long *batch, int32_t *face_index, void *stream);") in text
    doc = text.split("int da_mesh_cum_area(")[0][-3500:]
    for words in ("dataset/breakingbad_dt.py", ":113-149", "1 .. 2048", "clamped"):
        assert words in doc, words
    h = _lib.lib()
    for name, n_args in (("da_mesh_cum_area", 9), ("da_fragment_batch", 20)):
        assert getattr(h, name).argtypes == _lib.PROTOTYPES[name][1] and len(_lib.PROTOTYPES[name][1]) == n_args
    assert h.da_abi_version() == _lib.ABI_VERSION == 19                      # additive: the ABI number stays
    assert re.search(r"#define\s+DA_ABI_VERSION\s+19\b", open(os.path.join(ROOT, "include", "diffassemble_hip.h")).read())


def test_entry_points_check_their_arguments_before_launching():
    import ctypes as C
    from diffassemble_amd import _lib
    h = _lib.lib()
    one = C.c_void_p(1 << 20)                                                # never dereferenced: every call below is refused

    def cum(P=1, nv=3, nf=1, ptrs=(one,) * 5):
        vertices, faces, vert_ptr, face_ptr, out = ptrs
        return h.da_mesh_cum_area(P, vertices, nv, faces, nf, vert_ptr, face_ptr, out, None)

    def batch(n=1, P=1, N=4, nv=3, nf=1, ptrs=(one,) * 13, face_index=None):
        v, f, vp, fp, c, parts, uf, ul, rot, perm, pcds, x, b = ptrs
        return h.da_fragment_batch(n, P, N, v, nv, f, nf, vp, fp, c, parts, uf, ul, rot, perm, pcds, x, b, face_index, None)

    for k in range(5):
        assert cum(ptrs=tuple(None if i == k else one for i in range(5))) == 1 and b"null argument" in h.da_last_error(), k
    for kw in (dict(P=0), dict(nv=0), dict(nf=0), dict(P=-1)):
        assert cum(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    for k in range(13):
        assert batch(ptrs=tuple(None if i == k else one for i in range(13))) == 1 and b"null argument" in h.da_last_error(), k
    for kw in (dict(n=0), dict(P=0), dict(nv=0), dict(nf=-2)):
        assert batch(**kw) == 1 and b"bad sizes" in h.da_last_error(), kw
    for N in (0, -1, 2049, 1 << 20):
        assert batch(N=N) == 1 and b"n_points is 1 .. 2048" in h.da_last_error(), N
    assert batch(P=1 << 21, N=1024) == 1 and b"too large" in h.da_last_error()


def test_make_batch3d_is_exported_and_documents_its_differences():
    import diffassemble_amd
    from diffassemble_amd import fragment_batch as F
    assert diffassemble_amd.make_batch3d is F.make_batch3d and {"make_batch3d", "FragmentBatch"} <= set(diffassemble_amd.__all__)
    src = open(os.path.join(ROOT, "diffassemble_amd", "fragment_batch.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "import trimesh" not in src and "import scipy" not in src
    for words in ("``valids`` follows the kept parts", "torch's generator", "no bit-equality with it is claimed", "samples face 0",
                  "non-finite vertices propagate", "Mesh loading"):
        assert words in F.__doc__, words
    b = F.FragmentBatch(x=torch.zeros(2, 7), category=["a"], num_graphs=1)
    assert b.keys() == ["x", "category", "num_graphs"] and "x=[2, 7]" in repr(b) and b.to("cpu").category == ["a"]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3r" in design and "make_batch3d" in design and "trimesh" in design
