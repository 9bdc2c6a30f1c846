"""A 3D Batch from fragment meshes: sample every fragment's surface, centre, turn and shuffle the points, and lay out every
tensor the 3D modules read (host glue; runs once per Batch, before the encoder).  The 3D twin of puzzle_batch.py.

Counterpart of the reference's puzzle_diff/dataset/breakingbad_dt.py (:113-149: ``trimesh.sample.sample_surface`` of every
fragment mesh, ``_recenter_pc``, ``_rotate_pc``, ``_shuffle_pc``, ``_pad_data``) and dataset/objects_dataset.py (:174-225:
the valid parts, ``target = [quat | trans]``, ``missing``, ``degree``, the complete graph), followed by PyG's collation.  The
reference does all of it per part on the host in fp64 numpy.  The rule per part, in this project's words (everything in
fp64 until the final cast):

* the area of face (v0, v1, v2) is ``0.5 * |(v1 - v0) x (v2 - v0)|``; ``cum`` is the inclusive running sum of the areas;
* point i of N: ``pick = u_face[i] * cum[-1]``, the face is ``searchsorted(cum, pick)`` (left), clamped to ``F - 1``;
  ``(a, b) = u_len[i]``, and if ``a + b > 1`` then ``a, b = |a - 1|, |b - 1|``; ``point = v0 + a (v1 - v0) + b (v2 - v0)``;
* ``centroid`` = the mean of the N points, ``point <- point - centroid``, ``point <- rot_mat @ point``;
* output point j is point ``point_perm[j]``, cast to fp32;
* the part's row of ``x`` is fp32 of the scalar-first quaternion of ``rot_mat.T`` (scipy's ``from_matrix -> as_quat`` branch
  choice, sign included, in plain numpy: ``_matrix_to_quat``; the kernel repeats its operations), then fp32 of the centroid.

This is the published method of ``trimesh.sample.sample_surface`` (area-weighted face picking, then a uniform point of the
triangle).  trimesh is not a dependency and nothing here was compared with its outputs: no bit-equality with it is claimed.
Mesh loading (and trimesh itself) stays with the caller.

The draws.  Rows of ``u_face`` [P, N] fp64, ``u_len`` [P, N, 2] fp64, ``rot_mats`` [P, 3, 3] fp64 and ``point_perm`` [P, N]
belong to the P INPUT parts in input order, whatever ``shuffle_parts`` and ``missing`` do afterwards.  ``part_order``: per
object a permutation of its parts; ``keep``: per object the kept positions of that ordered list, in output order;
``edge_perm``: per object a permutation of its ``n * n`` complete edges.  A drawn ``point_perm`` row is a permutation of
0 .. N - 1; a handed-in one is used as a gather index list: values on the host are checked for their range, nothing checks that
they are distinct, and a repeated index repeats its point.  What is not handed in is drawn on the HOST with
torch under ``generator``, in this order: ``u_face = rand(P, N)``, ``u_len = rand(P, N, 2)``, the turns (``rand(P, 3)`` with
``rot_range > 0``: the extrinsic "xyz" Euler rotation of the angles ``(u - 0.5) * 2 * rot_range`` degrees; otherwise
``randn(P, 4)``: the rotation of that normalised quaternion, which is uniform), ``point_perm = rand(P, N).argsort(1)``, then
per object ``randperm(n)`` for ``shuffle_parts``, ``randperm(n)[:left]`` for ``missing`` and ``randperm(n * n)`` for
``degree``, each only when the option is on.  Draws are never made on the device.

Part selection.  ``missing`` keeps the head of a shuffled part list, ``n - ceil(n * missing / 100)`` parts; ``degree`` keeps
the first ``n * round(int(degree) * (n - 1) / 100)`` edges of the permuted complete edge list (one torch gather with
host-drawn indices, no kernel).

Differences from the reference, on purpose:

* ``valids`` follows the kept parts: with ``missing`` the reference leaves ``valids`` at the full part count while ``x`` and
  ``pcds`` are shortened (objects_dataset.py:184-191), and the losses need ``valids`` to mark exactly the rows of ``x``;
* the draws come from torch's generator (above), not from ``np.random`` / ``random``, and a part's draws do not depend on
  the order the parts end up in;
* a part whose total area is 0 samples face 0 (trimesh would too: every pick is 0); non-finite vertices propagate into the
  part's points and centroid on both routes (a NaN pick finds the first NaN of ``cum``, as ``numpy.searchsorted`` orders it),
  nothing is raised.

``make_batch3d`` on a ROCm device is three library calls (``da_mesh_cum_area``, ``da_fragment_batch``,
diffassemble_amd/csrc/da_fragment_batch.hip, DESIGN 3r, and ``da_complete_edges``) after one upload of the small tables, one
of every draw that lies on the host, and one of the meshes when they lie on the host.  For host input without ``device`` it
is ``_loop_batch3d``, the per-part route in fp64 numpy in the reference's order of operations: the contract the kernels are
tested against.  A Batch of CPU tensors is a reasonable thing to ask for, and the rule that kernels have no fallback concerns
the model's arithmetic."""
import math

import numpy as np
import torch

from .puzzle_batch import MAX_EDGE_BYTES, _complete_edges_host, _int_array

MAX_POINTS = 2048           # 24 * N bytes of LDS for the fp64 points + 6 KiB of reduction scratch <= the 64 KiB a launch gets unasked
_WHO = "make_batch3d"


class FragmentBatch:
    """What ``make_batch3d`` returns: a plain attribute object with ``x`` fp32 [n, 7], ``pcds`` fp32 [n, N, 3], ``valids`` bool
    [G * max_num_part], ``edge_index`` int64 [2, E] (absent with ``edges=None``), ``batch`` int64 [n], ``ptr`` int64 [G + 1],
    ``data_id`` int64 [G], ``category`` (a list) and ``num_graphs``; ``face_index`` int32 [n, N] (the sampled faces, in
    sampling order) on request.  Further attributes may be assigned freely."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def keys(self):
        return list(self.__dict__)

    def to(self, device):
        return FragmentBatch(**{k: v.to(device) if torch.is_tensor(v) else v for k, v in self.__dict__.items()})

    def __repr__(self):
        body = ", ".join(f"{k}={list(v.shape)}" if torch.is_tensor(v) else f"{k}={v!r}" for k, v in self.__dict__.items())
        return f"FragmentBatch({body})"


# ------------------------------------------------------------------------------------------------ rotations, plain numpy
def _matrix_of(q):
    """[P, 4] scalar-last quaternions, taken as they are -> [P, 3, 3] (the expressions of scipy's ``as_matrix``)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.empty((len(q), 3, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2
    return m


def _quat_to_matrix(q):
    """[P, 4] scalar-LAST quaternions (any length) -> [P, 3, 3], scipy's ``Rotation(q).as_matrix()`` operation for operation."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    return _matrix_of(q)


def _euler_xyz_to_matrix(deg):
    """[P, 3] angles in degrees -> [P, 3, 3] of the extrinsic "xyz" rotation (``Rotation.from_euler("xyz", deg, degrees=True)``):
    the elementary quaternions composed as scipy composes them; the product is not normalised again, as there."""
    a = np.deg2rad(np.asarray(deg, np.float64))
    q = None
    for ax in range(3):
        p = np.zeros((len(a), 4))
        p[:, ax], p[:, 3] = np.sin(a[:, ax] / 2), np.cos(a[:, ax] / 2)
        if q is None:
            q = p
            continue
        cr = (p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0])
        q = np.stack([p[:, 3] * q[:, 0] + q[:, 3] * p[:, 0] + cr[0], p[:, 3] * q[:, 1] + q[:, 3] * p[:, 1] + cr[1],
                      p[:, 3] * q[:, 2] + q[:, 3] * p[:, 2] + cr[2],
                      p[:, 3] * q[:, 3] - p[:, 0] * q[:, 0] - p[:, 1] * q[:, 1] - p[:, 2] * q[:, 2]], 1)
    return _matrix_of(q)


def _matrix_to_quat(m):
    """[P, 3, 3] rotation matrices -> [P, 4] SCALAR-FIRST unit quaternions: ``Rotation.from_matrix(m).as_quat()[[3, 0, 1, 2]]``
    with scipy's branch choice (the largest of the diagonal and the trace; the first of equals) and therefore its sign.  The
    matrices are taken as orthogonal (scipy re-orthogonalises those that are not)."""
    m = np.asarray(m, np.float64)
    d = np.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2], m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]], 1)
    choice = d.argmax(1)
    q = np.empty((len(m), 4))
    for i in range(3):
        a, j, k = m[choice == i], (i + 1) % 3, (i + 2) % 3
        q[choice == i, i] = 1 - d[choice == i, 3] + 2 * a[:, i, i]
        q[choice == i, j] = a[:, j, i] + a[:, i, j]
        q[choice == i, k] = a[:, k, i] + a[:, i, k]
        q[choice == i, 3] = a[:, k, j] - a[:, j, k]
    a = m[choice == 3]
    q[choice == 3] = np.stack([a[:, 2, 1] - a[:, 1, 2], a[:, 0, 2] - a[:, 2, 0], a[:, 1, 0] - a[:, 0, 1], 1 + d[choice == 3, 3]], 1)
    q = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    return q[:, [3, 0, 1, 2]]


# ------------------------------------------------------------------------------------------------ the contract: one part on the host
def _cum_area(v, f):
    """fp64 inclusive running sum of the face areas of one part (``v`` [V, 3] fp64, ``f`` [F, 3] integers)."""
    v0 = v[f[:, 0]]
    c = np.cross(v[f[:, 1]] - v0, v[f[:, 2]] - v0)
    return np.cumsum(np.sqrt((c * c).sum(1)) * 0.5)


def _sample_part(v, f, u_face, u_len):
    """The N surface points of one part, fp64 [N, 3], and their faces: the rule of the module docstring in the order of
    ``trimesh.sample.sample_surface``."""
    cum = _cum_area(v, f)
    pick = u_face * cum[-1]
    idx = np.minimum(np.searchsorted(cum, pick), len(f) - 1)
    origin = v[f[:, 0]]
    vectors = np.stack([v[f[:, 1]] - origin, v[f[:, 2]] - origin], 1)[idx]           # [N, 2, 3]
    lengths = np.array(u_len, np.float64).reshape(-1, 2, 1)
    flip = lengths.sum(1).reshape(-1) > 1.0
    lengths[flip] -= 1.0
    lengths = np.abs(lengths)
    return (vectors * lengths).sum(1) + origin[idx], idx


def _loop_batch3d(vertices, faces, vert_ptr, face_ptr, src, u_face, u_len, rot_mats, point_perm):
    """The per-part host route: numpy ``vertices`` fp64 [sum V, 3], ``faces`` [sum F, 3] (local indices) and their part offsets,
    ``src`` the input part of every output part, the draws by input part.  Every step is the reference's, in its order:
    sample_surface, ``_recenter_pc``, ``_rotate_pc``, ``_shuffle_pc``, the fp32 cast of ``_pad_data``.  Returns (x fp32 [n, 7],
    pcds fp32 [n, N, 3], face_index int32 [n, N])."""
    xs, ps, fs = [], [], []
    for s in src:
        v, f = vertices[vert_ptr[s]:vert_ptr[s + 1]], faces[face_ptr[s]:face_ptr[s + 1]]
        pc, idx = _sample_part(v, f, u_face[s], u_len[s])
        centroid = np.mean(pc, axis=0)
        pc = pc - centroid[None]
        pc = (rot_mats[s] @ pc.T).T
        pc = pc[point_perm[s]]
        quat = _matrix_to_quat(rot_mats[s].T[None])[0]
        ps.append(pc.astype(np.float32))
        xs.append(np.hstack((quat.astype(np.float32), centroid.astype(np.float32))))
        fs.append(idx.astype(np.int32))
    return torch.from_numpy(np.stack(xs)), torch.from_numpy(np.stack(ps)), torch.from_numpy(np.stack(fs))


# ------------------------------------------------------------------------------------------------ arguments
def _tensor(a, what):
    if torch.is_tensor(a):
        return a.detach()
    try:
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    except TypeError as e:
        raise ValueError(f"{_WHO}: {what} is an array or a tensor (got {type(a).__name__})") from e


def _meshes(meshes):
    """-> (vertices fp64 [sum V, 3] tensor, faces int32 [sum F, 3] tensor, vert_ptr, face_ptr (numpy int64 [P + 1]), parts per
    object) from either input form.  The two big tensors stay on the device they lie on."""
    if isinstance(meshes, dict):
        missing = [k for k in ("vertices", "faces", "vert_ptr", "face_ptr", "parts_per_object") if k not in meshes]
        if missing:
            raise ValueError(f"{_WHO}: the packed form lacks {missing}")
        vertices, faces = _tensor(meshes["vertices"], "vertices"), _tensor(meshes["faces"], "faces")
        if faces.dtype != torch.int32:
            raise ValueError(f"{_WHO}: packed faces are int32 [sum F, 3] (got {faces.dtype})")
        vert_ptr, face_ptr = _int_array(meshes["vert_ptr"], "vert_ptr"), _int_array(meshes["face_ptr"], "face_ptr")
        counts = _int_array(meshes["parts_per_object"], "parts_per_object").tolist()
    else:
        if isinstance(meshes, (str, bytes)) or not hasattr(meshes, "__len__"):
            raise ValueError(f"{_WHO}: meshes is a list of objects (each a list of (vertices, faces)) or the packed dict")
        vs, fs, counts = [], [], []
        for g, obj in enumerate(meshes):
            if isinstance(obj, (str, bytes, dict)) or torch.is_tensor(obj) or isinstance(obj, np.ndarray) or not hasattr(obj, "__len__"):
                raise ValueError(f"{_WHO}: object {g} is a list of (vertices, faces) pairs")
            counts.append(len(obj))
            for k, part in enumerate(obj):
                if torch.is_tensor(part) or isinstance(part, np.ndarray) or not hasattr(part, "__len__") or len(part) != 2:
                    raise ValueError(f"{_WHO}: part {k} of object {g} is a (vertices, faces) pair")
                v, f = _tensor(part[0], "vertices"), _tensor(part[1], "faces")
                if f.is_floating_point() or f.is_complex() or f.dtype == torch.bool:
                    raise ValueError(f"{_WHO}: the faces of part {k} of object {g} hold integers (got {f.dtype})")
                if v.dim() != 2 or f.dim() != 2:
                    raise ValueError(f"{_WHO}: part {k} of object {g} is (vertices [V, 3], faces [F, 3]) (got {tuple(v.shape)}, {tuple(f.shape)})")
                vs.append(v)
                fs.append(f.to(torch.int32))
        if not vs:
            raise ValueError(f"{_WHO}: no part")
        vert_ptr = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
        face_ptr = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
        if any(v.dtype != torch.float64 for v in vs):
            raise ValueError(f"{_WHO}: vertices are fp64 [V, 3] (got {sorted({str(v.dtype) for v in vs})})")
        if any(v.shape[1:] != (3,) for v in vs) or any(f.shape[1:] != (3,) for f in fs):
            raise ValueError(f"{_WHO}: every part is (vertices [V, 3], faces [F, 3])")
        dev = next((t.device for t in vs + fs if t.device.type != "cpu"), torch.device("cpu"))
        vertices, faces = torch.cat([v.to(dev) for v in vs]), torch.cat([f.to(dev) for f in fs])
    if vertices.dtype != torch.float64 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{_WHO}: vertices are fp64 [sum V, 3] (got {vertices.dtype} {tuple(vertices.shape)})")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{_WHO}: faces are int32 [sum F, 3] (got {tuple(faces.shape)})")
    P = sum(counts)
    if not counts or min(counts) < 0 or len(vert_ptr) != P + 1 or len(face_ptr) != P + 1:
        raise ValueError(f"{_WHO}: vert_ptr and face_ptr have one entry per part and one more, {P + 1} here "
                         f"(got {len(vert_ptr)}, {len(face_ptr)})")
    for name, ptr, total in (("vert_ptr", vert_ptr, len(vertices)), ("face_ptr", face_ptr, len(faces))):
        if ptr[0] != 0 or ptr[-1] != total or (np.diff(ptr) < 1).any():
            raise ValueError(f"{_WHO}: {name} runs from 0 to {total} and gives every part at least one row")
    if faces.device.type == "cpu":
        f = faces.numpy()
        limit = np.repeat(np.diff(vert_ptr), np.diff(face_ptr))[:, None]
        if ((f < 0) | (f >= limit)).any():
            bad = int(np.nonzero(((f < 0) | (f >= limit)).any(1))[0][0])
            raise ValueError(f"{_WHO}: face {bad} names a vertex outside its part (indices are local to the part)")
    return vertices.contiguous(), faces.contiguous(), vert_ptr, face_ptr, counts


def _draw(v, shape, what, integer=False):
    """A handed-in draw as a tensor of the given shape (on whatever device it lies): fp64, or integers."""
    t = _tensor(v, what)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{_WHO}: {what} is {list(shape)} (got {list(t.shape)})")
    if integer:
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{_WHO}: {what} holds integers (got {t.dtype})")
    elif t.dtype != torch.float64:
        raise ValueError(f"{_WHO}: {what} is fp64 (got {t.dtype})")
    return t


def _per_object(v, G, what):
    if v is not None and (isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != G):
        raise ValueError(f"{_WHO}: {what} is one list per object, {G} here")
    return v


def _perm_of(v, n, what):
    p = _int_array(v, what)
    if len(p) != n or not np.array_equal(np.sort(p), np.arange(n)):
        raise ValueError(f"{_WHO}: {what} is a permutation of 0 .. {n - 1}")
    return p


def _n_connections(n, degree):
    return int(n * round((int(degree) * (n - 1)) / 100))


def _draws(counts, N, rot_range, shuffle_parts, missing, degree, generator, u_face=None, u_len=None, rot_mats=None, point_perm=None,
           part_order=None, keep=None, edge_perm=None):
    """Everything random, in the documented order.  -> (u_face, u_len, rot_mats, point_perm: tensors by input part;
    src: per object the input parts of its output parts (global numbers); edge_sel: per object the kept edges' numbers within the
    object's complete list, or None)."""
    G, P = len(counts), sum(counts)
    if not 0 <= missing <= 100:
        raise ValueError(f"{_WHO}: missing is a percentage 0 .. 100 (got {missing})")
    if not 0 <= degree <= 100:
        raise ValueError(f"{_WHO}: degree is a percentage 0 .. 100 (got {degree})")
    part_order, keep, edge_perm = _per_object(part_order, G, "part_order"), _per_object(keep, G, "keep"), _per_object(edge_perm, G, "edge_perm")
    if edge_perm is not None and not degree > 0:
        raise ValueError(f"{_WHO}: edge_perm needs degree > 0")
    u_face = torch.rand(P, N, dtype=torch.float64, generator=generator) if u_face is None else _draw(u_face, (P, N), "u_face")
    u_len = torch.rand(P, N, 2, dtype=torch.float64, generator=generator) if u_len is None else _draw(u_len, (P, N, 2), "u_len")
    if rot_mats is not None:
        rot_mats = _draw(rot_mats, (P, 3, 3), "rot_mats")
    elif rot_range > 0:
        u = torch.rand(P, 3, dtype=torch.float64, generator=generator).numpy()
        rot_mats = torch.from_numpy(_euler_xyz_to_matrix((u - 0.5) * 2.0 * rot_range))
    else:
        rot_mats = torch.from_numpy(_quat_to_matrix(torch.randn(P, 4, dtype=torch.float64, generator=generator).numpy()))
    if point_perm is None:
        point_perm = torch.rand(P, N, generator=generator).argsort(1)
    else:
        point_perm = _draw(point_perm, (P, N), "point_perm", integer=True)
        if point_perm.device.type == "cpu" and bool(((point_perm < 0) | (point_perm >= N)).any()):
            raise ValueError(f"{_WHO}: point_perm names points 0 .. {N - 1}")
    src, edge_sel, lo = [], [], 0
    for g, n in enumerate(counts):
        if part_order is not None:
            order = _perm_of(part_order[g], n, f"part_order[{g}]")
        elif shuffle_parts:
            order = torch.randperm(n, generator=generator).numpy()
        else:
            order = np.arange(n)
        left = n - math.ceil(n * missing / 100)
        if left < 1:
            raise ValueError(f"{_WHO}: missing = {missing} leaves no part of object {g} ({n} parts)")
        if keep is not None:
            kg = _int_array(keep[g], f"keep[{g}]")
            if ((kg < 0) | (kg >= n)).any():
                raise ValueError(f"{_WHO}: keep[{g}] names positions 0 .. {n - 1} of the object's {n} parts")
            if len(np.unique(kg)) != len(kg):
                raise ValueError(f"{_WHO}: keep[{g}] repeats a part")
            if not len(kg):
                raise ValueError(f"{_WHO}: keep[{g}] leaves no part of object {g}")
            if missing and len(kg) != left:
                raise ValueError(f"{_WHO}: keep[{g}] has {len(kg)} parts, missing = {missing} leaves {left} of {n}")
        elif left < n:
            kg = torch.randperm(n, generator=generator)[:left].numpy()
        else:
            kg = np.arange(n)
        src.append(lo + order[kg])
        m = len(kg)
        if degree > 0:
            ep = _perm_of(edge_perm[g], m * m, f"edge_perm[{g}]") if edge_perm is not None else torch.randperm(m * m, generator=generator).numpy()
            edge_sel.append(ep[:_n_connections(m, degree)])
        lo += n
    return u_face, u_len, rot_mats, point_perm, src, (edge_sel if degree > 0 else None)


_TORCH_OF = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
             np.dtype(np.float64): torch.float64, np.dtype(np.bool_): torch.bool}


def _tables(vert_ptr, face_ptr, src, rot_mats, max_num_part, data_id):
    """Everything small the device route needs as ONE host buffer, and the byte range, dtype and shape of every part.  int64:
    vert_ptr, face_ptr [P + 1], the edge table [G, 3], ptr [G + 1], data_id [G]; fp64: the turns [P, 9] (``rot_mats`` numpy, or None
    when they lie on the device already); int32: parts [n, 2] (input part, object); bool: valids [G * max_num_part]."""
    G = len(src)
    counts = [len(s) for s in src]
    n = sum(counts)
    edge, ptr = np.zeros((G, 3), np.int64), np.zeros(G + 1, np.int64)
    parts = np.zeros((n, 2), np.int32)
    valids = np.zeros((G, max_num_part), np.bool_)
    e0 = 0
    for g, m in enumerate(counts):
        edge[g] = (e0, ptr[g], m)
        ptr[g + 1] = ptr[g] + m
        parts[ptr[g]:ptr[g + 1], 0], parts[ptr[g]:ptr[g + 1], 1] = src[g], g
        valids[g, :m] = True
        e0 += m * m
    named = [("vert_ptr", np.asarray(vert_ptr, np.int64)), ("face_ptr", np.asarray(face_ptr, np.int64)), ("edge", edge), ("ptr", ptr),
             ("data_id", np.asarray(data_id, np.int64)), ("parts", parts), ("valids", valids.reshape(-1))]
    if rot_mats is not None:
        named.insert(5, ("rot", np.ascontiguousarray(rot_mats, np.float64).reshape(-1, 9)))
    where, size = {}, 0
    for name, arr in named:
        size = (size + 15) & ~15
        where[name] = (size, size + arr.nbytes, arr.dtype, arr.shape)
        size += arr.nbytes
    buf = np.zeros(size, np.uint8)
    for name, arr in named:
        a, b = where[name][:2]
        buf[a:b] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    return buf, where, n, e0


def make_batch3d(meshes, *, num_points=1000, max_num_part=20, min_num_part=2, rot_range=-1, shuffle_parts=False, missing=0, degree=0,
                 category=None, data_id=None, generator=None, edges="complete", device=None, u_face=None, u_len=None, rot_mats=None,
                 point_perm=None, part_order=None, keep=None, edge_perm=None, return_face_index=False):
    """The Batch of G objects from the meshes of their fragments (see the module docstring for the rule, the draws and the
    differences from the reference).

    ``meshes``: a list of G objects, each a list of ``(vertices fp64 [V, 3], faces int [F, 3])`` arrays or tensors, or the packed
    dict ``vertices`` fp64 [sum V, 3], ``faces`` int32 [sum F, 3] (indices local to the part), ``vert_ptr`` / ``face_ptr`` [P + 1],
    ``parts_per_object`` [G]; on the host or on the device.  ``num_points`` (at most ``MAX_POINTS``), ``max_num_part``,
    ``min_num_part``, ``rot_range``, ``shuffle_parts`` are the reference's ``GeometryPartDataset`` arguments, ``missing`` and
    ``degree`` (percentages) its ``Objects_Dataset`` ones.  ``category``: G strings, ``data_id``: G integers (default 0 .. G - 1).
    ``u_face``, ``u_len``, ``rot_mats``, ``point_perm``, ``part_order``, ``keep``, ``edge_perm``: the draws; what is not given is drawn
    on the host under ``generator``.  ``edges``: ``"complete"`` or None (no ``edge_index``: attach your own graph).  ``device``:
    where the Batch is built; default: where the meshes lie.  ``return_face_index``: also return the sampled faces.
    Anything wrong raises ``ValueError``; a device that is neither ROCm nor the host raises ``DaError``."""
    for name, v in (("num_points", num_points), ("max_num_part", max_num_part), ("min_num_part", min_num_part)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{_WHO}: {name} is a positive integer (got {v!r})")
    N = int(num_points)
    if N > MAX_POINTS:
        raise ValueError(f"{_WHO}: num_points = {N} is above the kernel's limit of {MAX_POINTS} (24 bytes of LDS per point)")
    if edges not in ("complete", None):
        raise ValueError(f"{_WHO}: edges is 'complete' or None (got {edges!r})")
    if degree > 0 and edges is None:
        raise ValueError(f"{_WHO}: degree thins the complete graph and needs edges='complete'")
    vertices, faces, vert_ptr, face_ptr, counts = _meshes(meshes)
    G = len(counts)
    for g, n in enumerate(counts):
        if not min_num_part <= n <= max_num_part:
            raise ValueError(f"{_WHO}: object {g} has {n} parts, outside [{min_num_part}, {max_num_part}]")
    category = [None] * G if category is None else list(category)
    ids = list(range(G)) if data_id is None else _int_array(data_id, "data_id").tolist()
    if len(category) != G or len(ids) != G:
        raise ValueError(f"{_WHO}: category and data_id have one entry per object, {G} here (got {len(category)}, {len(ids)})")
    u_face, u_len, rot_mats, point_perm, src, edge_sel = _draws(counts, N, rot_range, bool(shuffle_parts), missing, degree, generator, u_face,
                                                                u_len, rot_mats, point_perm, part_order, keep, edge_perm)
    kept = [len(s) for s in src]
    n_edges = sum(m * m for m in kept)
    if edges == "complete" and 16 * n_edges > MAX_EDGE_BYTES:
        raise ValueError(f"{_WHO}: the complete graphs have {n_edges} edges = {16 * n_edges} bytes of edge_index, above {MAX_EDGE_BYTES}: "
                         "pass edges=None and attach a sparser graph yourself")
    dev = torch.device(device) if device is not None else vertices.device
    if dev.type not in ("cpu", "cuda"):
        from . import _lib
        raise _lib.DaError(f"make_batch3d needs a ROCm device or the host (got {dev})")
    if edge_sel is not None:
        first = np.concatenate([[0], np.cumsum([m * m for m in kept])])
        edge_sel = torch.from_numpy(np.concatenate([first[g] + e for g, e in enumerate(edge_sel)]).astype(np.int64))
    flat_src = np.concatenate(src)
    if dev.type == "cpu":
        x, pcds, face_index = _loop_batch3d(vertices.cpu().numpy(), faces.cpu().numpy(), vert_ptr, face_ptr, flat_src, u_face.cpu().numpy(),
                                            u_len.cpu().numpy(), rot_mats.cpu().numpy(), point_perm.cpu().numpy())
        out = FragmentBatch(x=x, pcds=pcds)
        valids = torch.zeros(G, max_num_part, dtype=torch.bool)
        for g, m in enumerate(kept):
            valids[g, :m] = True
        out.valids = valids.reshape(-1)
        if edges == "complete":
            out.edge_index = _complete_edges_host(kept)
            if edge_sel is not None:
                out.edge_index = out.edge_index[:, edge_sel]
        out.batch = torch.repeat_interleave(torch.arange(G), torch.tensor(kept))
        out.ptr = torch.tensor(np.concatenate([[0], np.cumsum(kept)]), dtype=torch.long)
        out.data_id = torch.tensor(ids, dtype=torch.long)
    else:
        from . import _lib
        rot_on_host = rot_mats.device.type == "cpu"                       # turns on the device are read where they lie: no copy back
        host, where, n, E = _tables(vert_ptr, face_ptr, src, rot_mats.numpy() if rot_on_host else None, max_num_part, ids)
        small = torch.from_numpy(host).to(dev)                                                         # one copy of the tables

        def part(name):
            a, b, dtype, shape = where[name]
            return small[a:b].view(_TORCH_OF[dtype]).view(shape)

        vertices, faces = vertices.to(dev), faces.to(dev)
        u_face, u_len, perm = u_face.to(dev).contiguous(), u_len.to(dev).contiguous(), point_perm.to(dev).to(torch.int32).contiguous()
        rot = part("rot") if rot_on_host else rot_mats.to(dev).contiguous()
        cum = torch.empty(len(faces), dtype=torch.float64, device=dev)
        pcds = torch.empty((n, N, 3), dtype=torch.float32, device=dev)
        x = torch.empty((n, 7), dtype=torch.float32, device=dev)
        bvec = torch.empty(n, dtype=torch.long, device=dev)
        face_index = torch.empty((n, N), dtype=torch.int32, device=dev) if return_face_index else None
        out = FragmentBatch(x=x, pcds=pcds, valids=part("valids"))
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            h = _lib.lib()
            _lib.check(h.da_mesh_cum_area(len(vert_ptr) - 1, _lib.ptr(vertices), len(vertices), _lib.ptr(faces), len(faces),
                                          _lib.ptr(part("vert_ptr")), _lib.ptr(part("face_ptr")), _lib.ptr(cum), st))
            _lib.check(h.da_fragment_batch(n, len(vert_ptr) - 1, N, _lib.ptr(vertices), len(vertices), _lib.ptr(faces), len(faces),
                                           _lib.ptr(part("vert_ptr")), _lib.ptr(part("face_ptr")), _lib.ptr(cum), _lib.ptr(part("parts")),
                                           _lib.ptr(u_face), _lib.ptr(u_len), _lib.ptr(rot), _lib.ptr(perm),
                                           _lib.ptr(pcds), _lib.ptr(x), _lib.ptr(bvec), _lib.ptr(face_index), st))
            if edges == "complete":
                out.edge_index = torch.empty((2, E), dtype=torch.long, device=dev)
                _lib.check(h.da_complete_edges(G, _lib.ptr(part("edge")), E, _lib.ptr(out.edge_index), st))
                if edge_sel is not None:
                    out.edge_index = out.edge_index[:, edge_sel.to(dev)]
        out.batch, out.ptr, out.data_id = bvec, part("ptr"), part("data_id")
    if return_face_index:
        out.face_index = face_index
    out.category, out.num_graphs = category, G
    return out
