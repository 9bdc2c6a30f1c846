"""Timing of the 3D Batch builder (diffassemble_amd/fragment_batch.py, csrc/da_fragment_batch.hip): 32 objects x 20 parts x 1000
points, on meshes generated here: 320, 1 280 and 2 000 faces per part (``--faces``: any count; 20 * 4^k gives a closed subdivided
icosahedron pushed out of round and moved, any other count a strip of triangles (i, i + 1, i + 2) over random vertices); the
draws are made once and handed in.

Arms, each after 5 warm-ups, median of the repetitions:
  make_batch3d       the whole call, meshes and draws already on the device, host clock between two device synchronisations: the
                     tables made on the host, their one upload, the three launches
  make_batch3d_host  the same call with meshes and draws on the host and ``device=``: + the upload of the draws (26 bytes per
                     point) and of the meshes
  da_mesh_cum_area   the first launch alone, everything prepared, device events around it
  da_fragment_batch  the second launch alone (no ``face_index``), likewise
  copy               ``Tensor.copy_`` of as many bytes as the second launch writes into ``pcds``, device to device, same process
  _loop_batch3d      the per-part host route (what ``make_batch3d`` does for CPU meshes, and what the reference's dataset does),
                     timed on ``--host-objects`` objects and scaled to the Batch
The device Batch must agree with the host route's on those objects first (faces equal, points within the test suite's bound).
``da_fragment_batch`` READS more than it writes (26 bytes of draws per point against 12 written, and the faces it samples), so
the copy of the bytes written is a floor it is not expected to reach; ``read_write_bytes`` is the sum.  One JSON line per shape.

    python tests/tools/fragment_batch_bench.py [--reps 30] [--objects 32] [--parts 20] [--points 1000] [--faces 320 1280 2000]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffassemble_amd import _lib, make_batch3d  # noqa: E402
from diffassemble_amd import fragment_batch as F  # noqa: E402

WARMUP = 5


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def host_timed(fn, reps, warmup=WARMUP, sync=True):
    ms = []
    for rep in range(warmup + reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        if rep >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def event_timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for rep in range(WARMUP + reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if rep >= WARMUP:
            ms.append(ev[0].elapsed_time(ev[1]))
    return stats(ms)


def icosphere(levels):
    g = (1 + 5 ** 0.5) / 2
    v = [np.array(p, np.float64) for p in ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                                           (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    v = [p / np.sqrt((p * p).sum()) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
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
    return np.array(v), np.array(f, np.int32)


def make_meshes(G, parts, faces, seed=0):
    levels = {20 * 4 ** k: k for k in range(6)}.get(faces)
    rng = np.random.default_rng(seed)
    if levels is not None:
        v0, f = icosphere(levels)
    else:                                          # any face count: a strip over random vertices near the unit sphere
        v0 = rng.standard_normal((faces + 2, 3))
        v0 /= np.sqrt((v0 * v0).sum(1, keepdims=True))
        i = np.arange(faces, dtype=np.int32)
        f = np.stack([i, i + 1, i + 2], 1)
    out = []
    for _ in range(G):
        out.append([((v0 * rng.uniform(0.5, 1.5, 3) * (1 + 0.2 * rng.standard_normal((len(v0), 1)))) * 0.2 + rng.uniform(-0.5, 0.5, 3), f)
                    for _ in range(parts)])
    return out


def pack(meshes, dev):
    flat = [p for obj in meshes for p in obj]
    return dict(vertices=torch.from_numpy(np.concatenate([v for v, _ in flat])).to(dev),
                faces=torch.from_numpy(np.concatenate([f for _, f in flat]).astype(np.int32)).to(dev),
                vert_ptr=np.concatenate([[0], np.cumsum([len(v) for v, _ in flat])]), face_ptr=np.concatenate([[0], np.cumsum([len(f) for _, f in flat])]),
                parts_per_object=[len(obj) for obj in meshes])


def launches_alone(packed, draws, N, dev, reps):
    """The two launches through the C ABI with the tables prepared (all parts present, input order)."""
    counts = packed["parts_per_object"]
    P = sum(counts)
    src, lo = [], 0
    for n in counts:
        src.append(np.arange(lo, lo + n))
        lo += n
    host, where, n_out, _ = F._tables(packed["vert_ptr"], packed["face_ptr"], src, None, max(counts), list(range(len(counts))))
    small = torch.from_numpy(host).to(dev)

    def part(name):
        a, b, dtype, shape = where[name]
        return small[a:b].view(F._TORCH_OF[dtype]).view(shape)

    v, f = packed["vertices"], packed["faces"]
    cum = torch.empty(len(f), dtype=torch.float64, device=dev)
    pcds = torch.empty((n_out, N, 3), device=dev)
    x = torch.empty((n_out, 7), device=dev)
    bv = torch.empty(n_out, dtype=torch.long, device=dev)
    perm = draws["point_perm"].to(torch.int32).contiguous()
    rot = draws["rot_mats"].contiguous()
    st = _lib.stream_ptr(dev)
    h = _lib.lib()
    a_cum = (P, _lib.ptr(v), len(v), _lib.ptr(f), len(f), _lib.ptr(part("vert_ptr")), _lib.ptr(part("face_ptr")), _lib.ptr(cum), st)
    a_fb = (n_out, P, N, _lib.ptr(v), len(v), _lib.ptr(f), len(f), _lib.ptr(part("vert_ptr")), _lib.ptr(part("face_ptr")), _lib.ptr(cum),
            _lib.ptr(part("parts")), _lib.ptr(draws["u_face"]), _lib.ptr(draws["u_len"]), _lib.ptr(rot), _lib.ptr(perm),
            _lib.ptr(pcds), _lib.ptr(x), _lib.ptr(bv), None, st)
    r_cum = event_timed(lambda: _lib.check(h.da_mesh_cum_area(*a_cum)), reps)
    r_fb = event_timed(lambda: _lib.check(h.da_fragment_batch(*a_fb)), reps)
    src_t = torch.empty_like(pcds)
    return r_cum, r_fb, event_timed(lambda: pcds.copy_(src_t), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=32)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--faces", type=int, nargs="+", default=[320, 1280, 2000])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-objects", type=int, default=2)
    a = ap.parse_args()
    assert a.reps >= 20, "median of at least 20 repetitions"
    assert torch.cuda.is_available(), "fragment_batch_bench needs the GPU"
    dev = torch.device("cuda:0")
    G, parts, N = a.objects, a.parts, a.points
    P = G * parts
    for faces in a.faces:
        meshes = make_meshes(G, parts, faces)
        draws = dict(zip(("u_face", "u_len", "rot_mats", "point_perm"), F._draws([parts] * G, N, -1, False, 0, 0, torch.Generator().manual_seed(0))[:4]))
        d_draws = {k: v.to(dev) for k, v in draws.items()}
        packed = pack(meshes, dev)
        kw = dict(num_points=N, max_num_part=parts, edges=None)
        hp = min(a.host_objects, G)
        h_draws = {k: v[:hp * parts] for k, v in draws.items()}
        got = make_batch3d(packed, return_face_index=True, **kw, **d_draws)
        want = make_batch3d(meshes[:hp], return_face_index=True, **kw, **h_draws)
        n = hp * parts
        assert torch.equal(got.face_index[:n].cpu(), want.face_index), faces
        err = (got.pcds[:n].cpu().double() - want.pcds.double()).abs()
        bound = torch.from_numpy(np.spacing(want.pcds.abs().numpy()).astype(np.float64)) + 2.0 ** -40 * 2.0
        assert bool((err <= bound).all()) and torch.equal(got.x[:n, :4].cpu(), want.x[:, :4]), faces
        del got, want
        out_bytes = P * N * 12
        read_bytes = P * N * (8 + 16 + 4) + P * faces * 8
        cum, fb, copy = launches_alone(packed, d_draws, N, dev, a.reps)
        res = {"objects": G, "parts": parts, "points": N, "faces_per_part": faces, "pcds_bytes": out_bytes, "read_write_bytes": out_bytes + read_bytes,
               "warmup": WARMUP, "reps": a.reps, "host_objects": hp,
               "make_batch3d": host_timed(lambda: make_batch3d(packed, **kw, **d_draws), a.reps),
               "make_batch3d_host": host_timed(lambda: make_batch3d(meshes, device=dev, **kw, **draws), a.reps),
               "da_mesh_cum_area": cum, "da_fragment_batch": fb, "copy": copy,
               "_loop_batch3d": host_timed(lambda: make_batch3d(meshes[:hp], **kw, **h_draws), 3, warmup=1, sync=False)}
        for arm in ("da_fragment_batch", "copy"):
            res[arm]["GB_per_s"] = round(out_bytes / (res[arm]["median_ms"] * 1e-3) / 1e9, 1)
        res["da_fragment_batch"]["read_write_GB_per_s"] = round((out_bytes + read_bytes) / (fb["median_ms"] * 1e-3) / 1e9, 1)
        res["_loop_batch3d"]["batch_ms"] = round(res["_loop_batch3d"]["median_ms"] * G / hp, 1)        # scaled from hp objects to the Batch
        res["kernel_over_copy"] = round(fb["median_ms"] / copy["median_ms"], 3)
        res["host_over_make_batch3d"] = round(res["_loop_batch3d"]["batch_ms"] / res["make_batch3d"]["median_ms"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
