#!/usr/bin/env python3
"""Dump what every route of the denoiser's training step computes, and compare two dumps: the check that a change to the training path's
host code (csrc/da_train*.hip) left every result as it was.

The routes, the seeded weights and inputs and the two accumulated forward and backward passes per route are those of
tests/test_gpu_train_routes.py (`ROUTES`, `run_route`); every route runs with the backward as ALL and as EARLY + LATE.  A dump holds,
per route and schedule, the forward outputs, d_feats, the flat gradient and da_train_workspace_bytes_ex.  The library is the one
DA_LIB_PATH names (default: the tree's); DA_TRAIN_SIDE_STREAMS is read once per process, so dump once per setting:

    DA_LIB_PATH=.../lib_parent/libdiffassemble_hip.so python tools/train_route_dump.py dump parent_side.npz
    python tools/train_route_dump.py dump new_side.npz
    DA_TRAIN_SIDE_STREAMS=0 python tools/train_route_dump.py dump new_one.npz
    python tools/train_route_dump.py compare parent_side.npz new_side.npz        # exit status 1 if any array differs

`compare` asks torch.equal of every array; the one exception is the time_emb rows of the gradient, which k_time_scatter adds with
atomics in any library: <= 1e-6 * max|g| + 1e-12 (the rule of the test).  `dump --expected` also prints the workspace sizes as the
literal table the test pins."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def dump(out, routes, expected):
    import numpy as np
    import torch
    import test_gpu_train_routes as TR
    from diffassemble_amd import _lib
    dev = torch.device("cuda:0")
    arrays, sizes = {}, {}
    for name in routes or list(TR.ROUTES):
        for tag, staged in (("all", False), ("early_late", True)):
            res = TR.run_route(name, dev, staged)
            sizes[name] = int(res["ws_bytes"])
            for k, v in res.items():
                arrays[f"{name}/{tag}/{k}"] = v.numpy()
    np.savez(out, **arrays)
    print(f"{out}: {len(arrays)} arrays of {len(sizes)} routes; library {_lib.LIB_PATH}; "
          f"DA_TRAIN_SIDE_STREAMS={os.environ.get('DA_TRAIN_SIDE_STREAMS', '(default)')}")
    if expected:
        print("EXPECTED = {")
        for name, b in sizes.items():
            print(f'    "{name}": {b},')
        print("}")


def compare(path_a, path_b):
    import numpy as np
    import torch
    import test_gpu_train_routes as TR
    a, b = np.load(path_a), np.load(path_b)
    runs = sorted({k.rsplit("/", 1)[0] for k in list(a.files) + list(b.files)})
    compared, bad = 0, []
    for run in runs:
        ra = {k.rsplit("/", 1)[1]: torch.from_numpy(a[k]) for k in a.files if k.rsplit("/", 1)[0] == run}
        rb = {k.rsplit("/", 1)[1]: torch.from_numpy(b[k]) for k in b.files if k.rsplit("/", 1)[0] == run}
        compared += len(set(ra) | set(rb))
        bad += [f"{run}/{k}" for k in TR.differing(ra, rb)]
    print(f"{path_a} vs {path_b}: {compared} arrays compared, {len(bad)} differ")
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--routes", default="", help="comma-separated route names (default: all)")
    d.add_argument("--expected", action="store_true", help="print the workspace sizes as the test's EXPECTED table")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(args.out, [r for r in args.routes.split(",") if r], args.expected)
        return 0
    return compare(args.a, args.b)


if __name__ == "__main__":
    sys.exit(main())
