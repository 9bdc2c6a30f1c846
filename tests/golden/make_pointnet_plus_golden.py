"""Writes tests/golden/pointnet_plus_v1.npz from the reference's own PointNetPlus (puzzle_diff/model/backbones/pointnet.py:200-256
and its helpers).  Build container only: it needs the reference tree (REFERENCE_ROOT, default /root/reference); the file it loads
imports only numpy and torch.  No reference program text goes into the repository, only these arrays:

  keys, shapes/<key>, sha/<key>   the state-dict keys of PointNetPlus() in order, their shapes, the SHA-256 of each tensor's bytes
                                  as pointnet_plus_refs.make_weights(weight_seed) generates it (the 1.47 M weights are not stored)
  weight_seed
  case/<P>x<N>/cloud_seed, cloud_sha   the cloud is pointnet_plus_refs.make_cloud(P, N, cloud_seed): 0.3 randn rounded to fp16
  case/<P>x<N>/seed               torch.manual_seed of the run
  case/<P>x<N>/start1, start2     what the reference drew (recorded around its torch.randint calls)
  case/<P>x<N>/{fps1,grp1,fps2,grp2}   the reference's farthest-point and ball-query indices of both levels: int16 arrays for
                                  P <= 3, else .../<name>_sha = SHA-256 of the int32 bytes
  case/<P>x<N>/eval_out           the reference's fp32 eval output [P, 256]
  case/<P>x<N>/dev/eval_out       max |fp32 - fp64| / max |fp64| of the reference against its own .double() (the fp64 run replays the
                                  fp32 run's selections: they are discrete)
  case/1x1/reference_refuses      the reference cannot run fewer points than sa1's 32 samples (its ball query fails to fill the
                                  group); the case holds cloud, seed and starts only, and the rule defines its result

Asserted while writing: the selection rule of pointnet_plus_refs reproduces every stored index; each 1000-point case has both cut
groups (more than 32 members) and centre-only groups at sa1; between 20 % and 80 % of the outputs are non-zero.  A cloud that
breaks one of these is replaced by the next cloud seed."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pointnet_plus_refs as R  # noqa: E402


def load_reference():
    root = os.environ.get("REFERENCE_ROOT", "/root/reference")
    spec = importlib.util.spec_from_file_location("ref_pointnet", os.path.join(root, "puzzle_diff", "model", "backbones", "pointnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Tap:
    """Records (mode "record") or replays (mode "replay") the results of the reference's two selection helpers and the starts its
    torch.randint calls draw."""

    def __init__(self, mod):
        self.mod, self.mode, self.fps, self.ball, self.starts = mod, "record", [], [], []
        self._fps, self._ball, self._randint = mod.farthest_point_sample, mod.query_ball_point, torch.randint
        mod.farthest_point_sample, mod.query_ball_point = self.fps_, self.ball_

    def fps_(self, xyz, npoint):
        if self.mode == "replay":
            return self.fps.pop(0).clone()

        def randint(*a, **k):
            r = self._randint(*a, **k)
            self.starts.append(r.clone())
            return r

        torch.randint = randint
        try:
            out = self._fps(xyz, npoint)
        finally:
            torch.randint = self._randint
        self.fps.append(out.clone())
        return out

    def ball_(self, radius, nsample, xyz, new_xyz):
        if self.mode == "replay":
            return self.ball.pop(0).clone()
        out = self._ball(radius, nsample, xyz, new_xyz)
        self.ball.append(out.clone())
        return out


def run_case(mod, tap, sd, P, N, cloud_seed, seed):
    """-> dict of the case's arrays, or a string saying which assertion the cloud breaks."""
    pts = R.make_cloud(P, N, cloud_seed)
    net = mod.PointNetPlus()
    net.load_state_dict(sd, strict=True)
    net.eval()
    tap.mode, tap.fps, tap.ball, tap.starts = "record", [], [], []
    torch.manual_seed(seed)
    if N < R.K1:
        # the reference cannot run a fragment of fewer points than sa1's 32 samples: its ball query cuts the sorted indices to N
        # columns and then fails to fill them (pointnet.py:350-353).  The case keeps its cloud, seed and drawn starts; the rule
        # (fill with the first member) defines the result, and only the contract and the kernels are held on it.
        try:
            with torch.no_grad():
                net(torch.from_numpy(pts))
        except IndexError:
            pass
        else:
            raise AssertionError("the reference ran a fragment of fewer than 32 points")
        start1 = tap.starts[0].numpy()
        torch.manual_seed(seed)
        start1b, start2 = (torch.randint(0, n, (P,), dtype=torch.long).numpy() for n in (N, R.S1))
        assert np.array_equal(start1, start1b)
        print(f"case {P}x{N}: the reference refuses it (fewer points than samples); starts only")
        return {"cloud_seed": np.int64(cloud_seed), "cloud_sha": np.array(R.digest(pts)), "seed": np.int64(seed),
                "start1": start1.astype(np.int32), "start2": start2.astype(np.int32), "reference_refuses": np.bool_(True)}
    with torch.no_grad():
        out32 = net(torch.from_numpy(pts)).clone()
    start1, start2 = (t.numpy() for t in tap.starts)
    ref = dict(fps1=tap.fps[0].numpy(), grp1=tap.ball[0].numpy(), fps2=tap.fps[1].numpy(), grp2=tap.ball[1].numpy())
    tap.mode = "replay"
    with torch.no_grad():
        out64 = net.double()(torch.from_numpy(pts).double())
    assert not tap.fps and not tap.ball
    sel = R.select(pts, start1, start2)
    for k in ref:
        if not np.array_equal(sel[k], ref[k]):
            return f"the rule and the reference differ in {k} ({int((sel[k] != ref[k]).sum())} entries)"
    if N == 1000:
        members = np.stack([(~(R.d2(pts[p][ref["fps1"][p]][:, None, :], pts[p][None]) > np.float32(R.R1 ** 2))).sum(1) for p in range(P)])
        if not ((members > R.K1).any() and (members == 1).any()):
            return "no cut or no centre-only group at sa1"
    nz = float((out32 != 0).float().mean())
    if not 0.2 <= nz <= 0.8:
        return f"{nz:.1%} of the outputs are non-zero"
    c = {"cloud_seed": np.int64(cloud_seed), "cloud_sha": np.array(R.digest(pts)), "seed": np.int64(seed),
         "start1": start1.astype(np.int32), "start2": start2.astype(np.int32), "eval_out": out32.numpy(),
         "dev/eval_out": np.float64(float((out32.double() - out64).abs().max() / out64.abs().max()))}
    for k, v in ref.items():
        if P <= 3:
            c[k] = v.astype(np.int16)
        else:
            c[k + "_sha"] = np.array(R.digest(v.astype(np.int32)))
    print(f"case {P}x{N}: cloud seed {cloud_seed}, non-zero outputs {nz:.1%}, fp32 vs fp64 {float(c['dev/eval_out']):.3e}")
    return c


def main():
    mod = load_reference()
    tap = Tap(mod)
    w = R.make_weights()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    keys = list(mod.PointNetPlus().state_dict())
    assert keys == list(w), "the generator's keys are not the reference's"
    out = {"keys": np.array(keys), "weight_seed": np.int64(R.WEIGHT_SEED)}
    for k, v in w.items():
        out[f"shapes/{k}"] = np.array(v.shape, dtype=np.int64)
        out[f"sha/{k}"] = np.array(R.digest(v))
    for ci, (P, N) in enumerate(R.CASES):
        for attempt in range(20):
            c = run_case(mod, tap, sd, P, N, cloud_seed=1000 * (ci + 1) + attempt, seed=300 + ci)
            if not isinstance(c, str):
                break
            print(f"case {P}x{N}: cloud seed {1000 * (ci + 1) + attempt} dropped: {c}")
        else:
            raise SystemExit(f"case {P}x{N}: no cloud seed passes")
        for k, v in c.items():
            out[f"case/{P}x{N}/{k}"] = v
    path = os.path.join(HERE, "pointnet_plus_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    sys.exit(main())
