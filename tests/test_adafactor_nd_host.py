"""The tables of da_adafactor_nd_step (FusedAdafactorND, diffassemble_amd/train.py) as a pure function of a list of shapes:
no GPU, no library call.  The kernels trust these tables for every address they form, so coverage and disjointness are
checked here, on the host, for every code path's shapes (tests/test_gpu_adafactor_nd.py runs the same list on the GPU)."""
import numpy as np
import pytest
import torch

from diffassemble_amd import _lib
from diffassemble_amd import train as T

SHAPES = [(8, 4, 4, 3, 3), (8, 3, 1, 3, 3), (8, 4, 4, 1, 1), (5, 1, 7), (3, 1), (1, 9), (70, 4100), (3, 16384), (32,), (4097,), (1,),
          (), (2, 3, 20, 30), (33, 1025), (64, 2), (544, 8192)]


@pytest.fixture(scope="module")
def plan():
    return T.AdafactorNDPlan(SHAPES)


def _prod(s):
    return int(np.prod(s, dtype=np.int64)) if len(s) else 1


def test_every_element_is_covered_exactly_once(plan):
    for pid, (shape, t) in enumerate(zip(SHAPES, plan.tensors)):
        blocks = plan.blocks[t["blk0"]:t["blk0"] + t["nblk"]]
        assert t["nblk"] > 0 and (blocks[:, 0] == pid).all(), shape
        assert t["B"] * t["R"] * t["C"] == _prod(shape) == t["numel"]
        cover = np.zeros(t["numel"], dtype=np.int32)
        for _, b, r0, nr, c0, nc in blocks:
            if t["kind"] == T.ND_KIND_VECTOR:
                assert 0 < nr <= T.ND_VEC_BLOCK and r0 >= 0 and r0 + nr <= t["numel"]
                cover[r0:r0 + nr] += 1
            elif t["kind"] == T.ND_KIND_TINY:
                assert 0 < nr <= T.ND_SLICES_PER_BLOCK and r0 >= 0 and r0 + nr <= t["B"]
                assert t["R"] * t["C"] <= T.ND_TINY_SLICE
                cover.reshape(t["B"], -1)[r0:r0 + nr] += 1
            else:
                assert 0 <= b < t["B"] and r0 % T.ND_TILE_ROWS == 0 and c0 % T.ND_TILE_COLS == 0
                assert 0 < nr <= T.ND_TILE_ROWS and 0 < nc <= T.ND_TILE_COLS and r0 + nr <= t["R"] and c0 + nc <= t["C"]
                cover.reshape(t["B"], t["R"], t["C"])[b, r0:r0 + nr, c0:c0 + nc] += 1
        assert (cover == 1).all(), shape
    # the block ranges of the tensors tile the block table
    assert [t["blk0"] for t in plan.tensors] == list(np.cumsum([0] + [t["nblk"] for t in plan.tensors[:-1]]))
    assert plan.tensors[-1]["blk0"] + plan.tensors[-1]["nblk"] == len(plan.blocks)


def test_kinds_follow_the_shapes(plan):
    kinds = {s: t["kind"] for s, t in zip(SHAPES, plan.tensors)}
    for s in [(32,), (4097,), (1,), ()]:
        assert kinds[s] == T.ND_KIND_VECTOR
    for s in [(8, 4, 4, 3, 3), (8, 3, 1, 3, 3), (8, 4, 4, 1, 1), (5, 1, 7), (3, 1), (1, 9)]:
        assert kinds[s] == T.ND_KIND_TINY
    for s in [(70, 4100), (3, 16384), (2, 3, 20, 30), (33, 1025), (64, 2), (544, 8192)]:
        assert kinds[s] == T.ND_KIND_TILED


def test_state_sizes_are_transformers_and_offsets_do_not_overlap(plan):
    used = np.zeros(plan.state_floats, dtype=np.int32)
    for shape, t in zip(SHAPES, plan.tensors):
        if len(shape) >= 2:
            assert t["row_size"] == _prod(shape[:-1])                       # exp_avg_sq_row
            assert t["col_size"] == _prod(shape[:-2]) * shape[-1]           # exp_avg_sq_col
        else:
            assert t["row_size"] == _prod(shape) and t["col_size"] == 0     # exp_avg_sq
        used[t["row_off"]:t["row_off"] + t["row_size"]] += 1
        used[t["col_off"]:t["col_off"] + t["col_size"]] += 1
    assert (used == 1).all()


def test_jobs_and_scratch(plan):
    """Every tensor has exactly one learning-rate job (b = 0, c0 < 0); a tiled tensor one row job per slice and column jobs that
    cover its columns once; the partial-sum areas of the tiled tensors are disjoint and inside the scratch buffer."""
    cp = np.zeros(plan.colpart_floats, dtype=np.int32)
    rp = np.zeros(plan.rowpart_floats, dtype=np.int32)
    rmean = np.zeros(plan.n_slices, dtype=np.int32)
    for pid, t in enumerate(plan.tensors):
        jobs = plan.jobs[plan.jobs[:, 0] == pid]
        rows = jobs[jobs[:, 2] < 0]
        cols = jobs[jobs[:, 2] >= 0]
        if t["kind"] != T.ND_KIND_TILED:
            assert len(cols) == 0 and rows[:, 1].tolist() == [0]
            continue
        assert sorted(rows[:, 1].tolist()) == list(range(t["B"]))
        for b in range(t["B"]):
            c = np.zeros(t["C"], dtype=np.int32)
            for c0 in cols[cols[:, 1] == b][:, 2]:
                assert c0 % T.ND_COL_JOB == 0 and c0 < t["C"]
                c[c0:c0 + T.ND_COL_JOB] += 1
            assert (c == 1).all()
        nrb, ncb = -(-t["R"] // T.ND_TILE_ROWS), -(-t["C"] // T.ND_TILE_COLS)
        cp[t["colpart_off"]:t["colpart_off"] + t["B"] * nrb * t["C"]] += 1
        rp[t["rowpart_off"]:t["rowpart_off"] + t["B"] * ncb * t["R"]] += 1
        rmean[t["rmean_off"]:t["rmean_off"] + t["B"]] += 1
    assert (cp == 1).all() and (rp == 1).all() and (rmean == 1).all()
    assert plan.scratch_floats == 2 * len(plan.blocks) + 4 * len(plan.tensors) + plan.n_slices + plan.colpart_floats + plan.rowpart_floats
    assert plan.scal_off == 2 * len(plan.blocks)


def test_param_table_layout(plan):
    tab = plan.param_table()
    assert tab.dtype.itemsize == 80 and len(tab) == len(SHAPES)           # sizeof(NdParam), da_optim_nd.hip
    assert (tab["p"] == 0).all() and (tab["g"] == 0).all() and (tab["active"] == 0).all()
    for rec, t in zip(tab, plan.tensors):
        for k in ("row_off", "col_off", "colpart_off", "rowpart_off", "B", "R", "C", "kind", "blk0", "nblk", "rmean_off"):
            assert int(rec[k]) == t[k], k


def test_constants_match_the_kernels():
    """The tile sizes the table builder uses are the ones da_optim_nd.hip is compiled with (the struct sizes are tied by a
    static_assert there; these are not)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "diffassemble_amd", "csrc", "da_optim_nd.hip")).read()
    got = {k: int(v) for k, v in re.findall(r"\b(ND_[A-Z]+) = (\d+)\b", src)}
    assert got == {"ND_TR": T.ND_TILE_ROWS, "ND_TC": T.ND_TILE_COLS, "ND_VEC": T.ND_VEC_BLOCK, "ND_BCH": T.ND_COL_JOB,
                   "ND_TINY": T.ND_TINY_SLICE, "ND_SPB": T.ND_SLICES_PER_BLOCK}
    assert "__launch_bounds__(256)" in src and T.ND_SLICES_PER_BLOCK == 256


def test_empty_and_oversized_tensors_are_refused():
    with pytest.raises(_lib.DaError, match="parameter 1"):
        T.AdafactorNDPlan([(3, 3), (0, 4)])
    with pytest.raises(_lib.DaError, match="parameter 0"):
        T.AdafactorNDPlan([(1 << 16, 1 << 15)])


def test_unsupported_parameters_raise_and_say_which():
    ok = torch.nn.Parameter(torch.zeros(4, 6))
    with pytest.raises(_lib.DaError, match=r"parameter 1 \(shape \(4, 6\)\) is torch.float16"):
        T.FusedAdafactorND([ok, torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.float16))])
    with pytest.raises(_lib.DaError, match=r"parameter 0 \(shape \(6, 4\)\) is not contiguous"):
        T.FusedAdafactorND([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(_lib.DaError, match=r"parameter 0 \(shape \(4, 6\)\) is on cpu"):
        T.FusedAdafactorND([ok])
