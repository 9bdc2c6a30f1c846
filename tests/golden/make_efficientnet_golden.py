"""Writes tests/golden/efficientnet_v1.npz: the keys, shapes, seed and SHA-256 digests of what the generators of
efficientnet_refs.py must produce (the 3.6 M weights themselves are not stored).  Run from the repository root:
``python tests/golden/make_efficientnet_golden.py``."""
import os

import numpy as np

import efficientnet_refs as R

if __name__ == "__main__":
    sd = R.make_weights()
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez(os.path.join(here, "efficientnet_v1.npz"), keys=np.array(list(sd)), shapes=np.array(["x".join(map(str, v.shape)) for v in sd.values()]),
             weight_seed=np.int64(R.WEIGHT_SEED), weights_sha256=np.array(R.digest(sd.values())), crops_sha256=np.array(R.digest([R.make_crops(6, 1)])))
