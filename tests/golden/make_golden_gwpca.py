#!/usr/bin/env python3
"""Golden fixture for group-wise PCA from the REFERENCE implementation (Utils/GroupWisePCA.py `applyGWPCA`), run with the
scikit-learn installed in the build container (1.7.2: its `auto` solver is exact, `covariance_eigh` when n >= 10 w and LAPACK
`full` otherwise; the 1.3 the reference pins would send a large scene through the randomized solver).

Runs only in the build container (needs /root/reference).  Only arrays are recorded:
  <tag>_raw   the raw scene [H, W, bands]            <tag>_out   applyGWPCA(raw, nc, group, whiten), fp64 [H, W, nc]
  <tag>_args  (nc, group, whiten)                    <tag>_dist  per component, max |reference - tests/gwpca_ref.py|: the
                                                                 reference's own rounding against an independent fp64 computation
  table_bands, table_widths   the reference's `split_data` widths (group 4) for 64 / 103 / 144 / 204 / 224 / 270 bands
Scenes (graded spectra, tests/gwpca_ref.py `graded`):
  A 13 x 13 x  64  n >= 10 w (covariance_eigh)       B 10 x 9 x 103  uneven split 25/26/26/26, n < 10 w (full)
  C  8 x  8 x 204  n < 10 w                          D  8 x 9 x 270  widths 67/68/67/68
  E 13 x 13 x  64  fp32, recorded from its fp64 widening
  F 10 x 10 x  64  group 2, nc 16                    G 10 x 10 x 40  group 1, nc 8
  H = B's scene with whiten=False
Condition, asserted here so that no component ever has to be left out of a comparison: every retained eigenvalue is at least
0.2 lambda_k away from every other eigenvalue of its group, and lambda_k >= 1e-4 lambda_1.

    python tests/golden/make_golden_gwpca.py        ->  tests/golden/gwpca.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from Utils.GroupWisePCA import applyGWPCA, split_data  # noqa: E402
import gwpca_ref as R  # noqa: E402

SCENES = {   # tag: (H, W, bands, seed, ratio, dtype, nc, group, whiten)
    "A": (13, 13, 64, 1, 0.55, np.float64, 32, 4, True),
    "B": (10, 9, 103, 2, 0.45, np.float64, 32, 4, True),
    "C": (8, 8, 204, 3, 0.4, np.float64, 32, 4, True),
    "D": (8, 9, 270, 4, 0.4, np.float64, 32, 4, True),
    "E": (13, 13, 64, 5, 0.55, np.float32, 32, 4, True),
    "F": (10, 10, 64, 6, 0.45, np.float64, 16, 2, True),
    "G": (10, 10, 40, 7, 0.45, np.float64, 8, 1, True),
}


def main():
    rec = {}
    for tag, (H, W, Cb, seed, ratio, dtype, nc, group, whiten) in SCENES.items():
        rec[tag + "_raw"] = R.graded(H, W, Cb, seed, group=group, ratio=ratio, dtype=dtype)
        rec[tag + "_args"] = np.array([nc, group, int(whiten)])
    rec["H_raw"], rec["H_args"] = rec["B_raw"], np.array([32, 4, 0])
    for tag in list(SCENES) + ["H"]:
        raw = rec[tag + "_raw"]
        nc, group, whiten = (int(v) for v in rec[tag + "_args"])
        wide = raw.astype(np.float64)                    # an fp32 scene is recorded from its exact widening
        out = applyGWPCA(wide, nc=nc, group=group, whiten=bool(whiten))
        ref = R.gwpca_ref(wide, nc=nc, group=group, whiten=bool(whiten))
        assert out.dtype == np.float64 and out.shape == raw.shape[:2] + (nc,)
        assert ref["gap_rel"].min() >= 0.2 and ref["lam_rel"].min() >= 1e-4, (tag, ref["gap_rel"].min(), ref["lam_rel"].min())
        rec[tag + "_out"] = out
        rec[tag + "_dist"] = R.component_err(out, ref["out"])
        print(f"{tag}: {raw.shape} {raw.dtype} nc={nc} group={group} whiten={whiten}  min gap/lambda {ref['gap_rel'].min():.2f}  "
              f"min lambda/lambda_1 {ref['lam_rel'].min():.1e}  max dist {rec[tag + '_dist'].max():.2e}  "
              f"worst dist/bound {(rec[tag + '_dist'] / ref['bound']).max():.2f}")
    del rec["H_raw"]                                     # the same array as B_raw
    bands = np.array([64, 103, 144, 204, 224, 270])
    rec["table_bands"] = bands
    rec["table_widths"] = np.array([[x.shape[1] for x in split_data([np.zeros((1, b))], 4)] for b in bands])
    path = os.path.join(HERE, "gwpca.npz")
    np.savez(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
