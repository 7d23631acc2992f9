#!/usr/bin/env python3
"""Golden fixture for the colour maps (hsimae_amd.label_to_colormap) from the REFERENCE implementation.

Needs a checkout of the reference: its `Utils.Label_to_Colormap.label_to_colormap` is called once, on the label map
np.arange(20).reshape(1, 20) (every label it supports), and only the returned uint8 [1, 20, 3] array is recorded.

    python tests/golden/make_golden_colormap.py <reference checkout>        ->  tests/golden/colormap.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from Utils.Label_to_Colormap import label_to_colormap

    label = np.arange(20).reshape(1, 20)
    colors = label_to_colormap(label)
    assert colors.shape == (1, 20, 3) and colors.dtype == np.uint8
    path = os.path.join(HERE, "colormap.npz")
    np.savez_compressed(path, label=label, colors=colors)
    print(colors[0].tolist(), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
