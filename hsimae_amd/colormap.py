"""The pictures of a classification map (Utils/Label_to_Colormap.py, Model_Finetuning.py:282-300): one colour per label and
the map written as an 8-bit RGB PNG.  A palette lookup on the host copy of the map: no arithmetic, no kernel, and no
dependency beyond zlib (the reference goes through matplotlib.image.imsave).
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import torch


def _default_palette() -> np.ndarray:
    """The reference's 20 colours: the PASCAL VOC colour map (label bits 0, 1, 2 feed r, g, b from the top bit down, three
    label bits per colour bit) with entry 7 replaced by (0, 64, 128).  tests/golden/colormap.npz holds the reference's own
    output for the labels 0 .. 19."""
    pal = np.zeros((20, 3), np.uint8)
    for label in range(20):
        c = label
        for bit in range(7, -1, -1):
            for ch in range(3):
                pal[label, ch] |= ((c >> ch) & 1) << bit
            c >>= 3
    pal[7] = (0, 64, 128)
    return pal


PALETTE = _default_palette()
PALETTE.setflags(write=False)


def label_to_colormap(label, palette=None) -> np.ndarray:
    """uint8 [H, W, 3] colours of an integer label map [H, W] (numpy array or tensor, CPU or device).  `palette`: uint8
    [n, 3], default the reference's 20 colours.  A label outside [0, n) raises ValueError (the reference asserts)."""
    pal = PALETTE if palette is None else np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.dtype != np.uint8 or pal.shape[0] < 1:
        raise ValueError("palette must be a uint8 array [n, 3]")
    lab = label.detach().cpu().numpy() if isinstance(label, torch.Tensor) else np.asarray(label)
    if lab.ndim != 2 or lab.dtype.kind not in "iu":
        raise ValueError(f"label must be an integer map [H, W], got shape {lab.shape}, dtype {lab.dtype}")
    if lab.size and (lab.min() < 0 or lab.max() >= pal.shape[0]):
        raise ValueError(f"label {int(lab.max() if lab.max() >= pal.shape[0] else lab.min())} outside the palette's "
                         f"{pal.shape[0]} classes")
    return pal[lab]


def encode_png(rgb: np.ndarray) -> bytes:
    """uint8 [H, W, 3] -> the bytes of an 8-bit RGB PNG (colour type 2, no interlace, every scanline with filter 0)."""
    rgb = np.ascontiguousarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("encode_png takes a non-empty uint8 array [H, W, 3]")
    h, w = rgb.shape[:2]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    lines = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, 3 * w)], axis=1)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(lines.tobytes(), 9)) + chunk(b"IEND", b""))


def save_label_png(path, label, palette=None) -> None:
    """Write label_to_colormap(label, palette) to `path` as a PNG."""
    data = encode_png(label_to_colormap(label, palette))
    with open(os.fspath(path), "wb") as fh:
        fh.write(data)
