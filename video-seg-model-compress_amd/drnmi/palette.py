"""The reference's colour tables (seg_video_old_no_plot.py:29-55, semantic_seg.py:52-78), as plain
data, and their device form for the renderer (drnmi.ops.render_labels, csrc/render.hip).

  CITYSCAPE_PALETTE  uint8 [20, 3] RGB: the 19 Cityscapes train classes, then black (entry 19 is
                     what labels >= 20, the ignore value 255 among them, are drawn with)
  TRIPLET_PALETTE    uint8 [3, 4] RGBA, used when num_classes == 3
  generic_palette(n) uint8 [n, 3] RGB for more than 20 classes (ADE20K's 150): not a reference table

Deviation: the renderer is RGB only.  as_device_palette drops a 4th column, so TRIPLET_PALETTE
images come out as RGB where the reference's Image.fromarray(palettes[pred]) makes RGBA; its alpha
is 255 everywhere, so the picture is the same.
"""
from __future__ import annotations

import numpy as np
import torch

CITYSCAPE_PALETTE = np.asarray([
    [128, 64, 128],
    [244, 35, 232],
    [70, 70, 70],
    [102, 102, 156],
    [190, 153, 153],
    [153, 153, 153],
    [250, 170, 30],
    [220, 220, 0],
    [107, 142, 35],
    [152, 251, 152],
    [70, 130, 180],
    [220, 20, 60],
    [255, 0, 0],
    [0, 0, 142],
    [0, 0, 70],
    [0, 60, 100],
    [0, 80, 100],
    [0, 0, 230],
    [119, 11, 32],
    [0, 0, 0]], dtype=np.uint8)

TRIPLET_PALETTE = np.asarray([
    [0, 0, 0, 255],
    [217, 83, 79, 255],
    [91, 192, 222, 255]], dtype=np.uint8)


def generic_palette(num_classes: int) -> np.ndarray:
    """uint8 [num_classes, 3] RGB for any 1 <= num_classes <= 256: the usual bit-interleaved colour
    map.  Eight rounds; round r takes bits 0, 1, 2 of what is left of the class id to bit 7 - r of
    R, G, B and drops them.  Class 0 is black, class 1 (128, 0, 0), class 2 (0, 128, 0), ...; the id
    can be read back from the colour, so all 256 entries are distinct."""
    if not 1 <= num_classes <= 256:
        raise ValueError(f"num_classes must be in 1..256, got {num_classes}")
    ids = np.arange(num_classes, dtype=np.int64)
    pal = np.zeros((num_classes, 3), dtype=np.int64)
    for r in range(8):
        for ch in range(3):
            pal[:, ch] |= ((ids >> ch) & 1) << (7 - r)
        ids = ids >> 3
    return pal.astype(np.uint8)


def palette_for(num_classes: int) -> np.ndarray:
    """The table the reference's eval drivers colour with (semantic_seg.py:450-452) for the class
    counts it covers: TRIPLET_PALETTE for 3, else CITYSCAPE_PALETTE (19 colours, then black).  Above
    20 classes that table would paint every class from 19 up black, so they get generic_palette."""
    if num_classes > 20:
        return generic_palette(num_classes)
    return TRIPLET_PALETTE if num_classes == 3 else CITYSCAPE_PALETTE


def as_device_palette(palette, device) -> torch.Tensor:
    """[P, 3] or [P, 4] (numpy array, nested list or tensor; values 0..255, 1 <= P <= 256) ->
    contiguous uint8 [P, 3] on `device`.  A 4th (alpha) column is dropped: the renderer is RGB only."""
    key = None
    if isinstance(palette, torch.Tensor):
        t = palette.detach()
    else:
        a = np.asarray(palette)
        if a.dtype.kind not in "iu":
            raise ValueError("palette must hold integers 0..255")
        # host tables are uploaded once per device: a later call copies nothing, so a segment(render=...)
        # with a numpy palette can be captured in a graph after one warm-up call
        key = (a.shape, a.astype(np.int64).tobytes(), str(torch.device(device)))
        if key in _DEVICE_PALETTES:
            return _DEVICE_PALETTES[key]
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64)))
    t = _checked_u8(t)[:, :3].contiguous().to(device)
    if key is not None:
        _DEVICE_PALETTES[key] = t
    return t


_DEVICE_PALETTES: dict = {}


def _checked_u8(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2 or t.shape[1] not in (3, 4) or not 1 <= t.shape[0] <= 256:
        raise ValueError(f"palette must be [P, 3] or [P, 4] with 1 <= P <= 256, got {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("palette must hold integers 0..255")
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError("palette values must be in 0..255")
        t = t.to(torch.uint8)
    return t


__all__ = ["CITYSCAPE_PALETTE", "TRIPLET_PALETTE", "palette_for", "generic_palette", "as_device_palette"]
