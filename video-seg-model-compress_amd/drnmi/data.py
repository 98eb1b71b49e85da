"""Fine-tune data path: the reference's per-sample transform pipeline as one GPU gather.

The reference builds every training sample on the CPU with PIL and numpy (semantic_seg.py:885-889):

    Compose([RandomCrop(crop_size), RandomHorizontalFlip(), ToTensor(), Normalize(mean, std)])

and the validation samples with the same list without the flip (:918-921).  Here the random draws
and the geometry stay on the host -- a few integers per sample -- and the pixels never do: a uint8
batch goes to the device once and `drnmi_train_ingest_u8` (csrc/ingest.hip) writes the fp32 NCHW
input and the int64 target the model and the criterion take.

Host logic (no GPU; our restatement of data_transforms.py:9-45, :96-106, :128-155):

  extend_1d(n, lo, hi)      source index of every position of pad_reflection along one axis
  draw_params(w, h, crop)   the reference's random draws in the reference's order
  index_maps(h, w, crop, x1, y1, flip)
                            the two int32 tables of one sample (include/drnmi.h, encoding below)

The reference's reflection padding is not numpy's 'reflect': the leading side mirrors without the
edge element (rows top..1), the trailing side mirrors with it (rows n-1..n-bottom).  A pad larger
than n - 1 is capped and the remainder applied, by the same rule, to the already extended axis.
The 2-D padding is separable into this map per axis.  The label is padded with the constant 255.

Table encoding: an entry e >= 0 is a source row / column inside the image; an entry e < 0 marks a
padded position whose image source index is ~e and whose label is 255.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from .drnseg import INFO_MEAN, INFO_STD


def extend_1d(n: int, lo: int, hi: int) -> list[int]:
    """Source index (0..n-1) of every position of an axis of length n after the reference's
    pad_reflection with `lo` leading and `hi` trailing elements (data_transforms.py:128-155)."""
    if n < 1 or lo < 0 or hi < 0:
        raise ValueError(f"extend_1d: need n >= 1 and pads >= 0, got n={n}, lo={lo}, hi={hi}")
    if n == 1 and (lo or hi):
        raise ValueError("extend_1d: an axis of length 1 cannot be reflection-padded "
                         "(the reference's pad_reflection recurses forever)")
    idx = list(range(n))
    while lo or hi:
        m = len(idx)
        next_lo, next_hi = max(lo - (m - 1), 0), max(hi - (m - 1), 0)
        lo, hi = lo - next_lo, hi - next_hi
        idx = idx[lo:0:-1] + idx + idx[-1:-hi - 1:-1]
        lo, hi = next_lo, next_hi
    return idx


def _pads(size: int, target: int) -> tuple[int, int]:
    """(leading, trailing) pad of RandomCrop along one axis (data_transforms.py:24-29)."""
    if size < target:
        lead = (target - size) // 2
        return lead, target - size - lead
    return 0, 0


def draw_params(w: int, h: int, crop, flip: bool = True, rng=random) -> tuple[int, int, bool]:
    """(x1, y1, flipped) of one sample, drawn as Compose([RandomCrop(crop), RandomHorizontalFlip()])
    draws them: nothing for the crop when the padded size equals it, otherwise
    x1 = randint(0, W' - tw) then y1 = randint(0, H' - th) (both always drawn, in that order), then
    random() < 0.5 for the flip (not drawn when flip=False, the validation pipeline).
    crop = (tw, th), as the reference's class unpacks `tw, th = self.size`; an int means a square."""
    tw, th = (int(crop), int(crop)) if isinstance(crop, (int, float)) else (int(crop[0]), int(crop[1]))
    left, right = _pads(w, tw)
    top, bottom = _pads(h, th)
    pw, ph = w + left + right, h + top + bottom
    x1 = y1 = 0
    if not (pw == tw and ph == th):
        x1 = rng.randint(0, pw - tw)
        y1 = rng.randint(0, ph - th)
    flipped = bool(rng.random() < 0.5) if flip else False
    return x1, y1, flipped


def _axis_map(size: int, target: int, start: int) -> np.ndarray:
    lead, trail = _pads(size, target)
    src = np.asarray(extend_1d(size, lead, trail), dtype=np.int32)
    pos = np.arange(src.size)
    enc = np.where((pos < lead) | (pos >= lead + size), ~src, src)
    if not 0 <= start <= src.size - target:
        raise ValueError(f"crop offset {start} outside 0..{src.size - target}")
    return enc[start:start + target]


def index_maps(h: int, w: int, crop, x1: int, y1: int, flip: bool) -> tuple[np.ndarray, np.ndarray]:
    """int32 (rowmap[th], colmap[tw]) of one h x w sample cropped to crop = (tw, th) at (x1, y1) of
    the padded image, flipped left-right when `flip`: colmap[x] is the extended axis at
    x1 + (tw - 1 - x if flip else x).  Padded positions are stored as ~src."""
    tw, th = (int(crop), int(crop)) if isinstance(crop, (int, float)) else (int(crop[0]), int(crop[1]))
    rowmap = _axis_map(h, th, y1)
    colmap = _axis_map(w, tw, x1)
    if flip:
        colmap = colmap[::-1]
    return np.ascontiguousarray(rowmap, dtype=np.int32), np.ascontiguousarray(colmap, dtype=np.int32)


class TrainIngest:
    """The reference's training transform list on the GPU, for a loader of uint8 batches.

        ingest = TrainIngest(crop_size)                      # validation: flip=False
        for images_u8, labels_u8 in loader:                  # [n,h,w,3] / [n,h,w] uint8
            input, target = ingest(images_u8.cuda(non_blocking=True), labels_u8.cuda(non_blocking=True))

    __call__(images_u8, labels_u8=None, params=None) -> (input fp32 [n,3,th,tw], target int64
    [n,th,tw] or None).  images_u8 is a uint8 [n,h,w,3] device tensor, or a list of [h_i,w_i,3]
    tensors (datasets whose images differ in size, as ADE20K: one launch per sample into slices of
    the batch outputs).  params, a list of n (x1, y1, flip), overrides the draws.  crop_size is
    (tw, th) or an int, as RandomCrop takes it.

    The draws come from `rng` (default: the `random` module, the reference's source) in the
    reference's order, one sample after the other in batch order: they equal the reference's with
    num_workers=0 (with worker processes the reference draws from each worker's own copy of the
    generator, which no single stream reproduces).  CPU tensors raise: there is no CPU fallback.
    """

    def __init__(self, crop_size, mean=INFO_MEAN, std=INFO_STD, flip: bool = True, rng=None):
        if isinstance(crop_size, (int, float)):
            crop_size = (int(crop_size), int(crop_size))
        self.crop = (int(crop_size[0]), int(crop_size[1]))            # (tw, th)
        if self.crop[0] <= 0 or self.crop[1] <= 0:
            raise ValueError(f"crop_size must be positive, got {crop_size}")
        self.mean = [float(v) for v in mean]
        self.std = [float(v) for v in std]
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("mean and std must have 3 entries")
        self.flip = flip
        self.rng = rng if rng is not None else random

    def tables(self, sizes, params=None):
        """One int32 host array holding every sample's rowmap then every sample's colmap, and the
        (x1, y1, flip) used.  sizes: (h, w) per sample."""
        tw, th = self.crop
        n = len(sizes)
        if params is None:
            params = [draw_params(w, h, self.crop, self.flip, self.rng) for h, w in sizes]
        elif len(params) != n:
            raise ValueError(f"params has {len(params)} entries for {n} samples")
        tab = np.empty(n * (th + tw), dtype=np.int32)
        for i, ((h, w), (x1, y1, fl)) in enumerate(zip(sizes, params)):
            r, c = index_maps(h, w, self.crop, x1, y1, fl)
            tab[i * th:(i + 1) * th] = r
            tab[n * th + i * tw:n * th + (i + 1) * tw] = c
        return tab, params

    def __call__(self, images_u8, labels_u8=None, params=None):
        from . import torch_ops  # noqa: F401  (registers torch.ops.drnmi.train_ingest)
        as_list = isinstance(images_u8, (list, tuple))
        imgs = list(images_u8) if as_list else images_u8
        labs = labels_u8
        if as_list and labs is not None:
            labs = list(labs)
            if len(labs) != len(imgs):
                raise ValueError("images and labels differ in length")
        first = imgs[0] if as_list else imgs
        if not first.is_cuda:
            raise RuntimeError("drnmi TrainIngest runs on the HIP kernel (no CPU fallback): "
                               "move the uint8 batch to the device")
        dev = first.device
        tw, th = self.crop
        if as_list:
            sizes = [(int(t.shape[0]), int(t.shape[1])) for t in imgs]
        else:
            if imgs.dim() != 4:
                raise ValueError("images_u8 must be uint8 [n, h, w, 3] or a list of [h, w, 3]")
            sizes = [(int(imgs.shape[1]), int(imgs.shape[2]))] * int(imgs.shape[0])
        n = len(sizes)
        tab, _ = self.tables(sizes, params)
        host = torch.from_numpy(tab)
        if torch.cuda.is_available():
            host = host.pin_memory()
        dtab = host.to(dev, non_blocking=True)                         # both tables, one copy
        rowmap, colmap = dtab[:n * th].view(n, th), dtab[n * th:].view(n, tw)
        op = torch.ops.drnmi.train_ingest
        if not as_list:
            inp, tgt = op(imgs, labs, rowmap, colmap, self.mean, self.std)
            return inp, (tgt if labs is not None else None)
        inp = torch.empty(n, 3, th, tw, dtype=torch.float32, device=dev)
        tgt = torch.empty(n, th, tw, dtype=torch.int64, device=dev) if labs is not None else None
        for i in range(n):
            torch_ops.train_ingest_into(imgs[i].unsqueeze(0), labs[i].unsqueeze(0) if labs is not None else None,
                                        rowmap[i:i + 1], colmap[i:i + 1], self.mean, self.std, inp[i:i + 1],
                                        tgt[i:i + 1] if tgt is not None else None)
        return inp, tgt


__all__ = ["extend_1d", "draw_params", "index_maps", "TrainIngest"]
