"""Generate tests/golden/ingest.npz by running the REFERENCE's data_transforms.

Run where the reference checkout is available (it never travels with the repository):

    python tests/golden/make_ingest_golden.py --reference <path to the reference checkout>

For every case (a seeded uint8 image and label, a crop size, a seed) it records what the reference's
training transform list makes of it (semantic_seg.py:885-889):

    random.seed(seed)
    image, label = Compose([RandomCrop(crop), RandomHorizontalFlip()])(image, label)
    image = Normalize(mean, std)(*ToTensor()(image))[0]          -> out_K   fp32 [3, th, tw]
    label = np.array(label, dtype=np.int64)                      -> tgt_K   int64 [th, tw]

(the reference's ToTensor label line uses the removed np.int, so the label is converted here), the
(x1, y1, flip) it reconstructs by replaying random.Random(seed) in the reference's draw order
(checked against the reference's own output through its pad_image), and the reference's
pad_reflection of an index image (padidx_K: element [y][x] is the flat source index y' * w + x'),
which pins the padding geometry on its own.

Cases, the smallest shapes where the logic can go wrong (h x w, crop = (tw, th)):
  a  10 x 12, (8, 6)     no padding; one seed flipped, one not
  b  10 x 12, (12, 10)   crop equal to the size: no crop draws
  c  10 x 12, (8, 15)    top 2 / bottom 3 (the asymmetric sides), w > tw
  d   3 x 4,  (13, 12)   pads above n - 1: two rounds, both axes
  e  10 x 5,  (9, 6)     w < tw, h > th
  f   2 x 2,  (5, 5)     h = w = 2
  g  10 x 12, (7, 6) and (3, 4)   odd tw and tw < 4
"""
from __future__ import annotations

import argparse
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = (0.29010095242892997, 0.32808144844279574, 0.28696394422942517)      # info.json
STD = (0.1829540508368939, 0.18656561047509476, 0.18447508988480435)

CASES = [            # name, h, w, (tw, th), seeds (None: the first flipped and the first unflipped seed)
    ("a", 10, 12, (8, 6), None),
    ("b", 10, 12, (12, 10), (1, 2)),
    ("c", 10, 12, (8, 15), (1, 2)),
    ("d", 3, 4, (13, 12), (1, 2)),
    ("e", 10, 5, (9, 6), (1, 2)),
    ("f", 2, 2, (5, 5), (1, 2)),
    ("g7", 10, 12, (7, 6), (1, 2)),
    ("g3", 10, 12, (3, 4), (1, 2)),
]


def pads(size, target):
    if size < target:
        lead = (target - size) // 2
        return lead, target - size - lead
    return 0, 0


def replay(seed, h, w, crop):
    """(x1, y1, flip) as RandomCrop then RandomHorizontalFlip draw them from random.seed(seed)."""
    tw, th = crop
    left, right = pads(w, tw)
    top, bottom = pads(h, th)
    pw, ph = w + left + right, h + top + bottom
    r = random.Random(seed)
    x1 = y1 = 0
    if not (pw == tw and ph == th):
        x1 = r.randint(0, pw - tw)
        y1 = r.randint(0, ph - th)
    return x1, y1, r.random() < 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "ingest.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import data_transforms as T
    from PIL import Image

    data = np.random.RandomState(20240)
    arrays, names, flips = {}, [], set()
    k = 0
    for name, h, w, crop, seeds in CASES:
        if seeds is None:
            want, seeds, s = {True, False}, [], 0
            while want:
                f = replay(s, h, w, crop)[2]
                if f in want:
                    want.discard(f)
                    seeds.append(s)
                s += 1
        img = data.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        lab = data.randint(0, 19, size=(h, w)).astype(np.uint8)
        lab[data.rand(h, w) < 0.15] = 255
        for seed in seeds:
            random.seed(seed)
            pim, plab = T.Compose([T.RandomCrop(crop), T.RandomHorizontalFlip()])(
                Image.fromarray(img), Image.fromarray(lab))
            cropped = np.asarray(pim).copy()
            out = T.Normalize(MEAN, STD)(*T.ToTensor()(pim))[0].numpy()
            tgt = np.array(plab, dtype=np.int64)
            tw, th = crop
            assert out.shape == (3, th, tw) and out.dtype == np.float32 and tgt.shape == (th, tw)

            x1, y1, flip = replay(seed, h, w, crop)
            (top, bottom), (left, right) = pads(h, th), pads(w, tw)
            pimg = np.asarray(T.pad_image('reflection', Image.fromarray(img), top, bottom, left, right))
            plb = np.asarray(T.pad_image('constant', Image.fromarray(lab), top, bottom, left, right, value=255))
            want_img, want_lab = pimg[y1:y1 + th, x1:x1 + tw], plb[y1:y1 + th, x1:x1 + tw]
            if flip:
                want_img, want_lab = want_img[:, ::-1], want_lab[:, ::-1]
            assert np.array_equal(cropped, want_img) and np.array_equal(tgt, want_lab), (name, seed)
            padidx = T.pad_reflection(np.arange(h * w, dtype=np.int32).reshape(h, w), top, bottom, left, right)

            arrays[f"img_{k}"], arrays[f"lab_{k}"] = img, lab
            arrays[f"crop_{k}"] = np.asarray(crop, dtype=np.int32)
            arrays[f"seed_{k}"] = np.asarray(seed, dtype=np.int64)
            arrays[f"params_{k}"] = np.asarray([x1, y1, int(flip)], dtype=np.int32)
            arrays[f"out_{k}"], arrays[f"tgt_{k}"] = out, tgt
            arrays[f"padidx_{k}"] = np.ascontiguousarray(padidx)
            names.append(name)
            flips.add(bool(flip))
            k += 1
    assert flips == {True, False}, "both flip values must occur"
    fa = [bool(arrays[f"params_{i}"][2]) for i, n in enumerate(names) if n == "a"]
    assert sorted(fa) == [False, True], fa
    arrays["names"] = np.asarray(names)
    arrays["mean"] = np.asarray(MEAN, dtype=np.float64)
    arrays["std"] = np.asarray(STD, dtype=np.float64)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out}: {k} cases, {os.path.getsize(a.out)} bytes")
    assert os.path.getsize(a.out) < 100 * 1024


if __name__ == "__main__":
    main()
