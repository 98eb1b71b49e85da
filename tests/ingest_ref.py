"""numpy restatement of drnmi_train_ingest_u8 (include/drnmi.h): a gather through the index tables
of drnmi.data.index_maps plus the fp32 normalise.  tests/test_data_ingest.py pins it bit for bit
against the reference's tensors (tests/golden/ingest.npz); the GPU tests compare the kernel with it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest.npz")


def load_cases():
    """The fixture as a list of dicts: name, img, lab, crop (tw, th), seed, params (x1, y1, flip),
    out fp32 [3, th, tw], tgt int64 [th, tw], padidx; plus (mean, std)."""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = []
    for k, name in enumerate(z["names"]):
        x1, y1, fl = (int(v) for v in z[f"params_{k}"])
        cases.append(dict(name=str(name), img=z[f"img_{k}"], lab=z[f"lab_{k}"],
                          crop=tuple(int(v) for v in z[f"crop_{k}"]), seed=int(z[f"seed_{k}"]),
                          params=(x1, y1, bool(fl)), out=z[f"out_{k}"], tgt=z[f"tgt_{k}"],
                          padidx=z[f"padidx_{k}"]))
    return cases, tuple(float(v) for v in z["mean"]), tuple(float(v) for v in z["std"])


def decode(table, size):
    """(source index clamped into [0, size - 1], padded flag) of int32 table entries."""
    table = np.asarray(table, dtype=np.int32)
    pad = table < 0
    src = np.where(pad, ~table, table)
    return np.clip(src, 0, size - 1), pad


def ingest_ref(img, lab, rowmap, colmap, mean, std):
    """img uint8 [h, w, 3], lab uint8 [h, w] or None -> (fp32 [3, th, tw], int64 [th, tw] or None):
    (float32(u8) / 255 - float32(mean)) / float32(std), each step rounded to fp32."""
    h, w = img.shape[:2]
    r, rpad = decode(rowmap, h)
    q, cpad = decode(colmap, w)
    g = img[r[:, None], q[None, :]].astype(np.float32)                       # [th, tw, 3]
    m = np.asarray(mean, dtype=np.float32)
    s = np.asarray(std, dtype=np.float32)
    out = ((g / np.float32(255.0) - m) / s).astype(np.float32).transpose(2, 0, 1)
    tgt = None
    if lab is not None:
        tgt = lab[r[:, None], q[None, :]].astype(np.int64)
        tgt[rpad[:, None] | cpad[None, :]] = 255
    return np.ascontiguousarray(out), tgt
