"""Generate tests/golden/drn_c.N.npz by running the REFERENCE DRN-C modules.

Run where the reference checkout is (it never travels), as make_golden.py:
    python tests/golden/make_drn_c_golden.py [--reference PATH]

The recipe is make_golden.forward_cases (reference lmodels/drnseg.DRNSeg head around
drn.drn_c_26 / drn_c_42, fp32 CPU, weights from drnmi.weights.synth_state_dict, frames from
synth_frames(seed + 100) through the reference data_transforms), with the per-stage records
under DRN's layer numbers ("layer0" = the stem output after its ReLU, "layer1" .. "layer8"):
an arch-C children()[:-2] has the stem as three bare modules, so Sequential index i >= 2 is
DRN layer i - 2.

  c26_2x72x136   drn_c_26, seed 6, frames seed 106, log-probs every 7th pixel
  c42_1x64x128   drn_c_42, seed 7, frames seed 107, log-probs every 7th pixel
  c58_1x32x64    drn_c_58, seed 9, frames seed 109, log-probs every 7th pixel: the Bottleneck trunk,
                 whose layer7 BasicBlock (residual=False) carries a 2048 -> 512 downsample it never runs
  (none has a pixel whose reference top-2 log-prob margin is <= 1e-4)

Also: keys/<arch> for drn_c_26 / drn_c_42 / drn_c_58, a JSON list of [state_dict key, shape]
sorted by key, of the reference DRNSeg-wrapped model.  Data only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402
from make_golden import synth_frames, synth_state_dict  # noqa: E402

CASES = [
    ("c26_2x72x136", "drn_c_26", 6, 2, 72, 136),
    ("c42_1x64x128", "drn_c_42", 7, 1, 64, 128),
    ("c58_1x32x64", "drn_c_58", 9, 1, 32, 64),
]
KEY_ARCHS = ("drn_c_26", "drn_c_42", "drn_c_58")


def forward_cases():
    out = {}
    for name, arch, seed, n, h, w in CASES:
        torch.manual_seed(1234)
        m = G.ref_seg_model(G.REF, arch)
        m.load_state_dict(synth_state_dict(m, seed))
        m.eval()
        frames = synth_frames(seed + 100, n, h, w)
        x = G.preprocess_ref(frames)
        stages = {}
        hooks = [m.layer[i].register_forward_hook(
            (lambda i: lambda mod, a, o: stages.__setitem__(f"layer{i - 2}", o.detach().clone()))(i))
            for i in range(2, len(m.layer))]
        with torch.no_grad():
            logprobs, logits = m(x)
        for hk in hooks:
            hk.remove()
        labels = torch.max(logprobs, 1)[1]
        p = name + "/"
        out[p + "frames"] = frames
        out[p + "input"] = x.numpy()
        out[p + "logits"] = logits.numpy()
        out[p + "labels"] = labels.numpy().astype(np.uint8)
        out[p + "meta"] = np.array([seed, n, h, w], dtype=np.int64)
        srt = np.sort(logprobs.numpy(), axis=1)
        margin = (srt[:, -1] - srt[:, -2]).astype(np.float32)
        out[p + "top2_margin"] = margin
        out[p + "logprobs_sub7"] = logprobs.numpy()[:, :, ::7, ::7].copy()
        for k, v in stages.items():
            vv = v.double()
            out[p + "stage_sum/" + k] = np.array([vv.sum().item(), vv.abs().sum().item()])
            out[p + "stage_crop/" + k] = v[:, :, :4, :4].numpy().copy()
        out[p + "logprob_plane_sum"] = logprobs.double().sum(dim=(2, 3)).numpy()
        print("forward", name, tuple(logprobs.shape), "logit absmax", float(logits.abs().max()),
              "margin <= 1e-4:", int((margin <= 1e-4).sum()), "<= 1e-3:", int((margin <= 1e-3).sum()))
    return out


def key_lists():
    out = {}
    for arch in KEY_ARCHS:
        m = G.ref_seg_model(G.REF, arch)
        out["keys/" + arch] = np.array(json.dumps(sorted([k, list(v.shape)] for k, v in m.state_dict().items())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    args = ap.parse_args()
    G.REF = args.reference
    sys.path.insert(0, G.REF)
    torch.set_num_threads(8)
    arrays = forward_cases()
    arrays.update(key_lists())
    print(G.save_parts(os.path.join(HERE, "drn_c"), arrays))


if __name__ == "__main__":
    main()
