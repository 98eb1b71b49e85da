"""Generate tests/golden/drn_d_more.N.npz by running the REFERENCE DRN-D modules no other fixture
covers: drn_d_24 / 40 / 56 (two conv+BN+ReLU units in layer7 and layer8) and drn_d_105 / 107 (23
Bottlenecks in layer5).

Run where the reference checkout is (it never travels), as make_golden.py:
    python tests/golden/make_drn_d_more_golden.py [--reference PATH]

The recipe is make_golden.forward_cases (reference lmodels/drnseg.DRNSeg head around drn.<arch>, fp32
CPU, weights from drnmi.weights.synth_state_dict, frames from synth_frames(seed + 100) through the
reference data_transforms, per-stage records "layer0" .. "layer8", log-probs every 7th pixel).
forward.N.npz is not touched.

A case's seed is the first of SEEDS[case] that meets both conditions (checked here, on the CPU):
  * no pixel has a reference top-2 log-prob margin <= 1e-4, so the GPU label gate excludes nothing;
  * the fp64 evaluation of oracle/drn_oracle.py on the same weights and input lies within 2.5e-4
    max-abs of the reference's fp32 logits: a quarter of the 1e-3 fp32 gate, so the fixture's own
    fp32 evaluation noise (up to 111 layers) does not spend the gate.
What the run that wrote the committed files printed:

  d24_2x72x136  seed 27 (24, 25, 26 had 1, 7, 3 px at or below the margin): logits (2, 19, 9, 17) absmax
                8.879, px with margin <= 1e-4: 0 (smallest margin 1.95e-04), fp64 vs fp32 logits 5.43e-06
  d40_1x64x128  seed 42 (40, 41 had 1, 2 px): logits (1, 19, 8, 16) absmax 9.610, px with margin <= 1e-4: 0
                (smallest margin 2.07e-04), fp64 vs fp32 logits 7.83e-06
  d56_1x64x128  seed 56: logits (1, 19, 8, 16) absmax 25.298, px with margin <= 1e-4: 0 (smallest margin
                2.17e-04), fp64 vs fp32 logits 2.46e-05
  d105_1x32x64  seed 105: logits (1, 19, 4, 8) absmax 19.017, px with margin <= 1e-4: 0 (smallest margin
                9.02e-04), fp64 vs fp32 logits 1.75e-05
  d107_1x32x64  seed 208 (207 had 4 px): logits (1, 19, 4, 8) absmax 19.880, px with margin <= 1e-4: 0
                (smallest margin 1.05e-03), fp64 vs fp32 logits 1.64e-05
  (no rejected seed missed the fp64 condition: the worst of all seeds tried was 2.46e-05)

Also: keys/<arch> for the five archs, a JSON list of [state_dict key, shape] sorted by key, of the
reference DRNSeg-wrapped model.  Data only.
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as G  # noqa: E402
from make_golden import synth_frames, synth_state_dict  # noqa: E402
from oracle import drn_oracle as O  # noqa: E402

# (case, arch, candidate seeds in the order tried, n, h, w)
CASES = [
    ("d24_2x72x136", "drn_d_24", range(24, 40), 2, 72, 136),
    ("d40_1x64x128", "drn_d_40", range(40, 56), 1, 64, 128),
    ("d56_1x64x128", "drn_d_56", range(56, 72), 1, 64, 128),
    ("d105_1x32x64", "drn_d_105", range(105, 121), 1, 32, 64),
    ("d107_1x32x64", "drn_d_107", range(207, 223), 1, 32, 64),
]
KEY_ARCHS = ("drn_d_24", "drn_d_40", "drn_d_56", "drn_d_105", "drn_d_107")
MARGIN = 1e-4
FP64_DIST = 2.5e-4


def fp64_logits(sd, arch, x):
    """The seg logits of oracle/drn_oracle.py evaluated in fp64 on fp32 weights and input."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    with torch.no_grad():
        feat, _ = O.backbone(sd, arch, x.double())
        return O._conv(sd, "seg", feat, bias=True)


def one_case(name, arch, seed, n, h, w):
    torch.manual_seed(1234)
    m = G.ref_seg_model(G.REF, arch)
    m.load_state_dict(synth_state_dict(m, seed))
    m.eval()
    frames = synth_frames(seed + 100, n, h, w)
    x = G.preprocess_ref(frames)
    stages = {}
    hooks = [m.layer[i].register_forward_hook(
        (lambda i: lambda mod, a, o: stages.__setitem__(f"layer{i}", o.detach().clone()))(i))
        for i in range(len(m.layer))]
    with torch.no_grad():
        logprobs, logits = m(x)
    for hk in hooks:
        hk.remove()
    labels = torch.max(logprobs, 1)[1]
    srt = np.sort(logprobs.numpy(), axis=1)
    margin = (srt[:, -1] - srt[:, -2]).astype(np.float32)
    dist = float((fp64_logits(m.state_dict(), arch, x) - logits.double()).abs().max())
    near = int((margin <= MARGIN).sum())
    print(f"forward {name} seed {seed}: logits {tuple(logits.shape)} absmax {float(logits.abs().max()):.3f}, "
          f"px with margin <= 1e-4: {near} (smallest margin {float(margin.min()):.2e}), "
          f"fp64 oracle vs fp32 reference logits max-abs {dist:.2e}, labels used {len(labels.unique())}")
    if near or dist > FP64_DIST:
        return None
    out, p = {}, name + "/"
    out[p + "frames"] = frames
    out[p + "input"] = x.numpy()
    out[p + "logits"] = logits.numpy()
    out[p + "labels"] = labels.numpy().astype(np.uint8)
    out[p + "meta"] = np.array([seed, n, h, w], dtype=np.int64)
    out[p + "top2_margin"] = margin
    out[p + "logprobs_sub7"] = logprobs.numpy()[:, :, ::7, ::7].copy()
    for k, v in stages.items():
        vv = v.double()
        out[p + "stage_sum/" + k] = np.array([vv.sum().item(), vv.abs().sum().item()])
        out[p + "stage_crop/" + k] = v[:, :, :4, :4].numpy().copy()
    out[p + "logprob_plane_sum"] = logprobs.double().sum(dim=(2, 3)).numpy()
    return out


def forward_cases():
    out = {}
    for name, arch, seeds, n, h, w in CASES:
        for seed in seeds:
            got = one_case(name, arch, seed, n, h, w)
            if got is not None:
                out.update(got)
                break
        else:
            raise SystemExit(f"{name}: no seed of {list(seeds)} meets the conditions")
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
    print(G.save_parts(os.path.join(HERE, "drn_d_more"), arrays))


if __name__ == "__main__":
    main()
