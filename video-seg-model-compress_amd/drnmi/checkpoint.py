"""Checkpoints that carry the pruner's masks.

The reference saves {epoch, arch, state_dict, best_miou, optimizer, dataset} with torch.save and
copies the best one (semantic_seg.py:286-290, called at :1085-1092) but never the masks: a resumed
SRMB run (unseeded np.random, SRMBRepMasker.py:102-334) or pr_static run re-draws different masks.
Here the masks go next to the checkpoint in the compact form of Pruner.save_masks (SRMB masks as
their period-tile factors, everything else 1 bit per weight), and resume() restores both.

  save_checkpoint(state, is_best, save_dir=".", filename="checkpoint.pth.tar", pruner=None, int8_model=None)
  resume(path, model, optimizer=None, pruner=None, int8=False) -> state

The calibrated int8 activation scales (DRNSeg.int8_state) travel the same way, as
<checkpoint>.int8.json: a deployed int8 model loads them and needs no calibration frames.
"""
from __future__ import annotations

import json
import os
import shutil

import torch


def mask_path(checkpoint_path: str) -> str:
    return checkpoint_path + ".masks.npz"


def int8_path(checkpoint_path: str) -> str:
    return checkpoint_path + ".int8.json"


def save_checkpoint(state, is_best, save_dir=".", filename="checkpoint.pth.tar", pruner=None, int8_model=None):
    """semantic_seg.py:286-290, plus the pruner's masks (<checkpoint>.masks.npz) and, with
    int8_model= (a calibrated DRNSeg), its activation scales (<checkpoint>.int8.json; a float's
    repr in JSON round-trips exactly); the best copy (checkpoint_best.pth.tar) gets both copied too."""
    fpath = os.path.join(save_dir, filename)
    torch.save(state, fpath)
    if pruner is not None:
        pruner.save_masks(mask_path(fpath))
    if int8_model is not None:
        with open(int8_path(fpath), "w") as f:
            json.dump(int8_model.int8_state(), f, indent=1, sort_keys=True, allow_nan=False)
    if is_best:
        best = os.path.join(save_dir, "checkpoint_best.pth.tar")
        shutil.copyfile(fpath, best)
        if pruner is not None:
            shutil.copyfile(mask_path(fpath), mask_path(best))
        if int8_model is not None:
            shutil.copyfile(int8_path(fpath), int8_path(best))


def resume(path, model, optimizer=None, pruner=None, int8=False):
    """The reference's --resume (semantic_seg.py:973-990) with the masks restored instead of
    re-drawn: loads the state dict (weights_only -- no code runs from the file), the optimizer
    state if given, and the pruner's masks if the checkpoint has them.  int8=True also installs
    the saved activation scales (DRNSeg.load_int8_state).  Returns the state."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(state["state_dict"])
    if optimizer is not None and "optimizer" in state:
        optimizer.load_state_dict(state["optimizer"])
    if pruner is not None:
        mp = mask_path(path)
        if not os.path.exists(mp):
            raise FileNotFoundError(f"{mp}: this checkpoint was saved without masks")
        pruner.load_masks(mp)
    if int8:
        ip = int8_path(path)
        if not os.path.exists(ip):
            raise FileNotFoundError(f"{ip}: this checkpoint was saved without int8 activation scales")
        with open(ip) as f:
            model.load_int8_state(json.load(f))
    return state


__all__ = ["save_checkpoint", "resume", "mask_path", "int8_path"]
