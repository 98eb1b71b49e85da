"""SRMB masks on their live channels (include/drnmi.h DRNMI_BF16_PSP, csrc/conv_psp.hip), the host side:
the new symbols, drnmi_psp_pack on masks from SRMBRepMasker.construct_mask (eligible: the blob unpacks to the
masked weight exactly; anything else: a violation count) and the DRNSeg switch.  No GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from drnmi import _lib
from drnmi.pruners import SRMBRepMasker, SRMBRepMaskerConfig

HEADER = Path(__file__).resolve().parents[1] / "include" / "drnmi.h"
# (cbh, cbw, ib, isp) -> the (P, d) the pack must find
MASKS = [((8, 32), 1, 0.5, (32, 16)), ((8, 64), 1, 0.75, (64, 16)), ((8, 64), 1, 0.875, (64, 8)), ((16, 32), 2, 0.75, (32, 8))]


def srmb_weight(cout, cin, ks, cb, ib, isp, seed=0):
    """Masked bf16 weights in the packed order [cout][ks*ks*cin] (k = tap * cin + ci), as int16 bits."""
    np.random.seed(seed)
    cfg = SRMBRepMaskerConfig(-1, -1, cb[0], cb[1], ib, ib, 0, "RAMANUJAN", isp, "RAMANUJAN", True, True, 0.5, False)
    mask = SRMBRepMasker.construct_mask(np.zeros((cout, cin, ks, ks), np.float32), cfg)
    w = np.where(mask != 0, np.random.randint(1, 4, size=mask.shape) * np.random.choice([-1, 1], size=mask.shape), 0)
    w = torch.from_numpy(w.astype(np.float32)).permute(0, 2, 3, 1).reshape(cout, ks * ks * cin)
    return w.to(torch.bfloat16).contiguous().view(torch.int16).numpy()


def psp_pack(w, cin, ks):
    """-> (variant, violations, blob or None)"""
    lib = _lib.load()
    variant, viol = ctypes.c_int32(-9), ctypes.c_int32(-9)
    args = (w.ctypes.data, w.shape[0], cin, ks)
    _lib.check(lib.drnmi_psp_pack(*args, None, 0, ctypes.byref(variant), ctypes.byref(viol)), "psp_pack")
    if variant.value < 0:
        return -1, viol.value, None
    nbytes = lib.drnmi_psp_pack_bytes(w.shape[0], cin, ks, variant.value)
    blob = np.full(nbytes + 64, 0xA5, np.uint8)
    _lib.check(lib.drnmi_psp_pack(*args, blob.ctypes.data, nbytes, ctypes.byref(variant), ctypes.byref(viol)), "psp_pack")
    assert (blob[nbytes:] == 0xA5).all(), "the packer wrote past drnmi_psp_pack_bytes"
    return variant.value, viol.value, blob[:nbytes]


def test_symbols_agree():
    text = HEADER.read_text()
    lib = _lib.load()
    for name in ("drnmi_psp_pack", "drnmi_psp_pack_bytes"):
        assert re.search(rf"\b{name}\(", text) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r"DRNMI_BF16_PSP = (\d+)", text).group(1)) == _lib.DRNMI_BF16_PSP
    assert lib.drnmi_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("cb,ib,isp,pd", MASKS, ids=lambda v: str(v))
@pytest.mark.parametrize("ks", [3, 1])
def test_pack_roundtrip(cb, ib, isp, pd, ks):
    cout, cin = 128, 512
    w = srmb_weight(cout, cin, ks, cb, ib, isp)
    variant, viol, blob = psp_pack(w, cin, ks)
    assert viol == 0 and _lib.PSP_VARIANTS[variant] == pd
    P, d = pd
    hdr = blob[:64].view(np.int32)
    kc = ks * ks * cin * d // P
    assert list(hdr[:8]) == [0x31505350, cout, cin, ks, P, d, P // d, kc]
    perm = blob[64:64 + 4 * cout].view(np.int32)
    order = blob[64 + 4 * cout:64 + 8 * cout].view(np.int32)
    ns = cout // 16 * ks * ks * d
    s = blob[64 + 8 * cout:64 + 8 * cout + ns].reshape(cout // 16, ks * ks, d).astype(np.int64)
    vals = blob[64 + 8 * cout + (ns + 15) // 16 * 16:].view(np.int16).reshape(cout, ks * ks, cin // P, d)
    assert sorted(perm) == list(range(cout)) and sorted(order) == list(range(128))
    assert (np.diff(perm[order]) > 0).all()
    back = np.zeros((cout, ks * ks, cin // P, P), np.int16)
    src = np.arange(d) + d * s                                            # [fragment][tap][v] -> channel inside a period
    for r in range(cout):
        for tap in range(ks * ks):
            back[perm[r], tap][:, src[r // 16, tap]] = vals[r, tap]
    assert np.array_equal(back.reshape(cout, -1), w)
    assert blob.nbytes - 64 - 8 * cout - (ns + 15) // 16 * 16 == w.nbytes * d // P


def test_most_compact_structure():
    """cbh 32: the union of four classes' supports (H = 8) is itself a valid, coarser structure; the pack must
    take the mask's own (P, d), not the first that fits."""
    w = srmb_weight(512, 256, 1, (32, 64), 1, 0.75)
    variant, viol, blob = psp_pack(w, 256, 1)
    assert viol == 0 and _lib.PSP_VARIANTS[variant] == (64, 16)


def test_rejections():
    cin, ks = 256, 3
    good = srmb_weight(128, cin, ks, (8, 32), 1, 0.5)
    assert psp_pack(good, cin, ks)[:2] == (0, 0)
    extra = good.copy()
    r, k = np.argwhere(extra == 0)[1234]
    extra[r, k] = 0x3F80                                                   # one extra live weight
    variant, viol, _ = psp_pack(extra, cin, ks)
    assert variant == -1 and viol >= 1
    rows8 = srmb_weight(128, cin, ks, (16, 32), 1, 0.5)                    # 16 classes of 8 rows
    assert psp_pack(rows8, cin, ks)[0] == -1 and psp_pack(rows8, cin, ks)[1] >= 1
    dense = np.full((128, ks * ks * cin), 0x3F80, np.int16)
    assert psp_pack(dense, cin, ks)[0] == -1 and psp_pack(dense, cin, ks)[1] >= 1
    short = srmb_weight(128, 128, ks, (8, 64), 1, 0.875)                   # K step 256 channels, cin 128
    assert psp_pack(short, 128, ks)[0] == -1 and psp_pack(short, 128, ks)[1] >= 1
    assert _lib.load().drnmi_psp_pack_bytes(128, 128, ks, 2) == -1


def test_switch():
    from drnmi.drnseg import DRNSeg
    m = DRNSeg("drn_d_22", 19, pretrained=False)
    assert m.srmb_sparse is False and m.srmb_sparse_layers() == []
    assert m.set_srmb_sparse(True) is m and m.srmb_sparse is True
    assert m.srmb_sparse_layers() == []                                    # fp32: untouched, no error
    import pickle
    assert pickle.loads(pickle.dumps(m)).srmb_sparse is True
    assert m.set_srmb_sparse(False).srmb_sparse_layers() == []
