"""One-off for the packer fold (README.txt §2): sha256 of every blob that test_pack_counts_violations of
tests/test_gpu_sp24.py and tests/test_gpu_sp24_i8.py packs (the clean matrices and the violating ones, guard
tail included), with the library DRNMI_LIB selects.  Run once per library and compare the two outputs.

    DRNMI_LIB=PARENT/libdrnmi.so python profiles/sp24_twins/pack_digests.py > pack_digests_parent.json
    python profiles/sp24_twins/pack_digests.py > pack_digests_new.json
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "video-seg-model-compress_amd"), REPO, os.path.join(REPO, "tests")]

import test_gpu_sp24  # noqa: E402
import test_gpu_sp24_i8  # noqa: E402

out = {}
for name, mod, blob_at in (("bf16", test_gpu_sp24, 1), ("int8", test_gpu_sp24_i8, 0)):
    packed = []

    def recording(*args, _pack=mod._pack, _packed=packed, _at=blob_at):
        r = _pack(*args)
        _packed.append({"sha256": hashlib.sha256(r[_at].cpu().numpy().tobytes()).hexdigest(), "violations": r[-1]})
        return r

    mod._pack = recording
    mod.test_pack_counts_violations()
    out[name] = packed
print(json.dumps(out, indent=1))
