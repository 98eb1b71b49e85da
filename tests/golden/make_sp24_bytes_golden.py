"""Records sp24_bytes.json: the sha256 of the output of every launch of tests/test_gpu_sp24_bytes.py
(each case of tests/test_gpu_sp24.py::CASES, fp32 NCHW and bf16 NHWC, the gather and where it exists the
forced strip form), as the library it is run against writes it.  Run once on an MI355X, on the commit
before conv_big_body moved to its own header and the launchers onto launch_lds.

    python tests/golden/make_sp24_bytes_golden.py [out.json] [path/to/libdrnmi.so]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "video-seg-model-compress_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    from drnmi import _lib
    _lib.load(sys.argv[2] if len(sys.argv) > 2 else None)
    import test_gpu_sp24_bytes as T
    out = {}
    for name in sorted(T.CASES):
        out[name] = T.run_case(name)
        for key in sorted(out[name]):
            print(out[name][key], key, name)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sp24_bytes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
