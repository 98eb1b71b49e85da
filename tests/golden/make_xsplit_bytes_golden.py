"""Records xsplit_bytes.json: the sha256 digests of every launch of tests/test_gpu_xsplit_bytes.py, as the
library it is run against writes them.  Run on an MI355X, on the commit before the fp32x2 conv and
weight-gradient kernels were folded into the fp32x family's headers; twice, in two processes, and the file is
kept only if both recordings agree.  The conditions the test puts on the data (no element left unwritten,
nothing written outside dw or the queried workspace) are checked here too.

    python tests/golden/make_xsplit_bytes_golden.py [out.json] [path/to/libdrnmi.so]
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
    import test_gpu_xsplit_bytes as T
    out = {}
    for name in sorted(T.CONV_CASES):
        out[name] = T.run_conv(name)
        print(*(d[:16] for d in out[name]), name)
    for fn in T.WGRAD_ENTRIES:
        out[fn] = T.run_wgrad(fn)
        print(*(d[:16] for d in out[fn]), fn)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "xsplit_bytes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
