"""Records wgrad_bytes.json: the sha256 of the raw dw buffer after each of the two launches
(accumulate 0, then 1) of every case of tests/test_gpu_wgrad_bytes.py, as the library it is run
against writes it.  Run once on an MI355X, on the commit before the weight-gradient tiles were folded
into one template.  The conditions the test puts on the data (every element finite and nonzero, the
edge cases on their kernels, nothing written outside dw or the queried workspace) are checked here too.

    python tests/golden/make_wgrad_bytes_golden.py [out.json] [path/to/libdrnmi.so]
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
    import test_gpu_wgrad_bytes as T
    out = {}
    for name in sorted(T.CASES):
        bufs, kernel = T.run_case(name)
        T.check_case(name, bufs, kernel)
        out[name] = [T.digest(b) for b in bufs]
        print(out[name][0], out[name][1], _lib.WGRAD_KERNELS[kernel], name)
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_bytes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
