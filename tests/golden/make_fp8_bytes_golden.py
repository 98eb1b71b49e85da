"""Records fp8_conv_bytes.json: the sha256 of the raw output buffer of every launch of
tests/test_gpu_fp8_bytes.py, as the library it is run against writes it.  Run once on an MI355X, on
the commit that added fp8 (before the int8 and fp8 epilogues were folded into one).

    python tests/golden/make_fp8_bytes_golden.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "video-seg-model-compress_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    import test_gpu_fp8_bytes as T
    out = {name: T.digest(T.run_case(name)) for name in sorted(T.CASES)}
    with open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fp8_conv_bytes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, d in out.items():
        print(d, name)


if __name__ == "__main__":
    main()
