"""asm_table.txt of this directory: per-kernel comparison of two trees' device assembly.

    python make_asm_table.py PARENT_DIR NEW_DIR conv_big conv_sp24 conv_halo > asm_table.txt

PARENT_DIR / NEW_DIR hold FILE.s as written by build.py's flags and per-file extras plus
--cuda-device-only -S.  Per kernel symbol the text between its label and .Lfunc_end is compared with
comments dropped and local labels renumbered in order of appearance (profiles/q8_fold/README.txt).
Columns: file, kernel, identical, parent and new next_free_vgpr / next_free_sgpr / accum_offset /
private_segment_fixed_size / group_segment_fixed_size, parent and new line counts."""
import re
import subprocess
import sys

RES = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]


def parse(path):
    text = open(path).read().split("\n")
    kernels, res = {}, {}
    cur, body = None, []
    for ln in text:
        m = re.match(r"^(_Z\w+):", ln)
        if cur is None and m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                kernels[cur] = body
                cur = None
                continue
            s = ln.split(";")[0].rstrip()
            if s.strip():
                body.append(s)
    ksym = None
    for ln in text:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            ksym = m.group(1)
            res[ksym] = {}
        m = re.match(r"^\s*\.amdhsa_(\w+)\s+(\S+)", ln)
        if m and ksym and m.group(1) in RES:
            res[ksym][m.group(1)] = m.group(2)
        if ".end_amdhsa_kernel" in ln:
            ksym = None
    out = {}
    for k, body in kernels.items():
        if k not in res:
            continue
        labels = {}
        norm = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), s) for s in body]
        out[k] = (norm, "/".join(res[k].get(r, "?") for r in RES))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    clean = [s.replace("drnmi::(anonymous namespace)::", "").replace("(drnmi_conv_args)", "").replace("void ", "")
             for s in r.stdout.strip().split("\n")]
    return dict(zip(names, clean))


def main():
    pdir, ndir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    rows, same, total = [], 0, 0
    for f in files:
        a, b = parse(f"{pdir}/{f}.s"), parse(f"{ndir}/{f}.s")
        names = demangle(list(a) + [k for k in b if k not in a])
        for k in a:
            total += 1
            if k not in b:
                rows.append((f, names[k], "GONE", a[k][1], "-", len(a[k][0]), 0))
                continue
            ident = a[k] == b[k]
            same += ident
            rows.append((f, names[k], "yes" if ident else "NO", a[k][1], b[k][1], len(a[k][0]), len(b[k][0])))
        rows += [(f, names[k], "NEW", "-", b[k][1], 0, len(b[k][0])) for k in b if k not in a]
    w = min(72, max(len(r[1]) for r in rows))
    for r in rows:
        print(f"{r[0]:<10} {r[1][:w]:<{w}} {r[2]:<4} {r[3]:<20} {r[4]:<20} {r[5]:>6} {r[6]:>6}")
    print(f"{same} of {total} kernels identical")


if __name__ == "__main__":
    main()
