"""asm_table.txt of this directory: per-kernel comparison of two trees' device assembly
(profiles/sp24_fold/make_asm_table.py, adapted: a file of the new tree may stand for several of the parent's).

    python make_asm_table.py PARENT_DIR NEW_DIR conv_sp24=conv_sp24+conv_sp24_i8 conv_big > asm_table.txt

PARENT_DIR / NEW_DIR hold FILE.s as written by build.py's flags and per-file extras plus
--offload-device-only -S.  NEW=OLD1+OLD2 compares NEW.s of the new tree with the kernels of OLD1.s and OLD2.s
of the parent.  Kernels are matched by demangled name (the two packers became sp24_pack_kernel<T>: RENAMED).
Per kernel symbol the text between its label and .Lfunc_end is compared with comments dropped and local
labels renumbered in order of appearance (profiles/q8_fold/README.txt).
Columns: parent file, kernel, identical, parent and new next_free_vgpr / next_free_sgpr / accum_offset /
private_segment_fixed_size / group_segment_fixed_size, parent and new line counts.  The last column says
whether a hard condition is broken: more VGPRs, SGPRs or a higher accum offset than the parent, a private
segment, another group segment."""
import re
import subprocess
import sys

RES = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"]
RENAMED = {"sp24_pack_kernel(": "sp24_pack_kernel<unsigned short>(", "sp24_pack_i8_kernel(": "sp24_pack_kernel<signed char>("}


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
    syms = [k for k in kernels if k in res]
    r = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True)
    out = {}
    for k, name in zip(syms, r.stdout.strip().split("\n")):
        name = name.replace("drnmi::(anonymous namespace)::", "").replace("(drnmi_conv_args)", "").replace("void ", "")
        labels = {}
        norm = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), s) for s in kernels[k]]
        out[name] = (norm, [res[k].get(r, "?") for r in RES])
    return out


def broken(a, b):
    a, b = [int(v) for v in a], [int(v) for v in b]
    return a[0] < b[0] or a[1] < b[1] or a[2] < b[2] or b[3] != 0 or a[4] != b[4]


def main():
    pdir, ndir, specs = sys.argv[1], sys.argv[2], sys.argv[3:]
    rows, same, total, bad = [], 0, 0, 0
    for spec in specs:
        new, _, olds = spec.partition("=")
        b = parse(f"{ndir}/{new}.s")
        seen = set()
        for f in (olds or new).split("+"):
            for k, (text, res) in parse(f"{pdir}/{f}.s").items():
                total += 1
                nk = k
                for old, now in RENAMED.items():
                    if k.startswith(old):
                        nk = now + k[len(old):]
                if nk not in b:
                    rows.append((f, k, "GONE", "/".join(res), "-", len(text), 0, ""))
                    continue
                seen.add(nk)
                ident = text == b[nk][0]
                same += ident
                over = broken(res, b[nk][1])
                bad += over
                rows.append((f, nk, "yes" if ident else "NO", "/".join(res), "/".join(b[nk][1]), len(text), len(b[nk][0]),
                             "BROKEN" if over else ""))
        rows += [(new, k, "NEW", "-", "/".join(b[k][1]), 0, len(b[k][0]), "") for k in b if k not in seen]
    w = min(72, max(len(r[1]) for r in rows))
    for r in rows:
        print(f"{r[0]:<12} {r[1][:w]:<{w}} {r[2]:<4} {r[3]:<20} {r[4]:<20} {r[5]:>6} {r[6]:>6} {r[7]}")
    print(f"{same} of {total} kernels identical, {bad} break a hard condition")


if __name__ == "__main__":
    main()
