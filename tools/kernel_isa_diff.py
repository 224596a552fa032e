"""Compare the kernels of two device assembly files (hipcc --cuda-device-only -S), kernel by kernel: for every
`.amdhsa_kernel NAME` the text from `NAME:` to `.end_amdhsa_kernel` -- the instructions and the kernel descriptor with its
register, LDS and scratch figures -- without comments and blank lines and with compiler-local labels renumbered in order of
appearance.  Prints the kernels only one file has and the kernels whose text differs; exit status 1 if there are any.
usage: python tools/kernel_isa_diff.py before.s after.s"""
import re
import sys

LABEL = re.compile(r"\.L(?:BB\d+_\d+|JTI\d+_\d+|tmp\d+|func_end\d+|func_begin\d+|post_getpc\d+)")


def kernels(path):
    lines = open(path).read().split("\n")
    start = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"([A-Za-z_][\w$.]*):", l)] if m}
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        text, seen = [], {}
        for raw in lines[start[name]:end + 1]:
            t = raw.split(";")[0].strip()
            if t:
                text.append(LABEL.sub(lambda k: seen.setdefault(k.group(0), ".L%d" % len(seen)), t))
        out[name] = text
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only = sorted(set(a) ^ set(b))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print("%d kernels | %d kernels" % (len(a), len(b)))
    for k in only:
        print("only in %s: %s" % (sys.argv[1] if k in a else sys.argv[2], k))
    for k in differ:
        print("differs: %s (%d | %d lines)" % (k, len(a[k]), len(b[k])))
    print("%d only in one file, %d differing" % (len(only), len(differ)))
    return 1 if only or differ else 0


if __name__ == "__main__":
    sys.exit(main())
