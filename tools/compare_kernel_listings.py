#!/usr/bin/env python3
"""Function-by-function comparison of two ISA listings of one source (hipcc -S --cuda-device-only): which kernels and device functions
exist on either side, and whether each common one has the same instruction stream, the same .amdhsa_ descriptor values and the same
resource symbols.  Reads listings only.
usage: compare_kernel_listings.py BEFORE.s AFTER.s [--drop SUBSTRING:I,J,... [--keep-values V,W,...]]
--drop: for a change that removes template parameters.  In every symbol of BEFORE that contains SUBSTRING followed by a template argument
list, the I-th, J-th, ... integral arguments (1-based) are removed before the two sides are matched; the functions in which a removed
argument had another value than --keep-values (default: all 0) are expected to be absent from AFTER and are listed as dropped."""
import argparse, re, sys
from collections import Counter

ap = argparse.ArgumentParser()
ap.add_argument("before"); ap.add_argument("after")
ap.add_argument("--drop", default="")
ap.add_argument("--keep-values", default="")
args = ap.parse_args()
GONE = "<dropped:"


def rename(text, sub, idx, keep):
    def f(m):
        ts = re.findall(r"L[a-z]n?\d+E", m.group(1))
        vals = [int(re.search(r"(\d+)E", ts[i - 1]).group(1)) for i in idx]
        if vals != keep:
            return sub + "I" + GONE + ",".join(map(str, vals)) + ">" + m.group(1)
        return sub + "I" + "".join(t for i, t in enumerate(ts, 1) if i not in idx)
    return re.sub(re.escape(sub) + r"I((?:L[a-z]n?\d+E)+)", f, text)


def functions(text):
    """name -> (is a kernel, normalised lines of the body incl. the descriptor, and the .set resource symbols)"""
    lines = text.split("\n")
    funcs = {m.group(1) for l in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", l))}
    kern = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out, cur = {}, None
    for l in lines:
        if cur is None:
            m = re.match(r"(\S+):", l)
            if m and m.group(1) in funcs:
                cur = m.group(1); out[cur] = []
                continue
            m = re.match(r"\s*\.set\s+(\S+)\.(\w+),\s*(.*)", l)
            if m and m.group(1) in out:
                out[m.group(1)].append(".set %s, %s" % (m.group(2), m.group(3)))
            continue
        if re.match(r"\.Lfunc_end\d+:", l):
            cur = None
            continue
        l = l.split(";")[0].strip()
        if l:
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", l))
    return out, kern


ta, tb = open(args.before).read(), open(args.after).read()
if args.drop:
    sub, idx = args.drop.split(":")
    idx = [int(i) for i in idx.split(",")]
    keep = [int(v) for v in args.keep_values.split(",")] if args.keep_values else [0] * len(idx)
    ta = rename(ta, sub, idx, keep)
(A, KA), (B, KB) = functions(ta), functions(tb)
gone = sorted(n for n in A if GONE in n)
A = {n: v for n, v in A.items() if GONE not in n}
only_a, only_b = sorted(set(A) - set(B)), sorted(set(B) - set(A))
same = [n for n in A if n in B and A[n] == B[n]]
diff = [n for n in A if n in B and A[n] != B[n]]
nk = lambda names, K: sum(n in K for n in names)
print("before: %d kernels + %d other functions (dropped by --drop: %d + %d); after: %d + %d" % (
    nk(A, KA) + nk(gone, KA), len(A) + len(gone) - nk(A, KA) - nk(gone, KA), nk(gone, KA), len(gone) - nk(gone, KA), nk(B, KB), len(B) - nk(B, KB)))
print("identical (instructions, descriptor, resources): %d kernels + %d other; different: %d; only before: %d; only after: %d" % (
    nk(same, KA), len(same) - nk(same, KA), len(diff), len(only_a), len(only_b)))
for n in gone:
    print("  dropped", n)
for n in diff:
    d = sum((Counter(A[n]) - Counter(B[n])).values()), sum((Counter(B[n]) - Counter(A[n])).values())
    print("  DIFFERENT %s: %d lines before, %d after; %d / %d lines without a counterpart" % (n, len(A[n]), len(B[n]), d[0], d[1]))
for n in only_a:
    print("  ONLY BEFORE", n)
for n in only_b:
    print("  ONLY AFTER", n)
sys.exit(1 if (diff or only_a or only_b) else 0)
