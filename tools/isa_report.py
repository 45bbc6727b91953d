"""Summarise kernels in a hipcc -S device assembly file: loads, VGPR/SGPR, spills.

usage: python tools/isa_report.py fjagg.s [substring-of-demangled-name ...]
       python tools/isa_report.py --jsonl fjagg.s [base.jsonl] > table.jsonl
       python tools/isa_report.py --compare before.jsonl after.jsonl [family-name ...]

--jsonl writes one JSON row per function symbol (kernels, and device functions kept out of line):
the demangled name up to its argument list (anonymous-namespace qualifiers dropped), a digest of
its instruction text with labels normalised, the instruction count n, and for kernels
next_free_vgpr, next_free_sgpr, private segment size (scratch) and group segment size (lds).
With base.jsonl the table holds a header row naming that file (looked up beside the table) and
only the rows that are new or differ from it; --compare reads such a table as base plus rows.

--compare checks a refactor of the named kernel families against the table of its parent: no
symbol appears or disappears (names are matched up to the argument list), every function outside
the families keeps its digest, every kernel inside keeps its VGPR count, private segment size
(which must be 0) and group segment size. Exit status 1 when a check fails.
"""
import hashlib
import json
import os
import re
import subprocess
import sys


def functions(s):
    """(mangled, demangled, body, metadata-or-None) of every function in the assembly text."""
    names = re.findall(r"^(_Z\S+):\s*;", s, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True).stdout.split("\n")
    for n, d in zip(names, dem):
        start = s.index("\n" + n + ":") + 1
        body = s[start:s.index(".Lfunc_end", start)]
        meta_i = s.find(".amdhsa_kernel " + n + "\n")
        meta = s[meta_i:s.find(".end_amdhsa_kernel", meta_i)] if meta_i >= 0 else None
        yield n, d, body, meta


def meta_get(meta, key):
    m = re.search(r"\." + key + r"\s+(\d+)", meta or "")
    return int(m.group(1)) if m else None


def instructions(body):
    """The function's instructions, one per entry: comments, directives and the function's own
    label dropped, basic-block labels kept with the function's index taken out of them."""
    out = []
    for l in body.splitlines()[1:]:
        l = l.split(";")[0].strip()
        if not l or (l.startswith(".") and not l.endswith(":")):
            continue
        out.append(re.sub(r"\.L(BB|JTI|func_end|tmp)\d+", r".L\1", l))
    return out


def short(name):
    """The demangled name up to its argument list (template arguments kept), without
    anonymous-namespace qualifiers and the return type."""
    name = name.replace("(anonymous namespace)::", "")
    depth = 0
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return name[5:] if name.startswith("void ") else name


def load(path):
    rows = [json.loads(l) for l in open(path)]
    table = {}
    if rows and "base" in rows[0]:
        table = load(os.path.join(os.path.dirname(path), rows.pop(0)["base"]))
    table.update((r["name"], r) for r in rows)
    return table


def jsonl(path, base=None):
    old = load(base) if base else {}
    rows = []
    for n, d, body, meta in functions(open(path).read()):
        ins = instructions(body)
        rows.append({
            "name": short(d),
            "digest": hashlib.sha256("\n".join(ins).encode()).hexdigest()[:12],
            "n": sum(not i.endswith(":") for i in ins),
            "vgpr": meta_get(meta, "amdhsa_next_free_vgpr"),
            "sgpr": meta_get(meta, "amdhsa_next_free_sgpr"),
            "scratch": meta_get(meta, "amdhsa_private_segment_fixed_size"),
            "lds": meta_get(meta, "amdhsa_group_segment_fixed_size"),
        })
    if base:
        gone = set(old) - {r["name"] for r in rows}
        if gone:  # a delta cannot say that a symbol left: write the whole table instead
            sys.exit("not in %s any more: %s" % (path, ", ".join(sorted(gone))))
        keep = [r for r in rows if old.get(r["name"]) != r]
        print(json.dumps({"base": os.path.basename(base), "rows_as_in_base": len(rows) - len(keep)}))
        rows = keep
    for r in rows:
        print(json.dumps(r))


def compare(before, after, families):
    a, b = load(before), load(after)
    bad = 0
    for n in sorted(set(a) ^ set(b)):
        print("only in %s: %s" % (before if n in a else after, n))
        bad += 1
    same = moved = 0
    for n in sorted(set(a) & set(b)):
        ra, rb = a[n], b[n]
        if re.sub(r"<.*", "", n) not in families:
            if ra["digest"] != rb["digest"]:
                print("digest changed outside the families: %s" % n)
                bad += 1
            continue
        same += ra["digest"] == rb["digest"]
        moved += ra["digest"] != rb["digest"]
        for k in ("vgpr", "scratch", "lds"):
            if ra[k] != rb[k] or (k == "scratch" and rb[k] != 0):
                print("%s %s -> %s: %s" % (k, ra[k], rb[k], n))
                bad += 1
    print("%d functions; in the families %d with the same digest, %d with another; %d failures" % (
        len(b), same, moved, bad))
    return 1 if bad else 0


def main():
    if sys.argv[1] == "--jsonl":
        return jsonl(*sys.argv[2:4])
    if sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3], set(sys.argv[4:]))
    path, pats = sys.argv[1], sys.argv[2:]
    for n, d, body, meta in functions(open(path).read()):
        if pats and not all(p in d for p in pats):
            continue
        lines = body.splitlines()
        get = lambda k: (lambda v: "?" if v is None else v)(meta_get(meta, k))
        gl = [l.strip() for l in lines if "global_load" in l or "buffer_load" in l]
        print(d)
        print("  vgpr(next_free)=%s sgpr=%s scratch=%s  global/buffer loads=%d  s_load=%d  waitcnt=%d" % (
            get("amdhsa_next_free_vgpr"), get("amdhsa_next_free_sgpr"),
            get("amdhsa_private_segment_fixed_size"), len(gl),
            sum("s_load" in l for l in lines), sum("s_waitcnt" in l for l in lines)))
        for l in gl[:3]:
            print("   ", l)


if __name__ == "__main__":
    sys.exit(main())
