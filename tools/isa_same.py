#!/usr/bin/env python3
"""Are the kernels of two device assembly files the same instruction streams?  (host only; no GPU)

For a change that must not move the code object -- a kernel renamed, its text re-arranged, its argument list extended -- compile the unit
before and after with the Makefile's FLAGS plus `--cuda-device-only -S` and compare:

    isa_same.py old.s new.s [--map names.txt]

names.txt: one `old_symbol new_symbol` pair per line (mangled, as the assembly spells them; `#` starts a comment).  A kernel not in the map is
paired with the kernel of the same name, and its WHOLE text, directives and
comments included, must be identical (white space and the function's number in the unit, which its labels carry, apart).  For a mapped pair the comments
and directives are stripped, local labels (.LBB7_3, .LJTI7_0, ...) are renumbered in order of appearance, and the streams are compared line
by line.  Per pair: instruction counts, code lengths, registers / scratch / occupancy as the compiler's own summary comments give them, and
every differing line, classed as
    kernarg offset only   the same s_load_* into the same destination from the same SGPR pair, another immediate offset, and that pair is
                          one the kernel-argument pointer arrives in or is copied to (what a longer argument list does to every
                          argument behind the new ones)
    other                 anything else
Exit status 1 if any pair has an `other` line, differing counts, code lengths or resource figures, if an unmapped kernel's text differs, or
if a kernel has no partner.  It compares; it does not look for particular instructions.
"""
import argparse
import difflib
import re
import sys

FACTS = ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def kernels(path):
    """{symbol: {"raw": [lines], "facts": {...}, "kernarg": "s[a:b]"}} for every .amdhsa_kernel of the file."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    out = {}
    for name in names:
        start = lines.index(next(ln for ln in lines if ln.startswith(name + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        # the compiler's summary comments follow the function's end, up to the next section
        tail_end = next((i for i in range(end, len(lines)) if re.match(r"\s*\.(text|section\s+\.text)", lines[i])), len(lines))
        facts = {}
        for ln in lines[end:tail_end]:
            m = re.match(r";\s*(\w+)\s*[:=]\s*(\d+)", ln)
            if m and m.group(1) in FACTS:
                facts[m.group(1)] = int(m.group(2))
        # the kernel descriptor says which user SGPRs come before the kernel-argument pointer
        d0 = next(i for i, ln in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+%s\s*$" % re.escape(name), ln))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        desc = dict(m.groups() for m in (re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln) for ln in lines[d0 + 1:d1]) if m)
        base = 4 * int(desc.get("user_sgpr_private_segment_buffer", "0")) + 2 * int(desc.get("user_sgpr_dispatch_ptr", "0")) + \
            2 * int(desc.get("user_sgpr_queue_ptr", "0"))
        out[name] = {"raw": lines[start:tail_end] + lines[d0:d1 + 1], "body": lines[start + 1:end], "facts": facts,
                     "kernarg": "s[%d:%d]" % (base, base + 1)}
    return out


def stream(body):
    """The instructions and labels of a kernel body: no comments, no directives, local labels renumbered by first appearance."""
    seen = {}

    def renumber(m):
        return seen.setdefault(m.group(0), "%s#%d" % (m.group(1), len(seen)))

    out = []
    for ln in body:
        ln = ln.split(";", 1)[0].strip()
        if not ln or (ln.startswith(".") and not ln.endswith(":")):
            continue
        out.append(re.sub(r"(\.L[A-Za-z_]+?)\d+(?:_\d+)?\b", renumber, re.sub(r"\s+", " ", ln)))
    return out


def kernarg_pairs(code, pair):
    """The SGPR pairs that may hold the kernel-argument pointer somewhere in the kernel: the pair it arrives in, and every pair that gets it
    through s_mov_b64 / s_mov_b32 or through a v_writelane_b32 / v_readlane_b32 round trip (the compiler parks it in a VGPR's lanes when
    scalar registers run short).  Flow-insensitive, i.e. an over-estimate: it only says which loads MAY be argument loads."""
    lo, hi = (int(x) for x in re.match(r"s\[(\d+):(\d+)\]", pair).groups())
    tag, lanes = {lo: 0, hi: 1}, {}                              # register / (vgpr, lane) -> half of the pointer
    while True:
        before = (len(tag), len(lanes))
        for ln in code:
            m = re.match(r"s_mov_b64 s\[(\d+):\d+\], s\[(\d+):\d+\]$", ln)
            if m and tag.get(int(m.group(2))) == 0 and tag.get(int(m.group(2)) + 1) == 1:
                tag.setdefault(int(m.group(1)), 0), tag.setdefault(int(m.group(1)) + 1, 1)
            m = re.match(r"s_mov_b32 s(\d+), s(\d+)$", ln)
            if m and int(m.group(2)) in tag:
                tag.setdefault(int(m.group(1)), tag[int(m.group(2))])
            m = re.match(r"v_writelane_b32 (v\d+), s(\d+), (\d+)$", ln)
            if m and int(m.group(2)) in tag:
                lanes.setdefault((m.group(1), m.group(3)), tag[int(m.group(2))])
            m = re.match(r"v_readlane_b32 s(\d+), (v\d+), (\d+)$", ln)
            if m and (m.group(2), m.group(3)) in lanes:
                tag.setdefault(int(m.group(1)), lanes[(m.group(2), m.group(3))])
        if before == (len(tag), len(lanes)):
            return {"s[%d:%d]" % (r, r + 1) for r in tag if tag[r] == 0 and tag.get(r + 1) == 1}


def kernarg_offset_only(a, b, pairs):
    pat = r"(s_load_\w+) (\S+), (s\[\d+:\d+\]), (\S+)$"
    ma, mb = re.match(pat, a), re.match(pat, b)
    return bool(ma and mb and ma.group(1, 2, 3) == mb.group(1, 2, 3) and ma.group(3) in pairs and ma.group(4) != mb.group(4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", help="file of `old_symbol new_symbol` lines")
    args = ap.parse_args()
    names = {}
    if args.map:
        for ln in open(args.map):
            ln = ln.split("#", 1)[0].split()
            if len(ln) == 2:
                names[ln[0]] = ln[1]
    old, new = kernels(args.old), kernels(args.new)
    bad = 0
    for o in names:                                              # (a map may cover several units: a pair neither file has is not this run's)
        if o not in old and names[o] in new:
            print("MISSING in %s: %s" % (args.old, o))
            bad += 1
    for n in sorted(set(new) - {names.get(o, o) for o in old}):
        print("NO PARTNER for new kernel %s" % n)
        bad += 1
    for o in sorted(old):
        n = names.get(o, o)
        if n not in new:
            print("NO PARTNER for old kernel %s (wanted %s)" % (o, n))
            bad += 1
            continue
        if o not in names:
            # (only the function's number in the unit, which its local labels carry, may differ)
            def fn_free(raw): return [re.sub(r"\s+", " ", re.sub(r"(\.L[A-Za-z_]+?|BB)\d+(_\d+)?\b", r"\1\2", ln)) for ln in raw]
            same = fn_free(old[o]["raw"]) == fn_free(new[n]["raw"])
            print("%s: %s" % (o, "identical text" if same else "TEXT DIFFERS (not in the map)"))
            bad += not same
            continue
        so, sn = stream(old[o]["body"]), stream(new[n]["body"])
        io, i_n = sum(not x.endswith(":") for x in so), sum(not x.endswith(":") for x in sn)
        print("%s\n  -> %s" % (o, n))
        print("  instructions %d / %d   %s" % (io, i_n, "   ".join("%s %s / %s" % (k, old[o]["facts"].get(k), new[n]["facts"].get(k)) for k in FACTS)))
        pair_bad = io != i_n or old[o]["facts"] != new[n]["facts"] or old[o]["kernarg"] != new[n]["kernarg"]
        if len(so) == len(sn):
            diffs = [(a, b) for a, b in zip(so, sn) if a != b]
        else:
            sm = difflib.SequenceMatcher(None, so, sn, autojunk=False)
            diffs = [("\n".join(so[i1:i2]), "\n".join(sn[j1:j2])) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal"]
        pairs = kernarg_pairs(so, old[o]["kernarg"]) & kernarg_pairs(sn, new[n]["kernarg"])
        n_karg = 0
        for a, b in diffs:
            if kernarg_offset_only(a, b, pairs):
                n_karg += 1
                print("    kernarg offset only: %-44s | %s" % (a, b))
            else:
                pair_bad = True
                print("    OTHER:               %-44s | %s" % (a, b))
        print("  %d differing lines: %d kernarg offset only, %d other -> %s" % (len(diffs), n_karg, len(diffs) - n_karg, "DIFFERENT" if pair_bad else "same"))
        bad += pair_bad
    print("%d kernels compared, %d not the same" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
