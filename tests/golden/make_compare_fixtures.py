#!/usr/bin/env python3
"""Extracts the KNOWN ANSWERS of the reference's hamming, prefix and postfix modules -- the assertions of their #[cfg(test)] blocks and doc
examples -- into compare_known_answers.json (beside make_reference_fixtures.py, same rule: only string literals, numbers and the expected
values are extracted, no reference code).

Run once where the reference tree is at hand; the output is committed:
    python tests/golden/make_compare_fixtures.py <reference root>
Every entry: {"metric", "op", "s1", "s2", "pad", "cutoff", "expect", "source"}; s1 / s2 are strings or lists of numbers; expect is the value, null for
None, or "DifferentLengthArgs" for the Err of hamming without pad; "pad" is null where the assertion leaves Args::pad alone (the default: no padding).
"""
import json
import os
import re
import sys

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compare_known_answers.json")

SEQ = r'(?:"([^"]*)"\.chars\(\)|\[([0-9, ]*)\])'


def seq(m_str, m_list):
    return m_str if m_list is None else [int(v) for v in m_list.split(",")]


def expect(text):
    text = text.strip()
    if "DifferentLengthArgs" in text:
        return "DifferentLengthArgs"
    if "None" in text:
        return None
    return int(re.search(r"\d+", text).group(0))


def line_of(txt, pos):
    return txt.count("\n", 0, pos) + 1


def extract(metric):
    name = metric + ".rs"
    txt = open(os.path.join(REF, "src/distance", name)).read()
    out = []

    def add(op, s1, s2, pad, cutoff, exp, pos):
        out.append({"metric": metric, "op": op, "s1": s1, "s2": s2, "pad": pad, "cutoff": cutoff, "expect": exp, "source": f"{name}:{line_of(txt, pos)}"})

    # assert_dist(3, "hamming", "hammers")  (the test module's helper: distance(a.chars(), b.chars()) == Ok(dist))
    for m in re.finditer(r'assert_dist\(\s*(\d+),\s*"([^"]*)",\s*"([^"]*)"\s*\)', txt):
        add("distance", m.group(2), m.group(3), None, None, int(m.group(1)), m.start())
    # assert_eq!(<expected>, [<module>::]<op>(<s1>, <s2>))
    for m in re.finditer(r"assert_eq!\(\s*([^,]+?),\s*(?:\w+::)?(distance|similarity)\(\s*" + SEQ + r",\s*" + SEQ + r"\s*\)\s*,?\s*\)", txt):
        add(m.group(2), seq(m.group(3), m.group(4)), seq(m.group(5), m.group(6)), None, None, expect(m.group(1)), m.start())
    # assert_eq!(<expected>, <op>_with_args(<s1>, <s2>, &Args::default()<builders>))
    for m in re.finditer(r"assert_eq!\(\s*([^,]+?),\s*(distance|similarity)_with_args\(\s*" + SEQ + r",\s*" + SEQ + r",\s*&Args::default\(\)((?:\s*\.\w+\([^)]*\))*)\s*,?\s*\)\s*,?\s*\)", txt):
        builders = dict(re.findall(r"\.(\w+)\(([^)]*)\)", m.group(7)))
        pad = None if "pad" not in builders else builders["pad"].strip() == "true"
        cutoff = int(builders["score_cutoff"]) if "score_cutoff" in builders else None
        add(m.group(2), seq(m.group(3), m.group(4)), seq(m.group(5), m.group(6)), pad, cutoff, expect(m.group(1)), m.start())
    # let scorer = <module>::BatchComparator::new("..".chars()); assert_eq!(<expected>, scorer.<op>("..".chars()));
    for m in re.finditer(r'BatchComparator::new\("([^"]*)"\.chars\(\)\);\s*(?:///\s*)?assert_eq!\(\s*([^,]+?),\s*scorer\.(distance|similarity)\("([^"]*)"\.chars\(\)\)\s*\)', txt):
        add(m.group(3), m.group(1), m.group(4), None, None, expect(m.group(2)), m.start())
    return out


if __name__ == "__main__":
    entries = extract("hamming") + extract("prefix") + extract("postfix")
    json.dump(entries, open(OUT, "w"), ensure_ascii=False, indent=1)
    print(f"wrote {OUT}: {len(entries)} known answers")
