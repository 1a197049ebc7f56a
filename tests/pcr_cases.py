"""What the pm_pcr_* tests share: the goldens of tests/golden/pcr_*.json as inputs of the pairing rule (stream, primer
patterns in pcr_match's numbering, options, entry starts) and the recorded one-line output parsed into numbers."""
import json
import os
import re

import numpy as np

import pcr_rule as R
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cases whose -A is the one-line format ONE of tests/golden/make_pcr_golden.py
ONELINE = ["sts_K1_oneline", "sts_k2_oneline", "pairs_r_k1", "pairs_r_k1_allorient", "pairs_r_k1_between"]
LINE = re.compile(r"^(\d+) \S+(?: REVERSE-STRAND)? \[([^\]]*)\] \[([^\]]*)\] (-?\d+) (-?\d+) (-?\d+) (\d+) ")


def load(fixture):
    with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
        return json.load(f)


def entries_of(fasta):
    ents = []
    for line in fasta.splitlines():
        if line.startswith(">"):
            ents.append([])
        elif ents:
            ents[-1].append(line.strip())
    return ["".join(e) for e in ents]


def setup(g, case):
    """dict: rule (pcr_rule.Rule), patterns (ids 1..2n in order), k, indels, codes, table, chars (the decoded stream),
    entry_starts, want (the recorded lines as tuples, sorted)"""
    c = g["cases"][case]
    opts = list(c["options"])
    o = dict(k=0, indels=True, a=False, b=False, m=0, M=2000, d=-1)
    i = 0
    while i < len(opts):
        f = opts[i]
        if f in ("-k", "-K"):
            o["k"], o["indels"] = int(opts[i + 1]), f == "-k"
            i += 2
        elif f in ("-m", "-M", "-d"):
            o[f[1]] = int(opts[i + 1])
            i += 2
        elif f in ("-A", "-R"):
            i += 2
        elif f in ("-a", "-b", "-r"):
            if f != "-r":
                o[f[1]] = True
            i += 1
        else:
            raise ValueError(f)
    prim, sizes = [], None
    if c["primers"] == "S":
        sizes = []
        for line in g["primers"]["S"].splitlines():
            t = line.split()
            prim += [t[1], t[2]]
            sz = t[3].split("-")
            sizes.append((int(sz[0]), int(sz[-1])))
    else:
        prim = g["primers"][c["primers"]].split()
    prim = [p if i % 2 == 0 else synth.revcomp(p) for i, p in enumerate(prim)]      # -S and -r (pcr_match.cc:776-790)
    n = len(prim)
    patterns = prim + [synth.revcomp(p) for p in prim]
    ents = entries_of(g["fasta"])
    table = synth.table_for(ents)
    raw = synth.stream(ents)
    starts, at = [], 1
    for e in ents:
        starts.append(at)
        at += len(e) + 1
    rule = R.Rule(n, [0] + [len(p) for p in patterns], o["k"], o["indels"], o["a"], o["b"], o["m"], o["M"], o["d"], sizes)
    want = []
    for line in c["stdout"].splitlines():
        m = LINE.match(line)
        assert m, line
        a, b = m.group(2).split(" "), m.group(3).split(" ")
        # %i, %>S %>E %<S %<E, %>d %<d, %l, %N
        want.append((int(m.group(1)), int(a[2]), int(a[3]), int(b[2]), int(b[3]), int(a[4]), int(b[4]), int(m.group(4)), int(m.group(7))))
    return dict(rule=rule, patterns=patterns, k=o["k"], indels=o["indels"], codes=synth.normalize(raw, table), table=table, chars=raw,
                entry_starts=starts, want=sorted(want), n_stream=len(raw))


def line_of(s):
    """a survivor of pcr_rule.round_survivors (or the same fields from the library) as the tuple of `want`"""
    hit, hit1, al, al1, alen, pi, nc = s
    return (pi, al[0], al[1], al1[0], al1[1], al[2], al1[2], al1[1] - al[0], nc)


def rounds(hits, n_stream, step):
    """The rounds of the host loop when find_patterns scans `step` positions per range and returns after the first range
    with hits: yields (new hits, scanned_to, more)."""
    pos = 0
    hits = sorted(hits)
    while True:
        new = []
        while pos < n_stream and not new:
            end = min(n_stream, pos + step)
            new = [h for h in hits if pos < h[0] <= end]
            pos = end
        yield new, pos, bool(new)
        if not new:
            return


def run_rounds(rule, hits, n_stream, step, align, entry_starts, chars):
    """all survivors of the rule applied round by round, and the rounds as (new, scanned_to, more)"""
    held, out, log = [], [], []
    for new, scanned_to, more in rounds(hits, n_stream, step):
        if not more and not held:
            break
        held = held + new
        log.append((new, scanned_to, more))
        sv, _, held = R.round_survivors(rule, held, scanned_to, more, align, entry_starts, chars)
        out += sv
    return out, log
