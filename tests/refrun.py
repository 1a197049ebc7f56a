"""Run oracle/_ref/ref_harness (the real reference engines) on in-memory inputs, or replay the recorded run
(tests/refrec.py).  Test-only."""
import refrec


def run_ref(harness, raw_or_codes, patterns, table=None, sel=0, k=0, indels=True, rc=False, minka=1000):
    """Returns the reference engine's hits as a sorted list of (end, id, value).  `harness` is the tool's name in
    oracle/_ref (the ref_harness fixture)."""
    if table is None:
        inputs = {"db": bytes(raw_or_codes)}
    else:
        inputs = {"db.sqn": bytes(raw_or_codes), "db.tbl": bytes(table)}
    inputs["pat.txt"] = ("\n".join(patterns) + "\n").encode()
    cmd = ["-N", str(sel), "-m", str(minka), "-i", "{d}/db", "-P", "{d}/pat.txt"]
    if k:
        cmd += ["-k" if indels else "-K", str(k)]
    if rc:
        cmd += ["-r"]
    if table is not None:
        cmd += ["-n"]
    status, out, _ = refrec.run(harness, cmd, inputs)
    if status != 0:
        raise RuntimeError("ref_harness failed (%d)" % status)
    return refrec.hits(out)
