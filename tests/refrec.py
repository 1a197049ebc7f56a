"""The reference's command-line runs the tests compare against, recorded.  Test-only.

oracle/_ref/ (ref_harness, compress_seq, primer_match) is compiled only where the reference sources lie, so a test
that ran those binaries itself could not run from a clean checkout.  run() takes a tool name, its arguments and the
bytes of its input files, and returns what the tool printed and wrote.  Every run is recorded in
tests/golden/ref_runs.json.gz (data only: exit status, stdout, the files written), keyed by a hash of the tool, its
arguments and its inputs:

  * the binary is built and the run is recorded: the tool runs and must give the recorded result (a stale recording fails);
  * the binary is not built: the recording is the result;
  * the run was never recorded: the test fails.  Record after `make -C oracle ref` with
        PM_REF_RECORD=1 python -m pytest tests/test_oracle_vs_ref.py tests/test_compress_seq.py tests/test_seq_io_formats.py
    (it adds the runs it meets to the recording and keeps the others)."""
import atexit
import base64
import gzip
import hashlib
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
STORE = os.path.join(ROOT, "tests", "golden", "ref_runs.json.gz")
RECORD = os.environ.get("PM_REF_RECORD", "") == "1"

_runs = None
_new = {}


def _load():
    global _runs
    if _runs is None:
        _runs = {}
        if os.path.exists(STORE):
            with gzip.open(STORE, "rt") as f:
                _runs = json.load(f)
    return _runs


def _save():
    if not _new:
        return
    runs = dict(_load())
    runs.update(_new)
    with open(STORE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps(runs, sort_keys=True, separators=(",", ":")).encode())


if RECORD:
    atexit.register(_save)


def built(tool):
    return os.path.exists(os.path.join(REF, tool))


def key(tool, args, inputs):
    h = hashlib.sha256(json.dumps([tool, list(args)]).encode())
    for name in sorted(inputs):
        h.update(name.encode() + b"\0" + hashlib.sha256(bytes(inputs[name])).digest())
    return h.hexdigest()[:40]


def _enc(rc, out, files):
    return {"rc": rc, "out": base64.b64encode(out).decode(), "files": {n: base64.b64encode(b).decode() for n, b in sorted(files.items())}}


def _dec(e):
    return e["rc"], base64.b64decode(e["out"]), {n: base64.b64decode(b) for n, b in e["files"].items()}


def run(tool, args, inputs, collect=(), timeout=600):
    """oracle/_ref/<tool> with `args` ("{d}" stands for the directory of the run) in a fresh directory that holds `inputs`
    ({file name: bytes}).  Returns (exit status, stdout bytes, {name: bytes} of the names in `collect` the run left there).
    A path instead of a name runs that binary unrecorded (the fuzzers in scripts/, the golden makers)."""
    if os.sep in tool:
        return _live(tool, args, inputs, collect, timeout)
    k = key(tool, args, inputs)
    rec = _load().get(k)
    if not built(tool):
        assert rec is not None, ("no recorded run of the reference's %s %s in %s (record it where oracle/_ref is built: "
                                 "PM_REF_RECORD=1, tests/refrec.py)" % (tool, " ".join(args)[:200], os.path.relpath(STORE, ROOT)))
        return _dec(rec)
    status, out, files = _live(os.path.join(REF, tool), args, inputs, collect, timeout)
    got = _enc(status, out, files)
    if rec is None:
        assert RECORD, "the reference's %s %s is not recorded in %s: record it with PM_REF_RECORD=1 (tests/refrec.py)" % (
            tool, " ".join(args)[:200], os.path.relpath(STORE, ROOT))
        _new[k] = got
    else:
        assert got == rec, "the reference's %s %s no longer gives the recorded result (%s)" % (tool, " ".join(args)[:200], os.path.relpath(STORE, ROOT))
    return status, out, files


def _live(exe, args, inputs, collect, timeout):
    with tempfile.TemporaryDirectory() as d:
        for name, data in inputs.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(bytes(data))
        r = subprocess.run([exe] + [a.replace("{d}", d) for a in args], capture_output=True, timeout=timeout)
        files = {}
        for name in collect:
            if os.path.exists(os.path.join(d, name)):
                with open(os.path.join(d, name), "rb") as f:
                    files[name] = f.read()
    return r.returncode, r.stdout, files


def hits(out):
    """ref_harness output -> sorted list of (end, id, value)"""
    return sorted(tuple(int(x) for x in line.split()) for line in out.decode().splitlines() if line and not line.startswith("#"))
