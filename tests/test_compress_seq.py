"""pm_compress_seq (host C++) against the files the reference's compress_seq wrote for the same
FASTA input (tests/golden/cli_*.json, made by tests/golden/make_cli_golden.py), byte for byte;
and against the reference binary (oracle/_ref where it is built, its recorded runs where it is not:
tests/refrec.py) on FASTA files with awkward layouts (CR LF, blank lines, lower case, no final
newline, control characters), incl. the bit-packed form (-z true: <db>.sqz + <db>.tbz, compress_seq.cc:741-905)."""
import base64
import json
import os
import subprocess
import tempfile

import pytest

import refrec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "sequence-alignment-tools_amd", "host", "pm_compress_seq")
EXTS = ("seq", "sqn", "tbl", "sqz", "tbz", "hdr", "idb")


def files_of(fa):
    out = {}
    for ext in EXTS:
        if os.path.exists(fa + "." + ext):
            with open(fa + "." + ext, "rb") as f:
                out[ext] = f.read()
    return out


@pytest.mark.parametrize("fixture", ["cli_a", "cli_b"])
@pytest.mark.parametrize("variant,args", [("normalized", ["-n", "true"]), ("indexed", []), ("compressed", ["-z", "true"])])
def test_against_golden_files(fixture, variant, args):
    assert os.path.exists(CS), "run __graft_entry__.build()"
    with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
        g = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "db.fa")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
        assert r.returncode == 0, r.stderr
        got = files_of(fa)
    want = {k: base64.b64decode(v) for k, v in g["db_files"][variant].items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (fixture, variant, k)


AWKWARD = [
    b">a first\nACGTACGT\nacgtnn\n>b\r\nAC GT\tAC\r\nGG\r\n\n>c empty follows\n>d\nAC\x01G*T-\n>e last without newline\nACGTN",
    b"junk before the first header\n>only one\nACGT\n",
    b">ends inside a header",
    b">x\nACGT\n>y\n",
    b"",                                                  # no bytes at all: the reference writes no files (scripts/fuzz_compress.py seed 31)
    b"\n",
]


def ref_compress_seq(fasta, args):
    """the reference's compress_seq on `fasta` (bytes): (exit status, {extension: bytes} of the files it wrote)"""
    status, _, files = refrec.run("compress_seq", ["-i", "{d}/db.fa"] + args, {"db.fa": fasta}, collect=["db.fa." + e for e in EXTS])
    return status, {n[len("db.fa."):]: b for n, b in files.items()}


@pytest.mark.parametrize("idx", range(len(AWKWARD)))
@pytest.mark.parametrize("args", [[], ["-n", "true"], ["-n", "true", "-u", "false"], ["-S", "false"], ["-e", "false", "-S", "false"],
                                  ["-E", "36", "-n", "true"], ["-n", "true", "-D", "false"], ["-n", "true", "-C", "false"],
                                  ["-z", "true"], ["-z", "true", "-n", "true", "-C", "false"], ["-z", "true", "-D", "false", "-u", "false"],
                                  ["-z", "true", "-E", "36"]])
def test_against_reference_binary(idx, args):
    res = [ref_compress_seq(AWKWARD[idx], args)]
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "db.fa")
        with open(fa, "wb") as f:
            f.write(AWKWARD[idx])
        r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
        res.append((r.returncode, files_of(fa)))
    if res[0][0] != 0:
        pytest.skip("reference refuses this input")
    assert res[1][0] == 0
    assert sorted(res[0][1]) == sorted(res[1][1]), (idx, args)
    for k in res[0][1]:
        assert res[0][1][k] == res[1][1][k], (idx, args, k)


@pytest.mark.parametrize("nsym", [2, 3, 5, 9, 17, 40])
def test_compressed_form_at_every_code_width(nsym):
    """.sqz packs ceil(log2(table size)) bits per character, most significant bit first, and fills the last
    buffer of lcm(bits, 8) bytes with end-of-sequence codes: alphabets of 2 .. 40 symbols (1 .. 6 bits), lengths
    around the buffer size."""
    import random
    rnd = random.Random(nsym)
    alphabet = "ACGTNRYKMSWBDHVXUQEFILPZJO0123456789abcd"[:nsym - 1]          # + the end-of-sequence character
    for length in (1, 7, 8, 23, 24, 25, 119, 120, 121, 1000):
        fasta = ">a\n" + "".join(rnd.choice(alphabet) for _ in range(length)) + "\n>b\n" + "".join(rnd.choice(alphabet) for _ in range(5)) + "\n"
        args = ["-z", "true", "-u", "false", "-D", "false"]
        status, ref = ref_compress_seq(fasta.encode(), args)
        assert status == 0, ("reference", nsym, length)
        res = [ref]
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "db.fa")
            with open(fa, "w") as f:
                f.write(fasta)
            r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
            assert r.returncode == 0, (CS, r.stderr)
            res.append(files_of(fa))
        assert sorted(res[0]) == sorted(res[1]) and "sqz" in res[0]
        for k in res[0]:
            assert res[0][k] == res[1][k], (nsym, length, k)
