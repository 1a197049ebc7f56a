"""CPU: the four database forms the command lines read (select.t:22-188) through host/seq_io.cc, without a GPU:
<db>.seq, <db>.sqn + .tbl, <db>.sqz + .tbz (written here by pm_compress_seq and, where present, by the reference's
compress_seq) and the FASTA file itself.  The streams must be the same characters position by position (the
compressed form may add end-of-sequence characters at the end, char_io.t:18-214), the entries must start at the same
positions with the same headers.  The reference's files come from its recorded runs where oracle/_ref is not built
(tests/refrec.py)."""
import os
import subprocess
import tempfile

import pytest

import refrec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
DUMP = os.path.join(HOST, "pm_seqdb_dump")
CS = os.path.join(HOST, "pm_compress_seq")
REF_CS = os.path.join(ROOT, "oracle", "_ref", "compress_seq")

FASTA = (">one first entry\n" + "ACGTTGCAAGCTTAGGCTCANNACGT\n" * 3 + "ACG\n" +
         ">two\tsecond\n" + "GATTACAGGCTTAACCGTGTCAATAC\n" * 2 +
         ">three\n" + "TTGACC\n")


def dump(db, fmt, uc=0):
    r = subprocess.run([DUMP, db, str(fmt), str(uc)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {"entries": []}
    for line in r.stdout.splitlines():
        k, _, v = line.partition(" ")
        if k == "entry":
            out["entries"].append(v)
        elif k == "entries":
            out["count"] = int(v)
        else:
            out[k] = v
    table = bytes.fromhex(out["table"])
    raw = bytes.fromhex(out["stream"])
    out["chars"] = bytes(table[c] for c in raw) if out["normalized"] == "1" else raw
    return out


EXTS = ("seq", "sqn", "tbl", "sqz", "tbz", "hdr", "idb")


@pytest.mark.parametrize("writer", [CS, REF_CS])
def test_all_forms_give_one_stream(writer):
    assert os.path.exists(DUMP) and os.path.exists(CS), "run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as d:
        forms = {}
        for name, args, fmt in (("indexed", [], 2), ("normalized", ["-n", "true"], 3), ("compressed", ["-z", "true"], 4), ("raw", None, 1)):
            os.mkdir(os.path.join(d, name))
            fa = os.path.join(d, name, "db.fa")
            with open(fa, "w") as f:
                f.write(FASTA)
            if args is not None and writer == REF_CS:
                status, _, files = refrec.run("compress_seq", ["-i", "{d}/db.fa"] + args, {"db.fa": FASTA.encode()},
                                              collect=["db.fa." + e for e in EXTS])
                assert status == 0 and files, name
                for n, b in files.items():
                    with open(os.path.join(d, name, n), "wb") as f:
                        f.write(b)
            elif args is not None:
                r = subprocess.run([writer, "-i", fa] + args, capture_output=True)
                assert r.returncode == 0, r.stderr
            forms[name] = dump(fa, fmt)
            assert dump(fa, 0)["chars"] == forms[name]["chars"], name            # the automatic choice finds the same files
        ref = forms["indexed"]
        assert ref["chars"].startswith(b"\n") and ref["chars"].endswith(b"\n") and ref["chars"].count(b"\n") == 4
        assert len(ref["entries"]) == 3 and "[one first entry|one]" in ref["entries"][0] and "[two\tsecond|two]" in ref["entries"][1]
        for name in ("normalized", "raw"):
            assert forms[name]["chars"] == ref["chars"], name
            assert forms[name]["entries"] == ref["entries"], name
        z = forms["compressed"]
        assert z["chars"].startswith(ref["chars"]) and set(z["chars"][len(ref["chars"]):]) <= {ord("\n")}
        assert len(z["chars"]) - len(ref["chars"]) < 64                        # 3-bit codes: buffers of 24 bytes = 64 characters
        assert z["entries"][:3] == ref["entries"]


def test_raw_fasta_case_and_line_ends():
    """lower case stays unless upper_case is asked for (ffp.upper_case = primer_match -u); CR LF line ends and a last
    line without a newline read like the plain file"""
    with tempfile.TemporaryDirectory() as d:
        plain = os.path.join(d, "plain.fa")
        with open(plain, "w") as f:
            f.write(FASTA)
        want = dump(plain, 1)
        crlf = os.path.join(d, "crlf.fa")
        with open(crlf, "wb") as f:
            f.write(FASTA.replace("\n", "\r\n").encode())
        assert dump(crlf, 1)["chars"] == want["chars"] and dump(crlf, 1)["entries"] == want["entries"]
        cut = os.path.join(d, "cut.fa")
        with open(cut, "w") as f:
            f.write(FASTA[:-1])
        assert dump(cut, 1)["chars"] == want["chars"]
        low = os.path.join(d, "low.fa")
        with open(low, "w") as f:
            f.write("".join(l if l.startswith(">") else l.lower() for l in FASTA.splitlines(True)))
        assert dump(low, 1)["chars"] == want["chars"].lower()
        assert dump(low, 1, uc=1)["chars"] == want["chars"]
