"""The bit-packed stream form on the host (no GPU): pm_pack_codes / pm_unpack_codes against numpy's packbits / unpackbits
(both most significant bit first, like <db>.sqz: char_io.t:18-214), against the .sqz files pm_compress_seq and the
reference's compress_seq wrote, and the argument checks of pm_init_packed."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import refrec
import sat_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
CS = os.path.join(HOST, "pm_compress_seq")
DUMP = os.path.join(HOST, "pm_seqdb_dump")
LENGTHS = (0, 1, 7, 8, 15, 16, 17, 63, 64, 65, 1000, 100003)
PM_E_INVALID, PM_E_HIP = -1, -4
EXTS = ("seq", "sqn", "tbl", "sqz", "tbz", "hdr", "idb")      # the files a recorded compress_seq run keeps (tests/refrec.py)


def np_pack(codes, bits):
    """codes -> packed bytes: the low `bits` bits of every code, most significant first, zero fill at the end"""
    return np.packbits(np.unpackbits(np.asarray(codes, dtype=np.uint8)[:, None], axis=1)[:, 8 - bits:].reshape(-1))


def np_unpack(packed, bits, first, n):
    b = np.unpackbits(np.asarray(packed, dtype=np.uint8))[first * bits:(first + n) * bits].reshape(n, bits)
    return np.packbits(np.concatenate([np.zeros((n, 8 - bits), dtype=np.uint8), b], axis=1), axis=1).reshape(-1)


@pytest.mark.parametrize("bits", range(1, 9))
def test_pack_and_unpack_against_numpy(bits):
    rng = np.random.default_rng(bits)
    for n in LENGTHS:
        codes = rng.integers(0, 1 << bits, n, dtype=np.uint8)
        want = np_pack(codes, bits)
        got = sat_amd.pack_codes(codes, bits)
        assert got.size == (n * bits + 7) // 8 and (got == want).all(), (bits, n)
        firsts = {0, 64, 128, 128 * 3, 128 * 700, 1, 3, 7, 9, 63, 65, 1001, n - 1, n}
        for first in sorted(f for f in firsts if 0 <= f <= n):
            out = sat_amd.unpack_codes(got, bits, first, n - first)
            assert (out == codes[first:]).all(), (bits, n, first)
            if n - first > 5:                                         # a run that ends inside a byte
                out = sat_amd.unpack_codes(got, bits, first, n - first - 3)
                assert (out == np_unpack(got, bits, first, n - first - 3)).all(), (bits, n, first)


def test_pack_and_unpack_refuse_bad_arguments():
    codes = np.arange(8, dtype=np.uint8)
    for bits in (0, 9, -1):
        with pytest.raises(sat_amd.PmError):
            sat_amd.pack_codes(codes, bits)
        with pytest.raises(sat_amd.PmError):
            sat_amd.unpack_codes(codes, bits, 0, 1)
    with pytest.raises(sat_amd.PmError):
        sat_amd.pack_codes(codes, 2)                                  # 7 does not fit two bits
    packed = sat_amd.pack_codes(codes, 3)                             # 3 bytes = 8 codes
    with pytest.raises(sat_amd.PmError):
        sat_amd.unpack_codes(packed, 3, 0, 9)
    with pytest.raises(sat_amd.PmError):
        sat_amd.unpack_codes(packed, 3, 8, 1)
    with pytest.raises(sat_amd.PmError):
        sat_amd.unpack_codes(packed, 3, -1, 1)
    assert sat_amd.unpack_codes(packed, 3, 8, 0).size == 0
    L = sat_amd.load_library()
    out = np.zeros(2, dtype=np.uint8)                                 # an output buffer that is too small
    assert L.pm_pack_codes(codes.ctypes.data_as(C.c_void_p), 8, 3, out.ctypes.data_as(C.c_void_p), 2) == PM_E_INVALID


def dump(db, fmt):
    r = subprocess.run([DUMP, db, str(fmt), "0"], capture_output=True)
    assert r.returncode == 0, r.stderr
    f = dict(line.split(" ", 1) for line in r.stdout.decode().splitlines() if " " in line and not line.startswith("entry "))
    return bytes.fromhex(f["table"]), np.frombuffer(bytes.fromhex(f["stream"]), dtype=np.uint8)


@pytest.mark.parametrize("nsym", [2, 3, 5, 9, 17, 40])
def test_sqz_files_at_every_code_width(nsym):
    """alphabets of 2 .. 40 symbols (1 .. 6 bits per code; the FASTA files of test_compress_seq.py's
    test_compressed_form_at_every_code_width): unpack_codes of <db>.sqz is the stream SeqDb hands out, and pack_codes of
    that stream is the file -- ours and the one the reference's compress_seq wrote."""
    rnd = random.Random(nsym)
    alphabet = "ACGTNRYKMSWBDHVXUQEFILPZJO0123456789abcd"[:nsym - 1]          # + the end-of-sequence character
    for length in (1, 7, 8, 23, 24, 25, 119, 120, 121, 1000):
        fasta = ">a\n" + "".join(rnd.choice(alphabet) for _ in range(length)) + "\n>b\n" + "".join(rnd.choice(alphabet) for _ in range(5)) + "\n"
        args = ["-z", "true", "-u", "false", "-D", "false"]
        status, _, ref = refrec.run("compress_seq", ["-i", "{d}/db.fa"] + args, {"db.fa": fasta.encode()}, collect=["db.fa." + e for e in EXTS])
        assert status == 0 and "db.fa.sqz" in ref, ("reference", nsym, length)
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "db.fa")
            with open(fa, "w") as f:
                f.write(fasta)
            r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
            assert r.returncode == 0, (CS, r.stderr)
            with open(fa + ".sqz", "rb") as f:
                sqz = np.frombuffer(f.read(), dtype=np.uint8)
            with open(fa + ".tbz", "rb") as f:
                tbz = f.read()
            table, stream = dump(fa, 4)
        assert table == tbz == ref["db.fa.tbz"] and len(tbz) <= nsym
        bits = max(1, (len(tbz) - 1).bit_length())
        n = sqz.size * 8 // bits
        assert stream.size == n and n >= length + 8
        for packed in (sqz, np.frombuffer(ref["db.fa.sqz"], dtype=np.uint8)):
            assert packed.size == sqz.size
            assert (sat_amd.unpack_codes(packed, bits, 0, n) == stream).all(), (nsym, length)
            assert (sat_amd.pack_codes(stream, bits) == packed).all(), (nsym, length)
        text = bytes(tbz[c] for c in stream).decode("latin1")                # the characters, with the reference's fill at the end
        assert text.startswith("\n" + fasta.split("\n")[1] + "\n" + fasta.split("\n")[3] + "\n"), (nsym, length)


def handle():
    pm = sat_amd.PatternMatch(k=0)
    pm.add_pattern("ACGTACGTACGT", 1)
    return pm


def test_init_packed_checks_its_arguments_before_the_gpu():
    """each of the documented checks is PM_E_INVALID -- also on a machine without a GPU, so before any HIP call"""
    L = sat_amd.load_library()
    codes = np.array([0, 1, 2, 3] * 16, dtype=np.uint8)
    packed = sat_amd.pack_codes(codes, 3)                             # 24 bytes = 64 codes
    table = (C.c_uint8 * 6).from_buffer_copy(b"ACGT\nN")
    big = (C.c_uint8 * 9).from_buffer_copy(b"ACGT\nNRYK")
    p = packed.ctypes.data_as(C.c_void_p)
    bad = {
        "bits 0": (p, 24, 0, 64, table, 6, 0), "bits 9": (p, 24, 9, 2, table, 6, 0), "bits -3": (p, 24, -3, 2, table, 6, 0),
        "n * bits > 8 * packed_bytes": (p, 24, 3, 65, table, 6, 0), "the same, one byte short": (p, 23, 3, 64, table, 6, 0),
        "no table": (p, 24, 3, 64, None, 0, 0), "table without a length": (p, 24, 3, 64, table, 0, 0),
        "table_len > 2^bits": (p, 24, 3, 64, big, 9, 0), "table_len > 2^bits (2 bits)": (p, 24, 2, 64, table, 5, 0),
        "negative n": (p, 24, 3, -1, table, 6, 0), "negative packed_bytes": (p, -24, 3, 0, table, 6, 0),
        "negative window": (p, 24, 3, 64, table, 6, -4096), "no packed bytes": (None, 24, 3, 64, table, 6, 0),
    }
    for what, a in bad.items():
        for window in ((a[6],) if a[6] else (0, 4096)):
            pm = handle()
            rc = L.pm_init_packed(pm._h, a[0], a[1], a[2], a[3], a[4], a[5], window)
            assert rc == PM_E_INVALID, (what, window, rc)
            assert L.pm_last_error(pm._h), what
            pm.close()
    pm = handle()
    with pytest.raises(sat_amd.PmError) as e:
        pm.init_packed(packed, 3, 65, b"ACGT\nN")
    assert e.value.code == PM_E_INVALID
    pm.close()


@pytest.mark.parametrize("window", [None, 4096])
def test_init_packed_without_a_gpu_fails_loudly(window):
    """no CPU fallback: a valid pm_init_packed without a device is PM_E_HIP, as pm_init (test_abi.py)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    pm = handle()
    codes = np.array([0, 1, 2, 3] * 16, dtype=np.uint8)
    with pytest.raises(sat_amd.PmError) as e:
        pm.init_packed(sat_amd.pack_codes(codes, 3), 3, codes.size, b"ACGT\nN", window=window)
    assert e.value.code == PM_E_HIP
    pm.close()
