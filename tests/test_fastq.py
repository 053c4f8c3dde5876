"""FASTQ input, the host side (no GPU): the new C-ABI calls are declared and exported, the record
frontier (fk_fastq_frontier) on hand-made buffers, the FASTQ file split (fk_split_bytes_fastq), and the
CLI's format variable.

A record starts at a line beginning with '@' whose second-next line begins with '+'.  The reference
here is a Python scan of the whole buffer written from that sentence.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk

NEW = ["fk_set_input_format", "fk_input_format", "fk_fastq_info", "fk_fastq_frontier", "fk_split_bytes_fastq"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def test_the_new_calls_are_declared_exported_and_bound():
    assert set(NEW) <= set(fk.header_functions())
    out = subprocess.check_output(["nm", "-D", "--defined-only", fk.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported
    L = fk.lib()
    with open(fk.HEADER_PATH) as f:
        text = f.read()
    assert "#define FK_FORMAT_FASTA 0" in text and "#define FK_FORMAT_FASTQ 1" in text
    assert "#define FK_ABI_VERSION 3" in text and L.fk_abi_version() == 3
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        args = re.search(r"\b%s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(getattr(L, name).argtypes) == len(args.split(",")), name
    assert fk.FORMATS == {"fasta": 0, "fastq": 1}


def test_null_arguments_are_invalid():
    L = fk.lib()
    off = ctypes.c_size_t(7)
    out = (ctypes.c_uint64 * 3)(7, 7, 7)
    assert L.fk_set_input_format(None, 1, 0, 33) == -1
    assert L.fk_input_format(None, None, None, None) == -1
    assert L.fk_fastq_info(None, out) == -1
    assert L.fk_fastq_frontier(None, 4, ctypes.byref(off)) == -1
    assert L.fk_fastq_frontier(b"@a\n", 3, None) == -1
    assert L.fk_split_bytes_fastq(None, 1, 0, None, 0, ctypes.byref(off)) == -1
    assert off.value == 7 and list(out) == [7, 7, 7]


# ---- the frontier

def line_starts(buf: bytes) -> list[int]:
    return [0] * (len(buf) > 0) + [i + 1 for i, c in enumerate(buf) if c == 0x0A and i + 1 < len(buf)]


def record_starts(buf: bytes) -> list[int]:
    """Every line start L of buf with buf[L] == '@' whose second-next line exists and begins with '+'."""
    ls = line_starts(buf)
    return [ls[i] for i in range(len(ls) - 2) if buf[ls[i]] == 0x40 and buf[ls[i + 2]] == 0x2B]


# quality lines beginning with '@' and with '+', a '+' line repeating the name
THREE = (b"@r0 first\nACGTACGTAC\n+\n@IIIIIIII+\n"
         b"@r1\nGGGTTTAAAC\n+r1\n+@>IIIII@@\n"
         b"@r2\nTTTT\n+\nI@+>\n")
TRUE_STARTS = [0, THREE.index(b"@r1"), THREE.index(b"@r2")]


def test_frontier_reference_scan_finds_the_three_records():
    assert record_starts(THREE) == TRUE_STARTS


def test_frontier_cut_at_every_byte():
    for n in range(len(THREE) + 1):
        buf = THREE[:n]
        off = fk.fastq_frontier(buf)
        want = record_starts(buf)
        if not want:
            assert off == n, (n, off)  # the documented no-record answer
            continue
        # always a true record start of the file, and the last one whose '@' and '+' line starts are visible
        assert off in TRUE_STARTS, (n, off)
        assert off == want[-1], (n, off, want)
    # once both line starts of a record are visible, it is the answer
    for s in TRUE_STARTS:
        plus = THREE.index(b"\n+", s) + 1
        assert fk.fastq_frontier(THREE[:plus + 1]) == s
        assert fk.fastq_frontier(THREE[:plus]) != s


def test_frontier_no_record_cases():
    assert fk.fastq_frontier(b"") == 0
    assert fk.fastq_frontier(b"@r\nACGT\n") == 8          # the '+' line has not begun
    assert fk.fastq_frontier(b"ACGT\n+\nIIII\n") == 12    # no '@' line
    assert fk.fastq_frontier(b"\n\n\n") == 3
    assert fk.fastq_frontier(b"@r\nACGT\n+") == 0
    assert fk.fastq_frontier(b"@r\r\nAC\r\n+\r\nII\r\n@s\r\nAC\r\n+\r\nII") == 15  # CRLF


# ---- the split

def make_fastq(n_reads, lo=30, hi=250, seed=1, crlf=False):
    rng = np.random.default_rng(seed)
    out = []
    eol = b"\r\n" if crlf else b"\n"
    for i in range(n_reads):
        n = int(rng.integers(lo, hi + 1))
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
        qual = bytearray((rng.integers(2, 41, n) + 33).astype(np.uint8).tobytes())
        if n and i % 5 == 0:
            qual[0] = b"@+>"[i // 5 % 3]
        out.append(b"@read%d/1" % i + eol + seq + eol + (b"+read%d/1" % i if i % 7 == 0 else b"+") + eol + bytes(qual) + eol)
    return b"".join(out)


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_split_bytes_fastq_covers_the_file_in_whole_records(tmp_path, world, crlf):
    data = make_fastq(700, crlf=crlf)  # ~200 KB
    assert 150_000 < len(data) < 300_000
    path = tmp_path / "reads.fq"
    path.write_bytes(data)
    starts = set(record_starts(data))
    parts = [fk.split_bytes_fastq(str(path), world, r) for r in range(world)]
    assert b"".join(parts) == data
    pos = 0
    for r, p in enumerate(parts):
        if p:
            assert pos in starts, (world, r, pos)
            # the records whose '@' line starts in the rank's byte range
            first = min(s for s in starts if s >= len(data) * r // world) if r else 0
            assert pos == first, (world, r)
        pos += len(p)
    if world > 1:
        assert sum(1 for p in parts if p) == world  # 700 records: every rank gets some


def test_split_bytes_fastq_file_smaller_than_world(tmp_path):
    data = make_fastq(3, seed=9)
    path = tmp_path / "tiny.fq"
    path.write_bytes(data)
    starts = set(record_starts(data))
    parts = [fk.split_bytes_fastq(str(path), 8, r) for r in range(8)]
    assert b"".join(parts) == data
    pos = 0
    for p in parts:
        assert not p or pos in starts
        pos += len(p)
    assert sum(1 for p in parts if p) <= 3
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    assert [fk.split_bytes_fastq(str(empty), 2, r) for r in range(2)] == [b"", b""]


def test_split_bytes_fastq_errors(tmp_path):
    with pytest.raises(fk.FastKmerError) as e:
        fk.split_bytes_fastq(str(tmp_path / "missing.fq"), 2, 0)
    assert e.value.code == -5
    path = tmp_path / "r.fq"
    path.write_bytes(make_fastq(4))
    for world, rank in ((0, 0), (2, 2), (2, -1)):
        with pytest.raises(fk.FastKmerError) as e:
            fk.split_bytes_fastq(str(path), world, rank)
        assert e.value.code == -1
    n = ctypes.c_size_t()
    buf = ctypes.create_string_buffer(8)
    assert fk.lib().fk_split_bytes_fastq(os.fsencode(str(path)), 1, 0, buf, 8, ctypes.byref(n)) == -6


# ---- Python surface and CLI

def test_python_keywords_default_to_fasta():
    import inspect
    p = inspect.signature(fk.KmerCounter.__init__).parameters
    assert (p["input_format"].default, p["min_quality"].default, p["quality_offset"].default) == ("fasta", 0, 33)
    p = inspect.signature(fk.KmerCounter.set_input_format).parameters
    assert (p["input_format"].default, p["min_quality"].default, p["quality_offset"].default) == ("fasta", 0, 33)
    assert inspect.signature(fk.execute_job).parameters["input_format"].default == "fasta"
    assert callable(fk.KmerCounter.fastq_info)


def test_cli_format_variable():
    ok = [fk.CLI_PATH, "28", "10", "3", "2048", "0", "0", "/nonexistent/in.fq", "out", "p", "0", "0", "0"]
    base = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}
    # a bad value is a usage error, before any input is read
    for bad in ("fastx", "FASTQ", "1"):
        r = subprocess.run(ok, capture_output=True, env=dict(base, FASTKMER_CLI_FORMAT=bad))
        assert r.returncode == 2 and b"usage" in r.stderr and b"FASTKMER_CLI_FORMAT" in r.stderr, bad
    for name, value in (("FASTKMER_CLI_MIN_QUAL", "94"), ("FASTKMER_CLI_MIN_QUAL", "x"), ("FASTKMER_CLI_QUAL_OFFSET", "7")):
        r = subprocess.run(ok, capture_output=True, env=dict(base, **{name: value}))
        assert r.returncode == 1 and b"invalid configuration" in r.stderr and name.encode() in r.stderr
    # unset, and every good value: nothing changes up to the point where the input is opened
    want = subprocess.run(ok, capture_output=True, env=base)
    assert want.returncode == 1 and b"cannot open /nonexistent/in.fq" in want.stderr
    for good in ("fasta", "fastq", "auto", ""):
        r = subprocess.run(ok, capture_output=True, env=dict(base, FASTKMER_CLI_FORMAT=good))
        assert (r.returncode, r.stdout, r.stderr) == (want.returncode, want.stdout, want.stderr), good
    # the errors of the positional contract stay as they are
    r = subprocess.run([fk.CLI_PATH], capture_output=True, env=dict(base, FASTKMER_CLI_FORMAT="fastq"))
    assert r.returncode == 2 and b"usage" in r.stderr
