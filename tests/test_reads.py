"""Read profiles, the host side (no GPU): fk_reads_csr against a pure-Python cutter written from the
header's sentences, its buffer rules and FASTQ errors, the ctypes / numpy mirrors of fk_read_stat, and
filter_reads on a hand-made statistics array."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk

NEW = ["fk_reads_csr", "fk_read_counts_device", "fk_read_counts", "fk_read_stats_of_counts_device",
       "fk_read_stats_device", "fk_read_stats", "fk_read_stats_scratch_bytes"]
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.fa")))


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def cut_fasta(text: bytes) -> list[bytes]:
    """A non-empty line beginning with '>' opens a read; the lines up to the next one are its bytes
    without their '\\n'; lines before the first header are no sequence."""
    reads = None
    for line in text.split(b"\n"):
        if line[:1] == b">":
            reads = (reads or []) + [b""]
        elif reads:
            reads[-1] += line
    return reads or []


def cut_fastq(text: bytes, min_q=0, q_off=33) -> list[bytes]:
    """Strict four-line records up to the last line with text (blank lines may trail, and complete a
    record whose quality line is empty); the read is the sequence line, masked where the quality is low."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # the last line ended with its '\n' (or the text is empty)
    n_text = max((i + 1 for i, line in enumerate(lines) if line.strip(b"\r")), default=0)
    lines = lines[:-(-n_text // 4) * 4]
    reads = []
    for r in range(0, len(lines), 4):
        rec = lines[r:r + 4]
        seq, qual = (rec[1].rstrip(b"\r"), rec[3].rstrip(b"\r")) if len(rec) == 4 else (b"", b"x")
        if len(rec) < 4 or rec[0][:1] != b"@" or rec[2][:1] != b"+" or len(seq) != len(qual):
            raise ValueError(r // 4)
        masked = bytes(ord("N") if q - q_off < min_q else c for c, q in zip(seq, qual)) if min_q > 0 else seq
        reads.append(masked + rec[1][len(seq):])
    return reads


def as_csr(reads):
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return bases, offsets


def same(got, reads):
    want = as_csr(reads)
    return (got[0].dtype, got[1].dtype) == (np.uint8, np.uint64) and np.array_equal(got[0], want[0]) and \
        np.array_equal(got[1], want[1])


def test_the_new_calls_are_declared_exported_and_bound():
    assert set(NEW) <= set(fk.header_functions())
    out = subprocess.check_output(["nm", "-D", "--defined-only", fk.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported
    L = fk.lib()
    with open(fk.HEADER_PATH) as f:
        text = f.read()
    assert "#define FK_ABI_VERSION 3" in text and L.fk_abi_version() == 3
    assert int(re.search(r"#define FK_READ_TILE (\d+)", text).group(1)) == fk.READ_TILE
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        args = re.search(r"\b%s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(getattr(L, name).argtypes) == len(args.split(",")), name
    assert L.fk_read_stats_scratch_bytes(1000) == 5000 == fk.read_stats_scratch_bytes(1000)


def test_read_stat_mirrors_the_header():
    with open(fk.HEADER_PATH) as f:
        body = re.search(r"typedef struct fk_read_stat \{(.*?)\} fk_read_stat;", f.read(), re.S).group(1)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [n for _, n in fields] == ["windows", "hits", "min", "median", "max", "reserved", "sum"]
    assert [(n, t) for n, t in fk.fk_read_stat._fields_] == [(n, ctype[t]) for t, n in fields]
    assert ctypes.sizeof(fk.fk_read_stat) == 32 == fk.READ_STAT_DTYPE.itemsize
    assert list(fk.READ_STAT_DTYPE.names) == [n for _, n in fields]
    assert [fk.READ_STAT_DTYPE.fields[n][1] for n in fk.READ_STAT_DTYPE.names] == \
        [getattr(fk.fk_read_stat, n).offset for n in fk.READ_STAT_DTYPE.names]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_fasta_golden_files(path):
    with open(path, "rb") as f:
        text = f.read()
    assert same(fk.reads_csr(text), cut_fasta(text))


def test_the_golden_set_covers_the_fasta_edge_cases():
    names = {os.path.basename(p) for p in GOLDEN}
    assert {"crlf_and_junk.fa", "no_records.fa", "empty.fa", "long_record_k28.fa"} <= names
    texts = {n: open(p, "rb").read() for n, p in zip(sorted(names), GOLDEN)}
    assert fk.reads_csr(texts["empty.fa"])[1].tolist() == [0] == fk.reads_csr(texts["no_records.fa"])[1].tolist()
    assert any(13 in fk.reads_csr(t)[0] for t in texts.values())          # a '\r' stays in its read
    assert any(t.count(b"\n") > 2 * t.count(b">") + 2 for t in texts.values())  # multi-line records


def test_fasta_hand_cases():
    for text in (b"", b"\n\n", b"ACGT\nAC", b">", b">\n", b">a", b">a\n>b\n\n>c\nAC\n\nGT", b"AC\n>a\nAC>GT\n >x\nTT\r\n>b\r\nnNRY",
                 b"\n>a\nA\n", b">a\nACGT"):
        assert same(fk.reads_csr(text), cut_fasta(text)), text
    assert cut_fasta(b"AC\n>a\nAC>GT\n >x\nTT\r\n>b\r\nnNRY") == [b"AC>GT >xTT\r", b"nNRY"]
    assert same(fk.reads_csr(">a\nAC\n"), [b"AC"])  # str is encoded


FQ = (b"@r0 first\nACGTACGTAC\n+\n@IIIIIIII+\n"      # a quality line beginning with '@'
      b"@r1\n\n+r1\n\n"                                 # an empty read
      b"@r2\nTTNT\n+\nI#5I\n")
FQ_READS = [b"ACGTACGTAC", b"", b"TTNT"]


def test_fastq_hand_cases():
    assert cut_fastq(FQ) == FQ_READS and same(fk.reads_csr(FQ, "fastq"), FQ_READS)
    assert same(fk.reads_csr(FQ[:-1], "fastq"), FQ_READS)                     # no final newline
    assert same(fk.reads_csr(FQ + b"\n\r\n\n", "fastq"), FQ_READS)             # blank lines trail
    crlf = FQ.replace(b"\n", b"\r\n")
    want = [b"ACGTACGTAC\r", b"\r", b"TTNT\r"]                                 # the '\r' is the count's invalid byte
    assert cut_fastq(crlf) == want and same(fk.reads_csr(crlf, "fastq"), want)
    assert same(fk.reads_csr(crlf[:-2], "fastq"), want)
    assert same(fk.reads_csr(b"@e\n\n+\n\n", "fastq"), [b""])                  # an empty quality line is a line
    assert same(fk.reads_csr(b"", "fastq"), []) and same(fk.reads_csr(b"\n\r\n", "fastq"), [])
    for text in (FQ, FQ[:-1], crlf, b"@e\n\n+\n\n", b"@e\n\n+\n\n\n"):
        assert same(fk.reads_csr(text, "fastq"), cut_fastq(text)), text


def test_fastq_quality_masking_at_both_offsets():
    # scores: '@' 31, 'I' 40, '+' 10 | '#' 2, '5' 20 under offset 33
    assert same(fk.reads_csr(FQ, "fastq", 11, 33), [b"ACGTACGTAN", b"", b"TNNT"])
    assert same(fk.reads_csr(FQ, "fastq", 32, 33), [b"NCGTACGTAN", b"", b"TNNT"])
    assert same(fk.reads_csr(FQ, "fastq", 2, 33), FQ_READS) and same(fk.reads_csr(FQ, "fastq", 3, 33), [FQ_READS[0], b"", b"TNNT"])
    # offset 64: '@' 0, 'I' 9, the others negative
    assert same(fk.reads_csr(FQ, "fastq", 1, 64), [b"NCGTACGTAN", b"", b"TNNT"])
    assert same(fk.reads_csr(FQ, "fastq", 10, 64), [b"N" * 10, b"", b"NNNN"])
    for q, off in ((11, 33), (32, 33), (1, 64), (9, 64), (10, 64)):
        assert same(fk.reads_csr(FQ, "fastq", q, off), cut_fastq(FQ, q, off)), (q, off)
    crlf = FQ.replace(b"\n", b"\r\n")
    assert same(fk.reads_csr(crlf, "fastq", 11, 33), [b"ACGTACGTAN\r", b"\r", b"TNNT\r"])


@pytest.mark.parametrize("text,record", [
    (b"r0\nAC\n+\nII\n" + FQ, 0),                       # no '@'
    (FQ + b"@r3\nAC\n-\nII\n", 3),                      # no '+'
    (FQ + b"@r3\nACG\n+\nII\n@r4\nA\n+\nI\n", 3),       # lengths differ
    (FQ + b"@r3\nAC\n+\nIII\r\n", 3),
    (FQ + b"@r3\nAC\n", 3),                             # the input ends inside a record
    (FQ + b"@r3\nAC\n+\n", 3),                          # ... before a non-empty read's quality line
    (b"@r0\nAC\n\n+\nII\n", 0),                         # a blank line inside
    (b"\n" + FQ, 0),
    (FQ + b"@e\n\n+\n", 3),                            # ... before an empty read's quality line
])
def test_malformed_fastq_names_the_first_record(text, record):
    with pytest.raises(ValueError) as want:
        cut_fastq(text)
    assert want.value.args[0] == record
    with pytest.raises(fk.FastKmerError) as e:
        fk.reads_csr(text, "fastq")
    assert e.value.code == -1 and f"record {record} " in str(e.value)
    nr, nb = ctypes.c_size_t(99), ctypes.c_size_t(99)
    assert fk.lib().fk_reads_csr(text, len(text), 1, 0, 33, None, 0, None, 0, ctypes.byref(nr), ctypes.byref(nb)) == -1
    good = cut_fastq(FQ)[:record] if record else []
    assert (nr.value, nb.value) == (len(good), sum(map(len, good)))


def test_buffer_rules_and_arguments():
    L = fk.lib()
    text = b">a\nACGT\n>b\n\n>c\nGG\n"
    nr, nb = ctypes.c_size_t(99), ctypes.c_size_t(99)
    call = lambda bases, cb, offs, cr: L.fk_reads_csr(text, len(text), 0, 0, 33, bases, cb, offs, cr,
                                                       ctypes.byref(nr), ctypes.byref(nb))
    bases, offs = np.full(8, 7, dtype=np.uint8), np.full(5, 7, dtype=np.uint64)
    for b, o in ((None, None), (bases.ctypes.data, None), (None, offs.ctypes.data)):  # sizing calls
        nr.value = nb.value = 99
        assert call(b, 0, o, 0) == 0 and (nr.value, nb.value) == (3, 6)
    assert (bases == 7).all() and (offs == 7).all()
    assert call(bases.ctypes.data, 6, offs.ctypes.data, 3) == 0
    assert bytes(bases[:6]) == b"ACGTGG" and offs[:4].tolist() == [0, 4, 4, 6] and bases[6] == 7 and offs[4] == 7
    for cb, cr in ((5, 3), (6, 2), (0, 0)):
        nr.value = nb.value = 99
        assert call(bases.ctypes.data, cb, offs.ctypes.data, cr) == -6 and (nr.value, nb.value) == (3, 6)
    assert bases[6] == 7 and offs[4] == 7
    assert L.fk_reads_csr(None, 4, 0, 0, 33, None, 0, None, 0, ctypes.byref(nr), ctypes.byref(nb)) == -1
    assert L.fk_reads_csr(text, len(text), 0, 0, 33, None, 0, None, 0, None, ctypes.byref(nb)) == -1
    for fmt, q, off in ((2, 0, 33), (1, 94, 33), (1, -1, 33), (1, 0, 40)):
        assert L.fk_reads_csr(text, len(text), fmt, q, off, None, 0, None, 0, ctypes.byref(nr), ctypes.byref(nb)) == -1
    with pytest.raises(ValueError):
        fk.reads_csr(text, "fastx")


def test_filter_reads():
    stats = np.zeros(5, dtype=fk.READ_STAT_DTYPE)
    stats["hits"] = [0, 1, 5, 73, 2]
    stats["windows"] = 73
    assert fk.filter_reads(stats).tolist() == [True] * 5
    assert fk.filter_reads(stats, min_hits=1).tolist() == [False, True, True, True, True]
    assert fk.filter_reads(stats, min_hits=2, max_hits=5).tolist() == [False, False, True, False, True]
    assert fk.filter_reads(stats, max_hits=0).tolist() == [True, False, False, False, False]
    assert fk.filter_reads(stats).dtype == bool


def test_python_surface():
    import inspect
    p = inspect.signature(fk.reads_csr).parameters
    assert [p[n].default for n in ("input_format", "min_quality", "quality_offset")] == ["fasta", 0, 33]
    p = inspect.signature(fk.KmerCounter.read_stats).parameters
    assert (p["offsets"].default, p["min_count"].default, p["max_count"].default) == (None, 1, None)
    assert inspect.signature(fk.KmerCounter.read_counts).parameters["return_valid"].default is False
    for name in ("read_counts_ptr", "read_stats_ptr", "read_stats_of_counts_ptr"):
        assert callable(getattr(fk.KmerCounter, name))
