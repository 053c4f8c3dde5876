"""The database file of a counted result (fk_save / fk_load / fk_db_info_read), as far as no GPU is needed:
the committed format and the header parser.

`golden/store_k21.fkdb` is the database of `golden/edge_bytes_k21.fa` (k = 21, m = 7, B = 64).  It is read
here by a numpy reader written from the format table of INTEGRATION.md ("Saving and loading results"), not
by the library: the reader must give exactly the oracle's (k-mer, count) lists per bin, and the checksum is
recomputed in numpy.  The header parser (fk_db_info_read, host only) is then fed headers it must refuse,
each with the right error code, and is run under the host's address and undefined-behaviour sanitizers in
a stand-alone program (store_header_check.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk
import oracle
from conftest import GOLDEN

DB = os.path.join(GOLDEN, "store_k21.fkdb")
FASTA = os.path.join(GOLDEN, "edge_bytes_k21.fa")
K, M, B = 21, 7, 64
E_INVALID, E_IO = -1, -5
GOLD = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()
    oracle.build()


def mix(x):
    """splitmix64's finaliser on a uint64 array (wrapping)."""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def checksum(key_words, counts):
    """The format's checksum of a key section (uint64 words) and a count section."""
    with np.errstate(over="ignore"):
        i = np.arange(key_words.size, dtype=np.uint64)
        j = np.uint64(1 << 63) + np.arange(counts.size, dtype=np.uint64)
        s = mix(key_words ^ (i * GOLD)).sum(dtype=np.uint64) + mix(counts.astype(np.uint64) ^ (j * GOLD)).sum(dtype=np.uint64)
    return int(s)


def read_db(raw: bytes):
    """The format table, field by field: (header dict, {bin: (key words, counts)})."""
    assert raw[:8] == b"FKMERDB\0"
    version, hb = struct.unpack_from("<II", raw, 8)
    k, m, bins, kw, n_ranks, rank = struct.unpack_from("<6i", raw, 16)
    stored, zero = struct.unpack_from("<II", raw, 40)
    distinct, kmers, cs = struct.unpack_from("<3Q", raw, 48)
    assert version == 1 and zero == 0 and hb % 8 == 0 and hb == 72 + 16 * stored
    table = [struct.unpack_from("<IIQ", raw, 72 + 16 * i) for i in range(stored)]
    assert all(z == 0 for _, z, _ in table)
    keys = np.frombuffer(raw, dtype="<u8", count=distinct * kw, offset=hb)
    counts = np.frombuffer(raw, dtype="<u4", count=distinct, offset=hb + distinct * kw * 8)
    assert len(raw) == hb + distinct * (kw * 8 + 4)
    out, at = {}, 0
    for b, _, n in table:
        out[b] = (keys[at * kw:(at + n) * kw], counts[at:at + n])
        at += n
    assert at == distinct
    head = dict(k=k, m=m, bins=bins, key_words=kw, n_ranks=n_ranks, rank=rank, version=version, stored_bins=stored,
                distinct=distinct, kmers=kmers, checksum=cs, file_bytes=len(raw))
    return head, out, keys, counts


@pytest.fixture(scope="module")
def raw():
    with open(DB, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def ref():
    with open(FASTA, "rb") as f:
        return oracle.OracleResult(f.read(), K, M, B)


def test_db_info_of_the_golden_file(raw, ref):
    info = fk.db_info(DB)
    assert info == read_db(raw)[0]
    assert (info["k"], info["m"], info["bins"], info["key_words"], info["n_ranks"], info["rank"]) == (K, M, B, 1, 1, 0)
    assert info["distinct"] == ref.distinct and info["kmers"] == ref.total_kmers
    assert info["stored_bins"] == int(np.count_nonzero(ref.bin_sizes())) and info["file_bytes"] == len(raw) < 64 << 10


def test_numpy_reader_gives_the_oracle_bins(raw, ref):
    head, bins, keys, counts = read_db(raw)
    assert sorted(bins) == list(bins) == np.nonzero(ref.bin_sizes())[0].tolist()  # the non-empty bins, ascending
    for b, (k, c) in bins.items():
        _, rlo, rcnt = ref.bin_arrays(b)
        assert np.array_equal(k, rlo) and np.array_equal(c, rcnt), f"bin {b}"
    assert checksum(keys, counts) == head["checksum"]
    assert int(counts.sum(dtype=np.uint64)) == head["kmers"]


def _put(raw, off, fmt, *v):
    b = bytearray(raw)
    struct.pack_into(fmt, b, off, *v)
    return bytes(b)


def _swap_bin_entries(raw):
    b = bytearray(raw)
    b[72:88], b[88:104] = raw[88:104], raw[72:88]
    return bytes(b)


HEADER_END = 72 + 16 * 58
REFUSED = [
    ("wrong magic", lambda r: b"FKMERDC\0" + r[8:], E_INVALID, "magic"),
    ("version 2", lambda r: _put(r, 8, "<I", 2), E_INVALID, "version"),
    ("header bytes not a multiple of 8", lambda r: _put(r, 12, "<I", HEADER_END + 4), E_INVALID, "header bytes"),
    ("header bytes against stored_bins", lambda r: _put(r, 40, "<I", 57), E_INVALID, "stored bins"),
    ("bins not ascending", _swap_bin_entries, E_INVALID, "ascend"),
    ("a bin twice", lambda r: r[:88] + r[72:76] + r[92:], E_INVALID, "ascend"),
    ("a bin not below bins", lambda r: _put(r, 72 + 16 * 57, "<I", 64), E_INVALID, "not below"),
    ("sizes not summing to distinct", lambda r: _put(r, 48, "<Q", 1140), E_INVALID, "sum"),
    ("a size that overflows the sum", lambda r: _put(r, 80, "<Q", (1 << 64) - 1), E_INVALID, "overflow"),
    ("key_words contradicts k", lambda r: _put(r, 28, "<i", 2), E_INVALID, "key_words"),
    ("k that contradicts key_words", lambda r: _put(r, 16, "<i", 33), E_INVALID, "key_words"),
    ("one byte short", lambda r: r[:-1], E_IO, "truncated"),
    ("one byte long", lambda r: r + b"\0", E_IO, "trailing bytes"),
] + [(f"truncated at {n}", (lambda n: lambda r: r[:n])(n), E_IO, "truncated")
     for n in (0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64, 72, 76, 80, 88, HEADER_END, HEADER_END + 8 * 1139)]


@pytest.mark.parametrize("name,change,code,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_header_refused(raw, tmp_path, name, change, code, word):
    assert read_db(raw)[0]["stored_bins"] == 58
    p = tmp_path / "bad.fkdb"
    p.write_bytes(change(raw))
    with pytest.raises(fk.FastKmerError) as e:
        fk.db_info(str(p))
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_missing_file_is_an_io_error(tmp_path):
    with pytest.raises(fk.FastKmerError) as e:
        fk.db_info(str(tmp_path / "none.fkdb"))
    assert e.value.code == E_IO and "cannot open" in str(e.value)


def test_header_parser_under_the_host_sanitizers(tmp_path):
    """The parser and a stand-alone program around it, compiled with -fsanitize=address,undefined: every
    truncation and every changed header byte is answered with a known code and no sanitizer report."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "store_header_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(here, "store_header_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), DB, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout and not r.stderr, r.stdout + r.stderr
